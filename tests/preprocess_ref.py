"""numpy float32 restatement of the reference's input pipeline, written from segmentation/mmseg_custom/datasets/pipelines/transform.py
(Pad_multimodal 2934-3010, Normalize_multimodal 2796-2804, Normalize_multimodal_Muses 2680-2694) and mmcv's imnormalize_:

    img = img.copy().astype(np.float32); mean = np.float64(mean); stdinv = 1 / np.float64(std)
    if to_rgb: BGR -> RGB in place;  cv2.subtract(img, mean, img);  cv2.multiply(img, stdinv, img)

on float32 data, i.e. one float32 rounding per step with the float64 scalars converted to the array's depth.  The checker of
tests/test_preprocess_gpu.py (bit-exact) and, against the float64 formula, of tests/test_preprocess_cpu.py.  OpenCV is not involved here."""
import json
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))


def load_cfgs():
    return json.load(open(os.path.join(HERE, "golden", "preprocess_cfgs.json")))["configs"]


def pipeline_of(cfg):
    """The reference config's test_pipeline (list of dicts) rebuilt from the fixture's values."""
    names, ch = cfg["modalities_name"], cfg["modalities_ch"]
    norm = dict(type=cfg["normalize"], mean=cfg["mean"], std=cfg["std"], to_rgb=cfg["to_rgb"], modalities_name=names, modalities_ch=ch, norm_by_max=cfg["norm_by_max"])
    steps = [dict(type=cfg["loader"], modalities_name=names, modalities_ch=ch)]
    if cfg["pad_size"] is not None:
        steps.append(dict(type="Pad_multimodal", size=tuple(cfg["pad_size"]), pad_val=cfg["pad_val"], seg_pad_val=255))
    if cfg["resize"] is not None:
        steps.append(dict(type="Resize_multimodal", img_scale=tuple(cfg["resize"]["img_scale"]), seg_scale=(1024, 1024), keep_ratio=cfg["resize"]["keep_ratio"],
                          modalities_name=names, modalities_ch=ch))
    steps.append(dict(type="MultiScaleFlipAug", img_scale=tuple(cfg["img_scale"]), flip=False,
                      transforms=[norm, dict(type="ImageToTensor", keys=["img"]), dict(type="Collectmod", keys=["img"], modalities_name=names, modalities_ch=ch)]))
    return steps


def sinv_of(std):
    """mmcv.imnormalize_: stdinv = 1 / np.float64(std) on the float32 std array, applied to float32 data."""
    return (1 / np.array(std, dtype=np.float32).astype(np.float64)).astype(np.float32)


def div255_of(variant, norm_by_max, names):
    if not norm_by_max:
        return [False, False]
    return [True, True] if variant == "multimodal" else [n == "rgb" for n in names]      # transform.py:2801-2804 / 2685-2694


def normalize_ref(rgb, aux, mean, std, to_rgb, names, norm_by_max, variant, pad_size=None, pad_val=0):
    """rgb, aux: [B, Hs, Ws, 3] uint8 or float32 -> [B, 6, H, W] float32, every step rounded to float32 once."""
    mean32, sinv32 = np.array(mean, dtype=np.float32), sinv_of(std)
    div = div255_of(variant, norm_by_max, names)
    B, Hs, Ws, _ = rgb.shape
    H, W = (Hs, Ws) if pad_size is None else pad_size
    out = np.empty((B, 6, H, W), dtype=np.float32)
    for m, src in enumerate((rgb, aux)):
        x = np.full((B, H, W, 3), np.float32(pad_val), dtype=np.float32)          # impad: bottom / right, BEFORE the normalisation
        x[:, :Hs, :Ws] = src.astype(np.float32)
        if div[m]:
            x = x / np.float32(255)                                                # `img / 255` on float32 data: a correctly rounded float32 division
        if to_rgb[m]:
            x = x[..., ::-1]
        y = (x - mean32[3 * m:3 * m + 3]) * sinv32[3 * m:3 * m + 3]                # cv2.subtract, cv2.multiply
        assert y.dtype == np.float32
        out[:, 3 * m:3 * m + 3] = y.transpose(0, 3, 1, 2)                          # ImageToTensor
    return out
