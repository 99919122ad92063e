"""numpy restatement of the resize the reference's test pipelines start with: `Resize_multimodal._resize_multimodal`
(segmentation/mmseg_custom/datasets/pipelines/transform.py:1136-1167) calls mmcv.imrescale (keep_ratio) / mmcv.imresize per 3-channel slice of the
concatenated HWC array = cv2.resize(slice, (new_w, new_h), interpolation=cv2.INTER_LINEAR).  Written from the algorithm OpenCV publishes in
resize.cpp (stated, not copied):

  per axis   inv = double(n_dst) / n_src; scale = 1.0 / inv; f = float32((d + 0.5) * scale - 0.5) (evaluated in double, rounded once);
             s = floor(f); f -= s; s < 0 -> (0, 0); s >= n_src - 1 -> (n_src - 1, 0), the second tap is then the same pixel.
  uint8      a0 = round_half_even((1 - f) * 2048), a1 = round_half_even(f * 2048) as int16 (rows: b0, b1); D = S[s] * a0 + S[s + 1] * a1 in int32;
             dst = (((b0 * (D0 >> 4)) >> 16) + ((b1 * (D1 >> 4)) >> 16) + 2) >> 2.
  float32    D = S[s] * (1 - f) + S[s + 1] * f; dst = D0 * (1 - fy) + D1 * fy; every product and sum rounded to float32 once.

The loaders concatenate the modalities into one array (loading.py:225), so a pair with one float32 modality is float32 as a whole: the fixed-point
path applies only when BOTH sources are uint8.  OpenCV turns INTER_LINEAR into its 2 x 2 area average when both scale factors are exactly 2: refused.
The checker of tests/test_preprocess_resize_gpu.py (bit-exact); tests/test_preprocess_resize_cpu.py holds it to a derived bound of the exact bilinear
value.  OpenCV itself is not involved here (it is not installed where this is built)."""
import json
import os

import numpy as np

from tests import preprocess_ref as PR

HERE = os.path.dirname(os.path.abspath(__file__))
COEF_BITS = 11          # INTER_RESIZE_COEF_BITS: coefficients are scaled by 2048


def load_cfgs():
    return json.load(open(os.path.join(HERE, "golden", "preprocess_resize_cfgs.json")))["configs"]


def pipeline_of(cfg):
    """The reference config's test_pipeline (list of dicts) rebuilt from the fixture's values, the Resize_multimodal step FIRST as in the configs."""
    names, ch = cfg["modalities_name"], cfg["modalities_ch"]
    norm = dict(type=cfg["normalize"], mean=cfg["mean"], std=cfg["std"], to_rgb=cfg["to_rgb"], modalities_name=names, modalities_ch=ch, norm_by_max=cfg["norm_by_max"])
    steps = [dict(type=cfg["loader"], modalities_name=names, modalities_ch=ch)]
    if cfg["resize"] is not None:
        steps.append(dict(type="Resize_multimodal", img_scale=tuple(cfg["resize"]["img_scale"]), seg_scale=tuple(cfg["resize"]["img_scale"]),
                          keep_ratio=cfg["resize"]["keep_ratio"], modalities_name=names, modalities_ch=ch))
    if cfg["pad_size"] is not None:
        steps.append(dict(type="Pad_multimodal", size=tuple(cfg["pad_size"]), pad_val=cfg["pad_val"], seg_pad_val=255))
    steps.append(dict(type="MultiScaleFlipAug", img_scale=tuple(cfg["img_scale"]), flip=False,
                      transforms=[norm, dict(type="ImageToTensor", keys=["img"]), dict(type="Collectmod", keys=["img"], modalities_name=names, modalities_ch=ch)]))
    return steps


def new_size(Hs, Ws, img_scale, keep_ratio):
    """(new_h, new_w): mmcv.rescale_size for keep_ratio (the largest size inside (long edge, short edge), int(x * f + 0.5)), else img_scale = (w, h)."""
    if not keep_ratio:
        return int(img_scale[1]), int(img_scale[0])
    f = min(max(img_scale) / max(Hs, Ws), min(img_scale) / min(Hs, Ws))
    return int(Hs * float(f) + 0.5), int(Ws * float(f) + 0.5)


def axis_taps(n_src, n_dst):
    """(s int32 [n_dst], f float32 [n_dst]) of one axis."""
    inv = np.float64(n_dst) / np.float64(n_src)
    scale = np.float64(1.0) / inv
    f = ((np.arange(n_dst, dtype=np.float64) + 0.5) * scale - 0.5).astype(np.float32)
    s = np.floor(f).astype(np.int32)
    f = f - s.astype(np.float32)
    assert f.dtype == np.float32
    low, high = s < 0, s >= n_src - 1
    s[low], f[low] = 0, 0
    s[high], f[high] = n_src - 1, 0
    return s, f


def fixed_coefs(f):
    """int16 [n, 2]: round-half-even of (1 - f) * 2048 and f * 2048 (both products are exact in float32)."""
    one = np.float32(1 << COEF_BITS)
    return np.stack([np.rint((np.float32(1) - f) * one), np.rint(f * one)], 1).astype(np.int16)


def float_coefs(f):
    return np.stack([np.float32(1) - f, f], 1).astype(np.float32)


def refuse_area(Hs, Ws, new_h, new_w):
    if Hs == 2 * new_h and Ws == 2 * new_w:
        raise NotImplementedError("cv2.resize INTER_LINEAR with both scale factors exactly 2 is OpenCV's 2 x 2 area average (INTER_AREA), another function")


def resize_u8(img, new_h, new_w):
    """[..., Hs, Ws, C] uint8 -> [..., new_h, new_w, C] uint8, the 8-bit fixed-point path."""
    assert img.dtype == np.uint8
    Hs, Ws = img.shape[-3], img.shape[-2]
    refuse_area(Hs, Ws, new_h, new_w)
    ys, fy = axis_taps(Hs, new_h)
    xs, fx = axis_taps(Ws, new_w)
    a, b = fixed_coefs(fx).astype(np.int32), fixed_coefs(fy).astype(np.int32)
    S = img.astype(np.int32)
    x1, y1 = np.minimum(xs + 1, Ws - 1), np.minimum(ys + 1, Hs - 1)
    D = S[..., xs, :] * a[:, 0, None] + S[..., x1, :] * a[:, 1, None]                  # [..., Hs, new_w, C] int32
    D0, D1 = D[..., ys, :, :] >> 4, D[..., y1, :, :] >> 4
    out = (((b[:, 0, None, None] * D0) >> 16) + ((b[:, 1, None, None] * D1) >> 16) + 2) >> 2
    assert out.min() >= 0 and out.max() <= 255
    return out.astype(np.uint8)


def resize_f32(img, new_h, new_w):
    """[..., Hs, Ws, C] float32 (or uint8, converted exactly) -> float32, one rounding per product and sum."""
    Hs, Ws = img.shape[-3], img.shape[-2]
    refuse_area(Hs, Ws, new_h, new_w)
    ys, fy = axis_taps(Hs, new_h)
    xs, fx = axis_taps(Ws, new_w)
    a, b = float_coefs(fx), float_coefs(fy)
    S = img.astype(np.float32)
    x1, y1 = np.minimum(xs + 1, Ws - 1), np.minimum(ys + 1, Hs - 1)
    D = S[..., xs, :] * a[:, 0, None] + S[..., x1, :] * a[:, 1, None]
    out = D[..., ys, :, :] * b[:, 0, None, None] + D[..., y1, :, :] * b[:, 1, None, None]
    assert out.dtype == np.float32
    return out


def resize_pair(rgb, aux, new_h, new_w):
    """The two modalities as the reference's resize sees them: both uint8 -> fixed point; otherwise both on the float32 path."""
    if rgb.dtype == np.uint8 and aux.dtype == np.uint8:
        return resize_u8(rgb, new_h, new_w), resize_u8(aux, new_h, new_w)
    return resize_f32(rgb, new_h, new_w), resize_f32(aux, new_h, new_w)


def pipeline_ref(rgb, aux, resize, mean, std, to_rgb, names, norm_by_max, variant, pad_size=None, pad_val=0):
    """resize -> pad -> normalise -> CHW: [B, Hs, Ws, 3] x 2 -> [B, 6, H, W] float32.  `resize` = dict(img_scale=(w, h), keep_ratio=...)."""
    Hs, Ws = rgb.shape[1:3]
    nh, nw = new_size(Hs, Ws, resize["img_scale"], resize["keep_ratio"])
    if (nh, nw) != (Hs, Ws):
        rgb, aux = resize_pair(rgb, aux, nh, nw)
    return PR.normalize_ref(rgb, aux, mean, std, to_rgb, names, norm_by_max, variant, pad_size=pad_size, pad_val=pad_val)
