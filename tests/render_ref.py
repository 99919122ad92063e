"""numpy restatement of the picture the reference's test loop writes for `--show` / `--show-dir`, written from
segmentation/mmseg_custom/apis/test_bs.py (tensor2imgs 18-63, the crop to img_shape 275-276), mmcv.imdenormalize

    mean, std -> float64 (1, 3);  img = cv2.multiply(img, std);  cv2.add(img, mean, img);  if to_bgr: cv2.cvtColor(img, cv2.COLOR_RGB2BGR, img)

on float32 data (one float32 rounding per step, the scalars converted to the array's depth -- NOT verified against OpenCV: cv2.multiply / cv2.add are
taken to round once each), and segmentation/tools/color_gt_according_palette.py:23-81 (show_result).  The checker of tests/test_render_gpu.py
(bit for bit) and, against integer and rational arithmetic, of tests/test_render_cpu.py.  OpenCV is not involved here.

One deviation from the reference, shared with the device code: `.astype(np.uint8)` of a float outside 0..255 (C semantics, undefined for negatives)
saturates to 0 / 255 here, and NaN gives 0."""
import numpy as np


def to_u8(x):
    """float -> uint8 by truncation, saturating."""
    x = np.asarray(x)
    with np.errstate(invalid="ignore"):
        return np.where(x >= 255, 255, np.where(x > 0, np.trunc(x), 0)).astype(np.uint8)


def tensor2imgs_ref(tensor, mean, std, to_rgb, norm_by_max):
    """test_bs.py:18-63 on planes 0..2 (test_bs.py:262) of a float32 [B, C, H, W] array -> uint8 [B, H, W, 3]."""
    img = np.asarray(tensor, dtype=np.float32)[:, :3].transpose(0, 2, 3, 1)
    mean32, std32 = np.array(mean[:3], dtype=np.float32), np.array(std[:3], dtype=np.float32)
    d = img * std32                   # cv2.multiply
    d = d + mean32                    # cv2.add
    assert d.dtype == np.float32
    if to_rgb:
        d = d[..., ::-1]              # cv2.cvtColor(RGB2BGR)
    if norm_by_max:
        d = d * np.float32(255)       # test_bs.py:59 `img * 255` on float32 data
    return np.ascontiguousarray(to_u8(d))


def blend(img, color_seg, opacity):
    """color_gt_according_palette.py:67-68: uint8 arrays -> float64 products and sum, each rounded -> uint8."""
    out = img * (1 - opacity) + color_seg * opacity
    assert out.dtype == np.float64
    return out.astype(np.uint8)


def show_result_ref(img, seg, palette, opacity=0.5, bgr=True):
    """color_gt_according_palette.py:56-68 for one image: img uint8 [h, w, 3], seg [h, w] -> uint8 [h, w, 3].  `bgr=False` skips the channel reversal."""
    palette = np.array(palette)
    assert palette.shape[1] == 3 and len(palette.shape) == 2 and 0 < opacity <= 1.0
    color_seg = np.zeros((seg.shape[0], seg.shape[1], 3), dtype=np.uint8)
    for label, color in enumerate(palette):
        color_seg[seg == label, :] = color
    if bgr:
        color_seg = color_seg[..., ::-1]
    return blend(img, color_seg, opacity)


def render_ref(pred, palette, opacity, source=None, bgr=True):
    """pred uint8 [B, h, w]; source: None (a black image) or uint8 [B, Hs, Ws, 3] pictures (raw frames, or tensor2imgs_ref's) -> uint8 [B, h, w, 3]."""
    B, h, w = pred.shape
    out = np.empty((B, h, w, 3), dtype=np.uint8)
    for b in range(B):
        img = np.zeros((h, w, 3), dtype=np.uint8) if source is None else source[b][:h, :w, :]      # test_bs.py:275-276
        out[b] = show_result_ref(img, pred[b], palette, opacity, bgr=bgr)
    return out
