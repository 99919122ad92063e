"""The picture the reference's test loop writes for `--show` / `--show-dir`, on device (segmentation/mmseg_custom/apis/test_bs.py:257-349):
`tensor2imgs` de-normalises the RGB half of the input tensor (test_bs.py:18-63), the result is cropped to `img_shape` (test_bs.py:275-276) and
`show_result` paints the palette over it (tools/color_gt_according_palette.py:23-81): color_seg[seg == label] = color, the channels reversed,
img * (1 - opacity) + color_seg * opacity in float64, .astype(np.uint8).  One launch (csrc/render.hip) from the uint8 class map to the uint8 HWC picture
[B, h, w, 3], the layout mmcv.imwrite takes.

Three source forms: none (show_result on a black image; opacity 1.0 gives the pure palette picture), `raw` (the loaders' uint8 HWC frame: what
tensor2imgs aims to restore, without its rounding losses) and `tensor` (the normalised float32 NCHW tensor the backbone read, de-normalised exactly as
tensor2imgs does it: float32, n * std + mean, one rounding per step, `* 255` when norm_by_max, truncation).  The blend is numpy's three separately rounded
float64 operations; `1 - opacity` is formed here, on the host, as the reference forms it.

One deviation: where tensor2imgs casts a float outside 0..255 to uint8 (C semantics, undefined for negatives) the value saturates to 0 / 255 here.
Out of scope: the `resize_dim` rescale of the picture (test_bs.py:280-285, the identity for every DELIVER config) and writing files.  There is no CPU path."""
import ctypes

import numpy as np
import torch

from . import lib
from . import ops
from .preprocess import _capturing

MAX_PALETTE = 256


class Renderer:
    """`show_result` for a fixed palette and opacity.

    palette: [n, 3] integers in 0..255, n <= 256 -- the reference's `dataset.PALETTE` (RGB).  A missing palette is refused (the reference would draw a
      random one).  A class without an entry, 255 = "uncovered" included, is painted with colour 0, as the reference's zero-initialised color_seg is.
    opacity: in (0, 1], as the reference asserts.
    preprocess: the mmsa.preprocess.Preprocess whose output the `tensor` form de-normalises: mean / std / to_rgb of its first (RGB) modality, and
      `* 255` where that modality was divided by 255 (test_bs.py:265-269 decides that by `np.all(mean <= 1)` over the means of BOTH modalities, which
      undoes the division for DELIVER / FMB and leaves a MUSES RGB + LiDAR picture in 0..1, i.e. black; the flag here is the RGB modality's own).
    bgr: the picture is BGR, the palette's channels reversed as show_result reverses them (what mmcv.imwrite expects); False keeps the palette's order.
    The packed palette is uploaded once per device and kept on the object: later calls with `out=` copy and allocate nothing and can be captured."""

    def __init__(self, palette, opacity=0.5, preprocess=None, bgr=True):
        if palette is None:
            raise ValueError("mmsa.Renderer: a palette is required (the reference draws a random one when the dataset has none; that is not built)")
        pal = np.asarray(palette)
        if pal.ndim != 2 or pal.shape[1] != 3 or pal.dtype.kind not in "iu":
            raise ValueError(f"mmsa.Renderer: the palette must be an [n, 3] integer array, got shape {pal.shape} of {pal.dtype}")
        if not 1 <= pal.shape[0] <= MAX_PALETTE:
            raise ValueError(f"mmsa.Renderer: a palette has 1..{MAX_PALETTE} entries, got {pal.shape[0]}")
        if pal.min() < 0 or pal.max() > 255:
            raise ValueError("mmsa.Renderer: palette values must be in 0..255")
        opacity = float(opacity)
        if not 0 < opacity <= 1.0:
            raise ValueError(f"mmsa.Renderer: opacity {opacity} must be in (0, 1]")
        self.palette = pal.astype(np.uint8)
        p = pal.astype(np.uint32)
        self.packed = np.ascontiguousarray(p[:, 0] | (p[:, 1] << 8) | (p[:, 2] << 16)).view(np.int32)     # the same bits: torch uploads int32
        self.opacity, self.one_minus = opacity, 1 - opacity                                            # the reference's `1 - opacity`, a double
        self.bgr = bool(bgr)
        self.preprocess = preprocess
        if preprocess is not None:
            self._c_mean = (ctypes.c_float * 3)(*preprocess.mean[:3].tolist())
            self._c_std = (ctypes.c_float * 3)(*preprocess.std[:3].tolist())
        self._pal_dev = {}      # device -> packed palette

    def palette_on(self, device):
        device = torch.device(device)
        t = self._pal_dev.get(device)
        if t is None:
            if _capturing(device):
                raise RuntimeError("mmsa.Renderer: the palette is not on the device yet and cannot be uploaded during a graph capture: run one call before capturing")
            t = self._pal_dev[device] = torch.from_numpy(self.packed).to(device)
        return t

    def check_pred(self, pred):
        if not isinstance(pred, torch.Tensor) or not pred.is_cuda:
            raise RuntimeError("mmsa.Renderer: pred must be a GPU tensor (there is no CPU path)")
        if pred.dtype != torch.uint8 or pred.dim() != 3:
            raise RuntimeError(f"mmsa.Renderer: pred must be a uint8 [B, h, w] class map, got {pred.dtype} {tuple(pred.shape)}")
        if pred.numel() == 0 or pred.stride(2) != 1 or pred.stride(1) < pred.shape[2] or (pred.shape[0] > 1 and pred.stride(0) < (pred.shape[1] - 1) * pred.stride(1) + pred.shape[2]):
            raise RuntimeError(f"mmsa.Renderer: pred must have unit stride along a row and rows / images that do not overlap (a crop of a larger map is fine), "
                               f"got shape {tuple(pred.shape)} with strides {pred.stride()}")
        return pred

    @torch.no_grad()
    def __call__(self, pred, source=None, img_shape=None, out=None, source_reverse=False):
        """pred: uint8 class map [B, h, w] (any row / image stride) -> uint8 picture [B, h, w, 3].
        source: None = the colour map alone; a uint8 [B, Hs, Ws, 3] tensor = the raw frames (`source_reverse`: their channels are in the opposite order
          to the picture's; the loaders give BGR, the order of the picture, whatever `to_rgb` made of the tensor); a float32 [B, >= 3, Hs, Ws] tensor = the
          normalised input (needs `preprocess=` at construction).  Hs >= h, Ws >= w: the top-left h x w is used, `img[:h, :w]` of test_bs.py:276.
        img_shape: (h, w) of the frame's meta; it must equal the map's size (the reference's mask indexing fails otherwise).
        out: the picture buffer; with it the call allocates and copies nothing."""
        pred = self.check_pred(pred)
        B, h, w = (int(v) for v in pred.shape)
        if img_shape is not None and (int(img_shape[0]), int(img_shape[1])) != (h, w):
            raise RuntimeError(f"mmsa.Renderer: img_shape {tuple(int(v) for v in img_shape[:2])} differs from the {h} x {w} class map (the reference's "
                               "color_seg[seg == label] needs them equal)")
        form = None
        if source is not None:
            if not isinstance(source, torch.Tensor) or not source.is_cuda:
                raise RuntimeError("mmsa.Renderer: source must be a GPU tensor (there is no CPU path)")
            if source.device != pred.device or not source.is_contiguous() or source.dim() != 4 or source.shape[0] != B:
                raise RuntimeError(f"mmsa.Renderer: source must be a contiguous 4-D tensor of {B} images on {pred.device}, got {tuple(source.shape)} on {source.device}")
            if source.dtype == torch.uint8 and source.shape[3] == 3:
                form, Hs, Ws = "raw", int(source.shape[1]), int(source.shape[2])
            elif source.dtype == torch.float32 and source.shape[1] >= 3:
                form, Hs, Ws = "tensor", int(source.shape[2]), int(source.shape[3])
                if self.preprocess is None:
                    raise RuntimeError("mmsa.Renderer: a normalised float32 source needs the Renderer made with preprocess= (mean, std, to_rgb, norm_by_max)")
            else:
                raise RuntimeError(f"mmsa.Renderer: source must be uint8 [B, H, W, 3] (raw frames) or float32 [B, >= 3, H, W] (the normalised input), got "
                                   f"{source.dtype} {tuple(source.shape)}")
            if Hs < h or Ws < w:
                raise RuntimeError(f"mmsa.Renderer: the {Hs} x {Ws} source is smaller than the {h} x {w} map")
        with torch.cuda.device(pred.device):
            pal = self.palette_on(pred.device)
            if out is None:
                out = torch.empty(B, h, w, 3, dtype=torch.uint8, device=pred.device)
            if tuple(out.shape) != (B, h, w, 3) or out.dtype != torch.uint8 or out.device != pred.device or not out.is_contiguous():
                raise RuntimeError(f"mmsa.Renderer: `out` must be a contiguous uint8 {(B, h, w, 3)} tensor on {pred.device}")
            head = (pred.data_ptr(), pred.stride(0), pred.stride(1), B, h, w, pal.data_ptr(), pal.numel(), int(self.bgr))
            if form == "tensor":
                pp = self.preprocess
                lib.call("mmsa_render_denorm_f32", *head, source.data_ptr(), int(source.shape[1]), Hs, Ws, self._c_mean, self._c_std, int(pp.to_rgb[0]),
                         int(pp.div255[0]), self.opacity, self.one_minus, out.data_ptr(), ops._stream())
            else:
                lib.call("mmsa_render_u8", *head, None if form is None else source.data_ptr(), Hs if form else 0, Ws if form else 0, int(bool(source_reverse)),
                         self.opacity, self.one_minus, out.data_ptr(), ops._stream())
        return out


def raw_source(rgb, H, W):
    """The `raw` source of a class-map call on raw frames: the uint8 RGB frames when they have the map's size, else None."""
    if rgb.dtype == torch.uint8 and (int(rgb.shape[1]), int(rgb.shape[2])) == (H, W):
        return rgb
    return None


def slide_source(render, preprocess, frame, plan, return_map, what):
    """The source `render=` paints over in the slide modes, where no full-size normalised tensor exists with raw frames: the raw uint8 frame of the map's
    size, or the normalised frame itself.  `plan`: the frame's mmsa.inference.MapPlan.  A raw frame of another size (padded, or resized on device) or
    dtype, and a normalised frame under a map rescaled to another size, are refused by name; every refusal comes before any launch."""
    H, W = plan.Ho, plan.Wo
    if not return_map:
        raise RuntimeError(f"mmsa.{what}: render= paints the stored map; drop return_map=False")
    if preprocess is None:
        if plan.rescaled:
            raise RuntimeError(f"mmsa.{what}: render= has no source for the picture: the class map is rescaled to {H} x {W}, the normalised frame has another size "
                               "(raw uint8 frames of the map's size, with preprocess=, are needed)")
        if render.preprocess is None:
            raise RuntimeError(f"mmsa.{what}: render= on a normalised frame needs the Renderer made with preprocess= (mean, std, to_rgb, norm_by_max)")
        return frame
    src = raw_source(frame[0], H, W)
    if src is None:
        raise RuntimeError(f"mmsa.{what}: render= has no source for the picture: the raw frame is {frame[0].dtype} {int(frame[0].shape[1])} x {int(frame[0].shape[2])}, "
                           f"the class map {H} x {W}, and slide mode never writes the full-size normalised frame (uint8 frames of the map's size are needed; "
                           "Resize_multimodal on device / Pad_multimodal / a float32 RGB modality are not)")
    return src


def whole_source(render, rgb, plan, return_map, what):
    """The source in the whole modes -> the raw uint8 frames `rgb` (None without `preprocess=`) where they have the size of the map before its cut, else
    None: the caller paints over the normalised tensor the backbone reads, which exists here -- a padded or device-resized frame, a float32 RGB
    modality, no `preprocess=`.  That tensor is no source for a map resized to another size (a cut alone is fine: its top-left is used)."""
    src = None if rgb is None else raw_source(rgb, plan.Hd, plan.Wd)
    if src is None and plan.resized:
        raise RuntimeError(f"mmsa.{what}: render= has no source for the picture: the class map is rescaled to {plan.Hd} x {plan.Wd}, the input tensor is "
                           f"{plan.H} x {plan.W} (raw uint8 frames of the map's size, with preprocess=, are needed)")
    if not return_map:
        raise RuntimeError(f"mmsa.{what}: render= paints the stored map; drop return_map=False")
    if src is None and render.preprocess is None:
        raise RuntimeError(f"mmsa.{what}: render= on the normalised tensor needs the Renderer made with preprocess= (mean, std, to_rgb, norm_by_max)")
    return src
