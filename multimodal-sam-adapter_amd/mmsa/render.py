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
        self._tab_dev = {}      # (method, options, device) -> packed paint table of a diagnostic picture

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

    def check_source(self, source, B, h, w, device):
        """The source of a [B, h, w] picture -> (form, Hs, Ws): form None (no source), "raw" or "tensor"."""
        form, Hs, Ws = None, 0, 0
        if source is not None:
            if not isinstance(source, torch.Tensor) or not source.is_cuda:
                raise RuntimeError("mmsa.Renderer: source must be a GPU tensor (there is no CPU path)")
            if source.device != device or not source.is_contiguous() or source.dim() != 4 or source.shape[0] != B:
                raise RuntimeError(f"mmsa.Renderer: source must be a contiguous 4-D tensor of {B} images on {device}, got {tuple(source.shape)} on {source.device}")
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
        return form, Hs, Ws

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
        form, Hs, Ws = self.check_source(source, B, h, w, pred.device)
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

    # ---- diagnostic pictures (csrc/render_diag.hip): ONE paint per pixel from a packed table, then the blend of __call__ ----
    def palette_colour(self, code):
        """The palette's colour of a code (RGB); a code without an entry has colour 0, as in __call__."""
        return tuple(int(v) for v in self.palette[code]) if 0 <= code < self.palette.shape[0] else (0, 0, 0)

    def paint(self, what, code=0, mark=False):
        """One table entry: `what` = None (leave the source), an RGB triple, or "pred" / "label" (the palette's colour of `code`)."""
        if what is None:
            return 0
        return pack_paint(self.palette_colour(code) if isinstance(what, str) else what, self.bgr, mark)

    def labels_table(self, num_classes, ignored=(0, 0, 0)):
        """[C + 1]: the palette's colour of every class, then `ignored` (kept labels out of range and ignored ones)."""
        ignored = _paint_spec(ignored, "ignored", ())
        return np.array([self.paint("label", k) for k in range(num_classes)] + [self.paint(ignored)], dtype=np.uint32)

    def errors_table(self, wrong=(255, 0, 0), correct=None, ignored=None):
        """[513]: entry 0 = ignored; 1 + pred = correct; 257 + code = wrong (MARKED), the code being the label's for "label", else the prediction's."""
        wrong, correct, ignored = _paint_spec(wrong, "wrong", ("label", "pred"), none=False), _paint_spec(correct, "correct", ("pred",)), _paint_spec(ignored, "ignored", ())
        return np.array([self.paint(ignored)] + [self.paint(correct, k) for k in range(256)] + [self.paint(wrong, k, mark=True) for k in range(256)], dtype=np.uint32)

    def heat_table(self, colormap):
        """[N]: one opaque-by-`opacity` paint per bin."""
        return np.array([self.paint(c) for c in _check_colormap(colormap, "colormap")], dtype=np.uint32)

    def abstained_table(self, bins, colour=(0, 0, 0)):
        """[256 + bins]: the palette as __call__ paints it, then the MARKED colour of every bin below min_bin (one triple, or a [bins, 3] colormap)."""
        cols = _abstained_colours(bins, colour)
        return np.array([self.paint("pred", k) for k in range(256)] + [self.paint(col, mark=True) for col in cols], dtype=np.uint32)

    def band_table(self, colour=(255, 255, 255), inside="pred"):
        """[512]: code -> the MARKED paint of a band pixel, then 256 + code -> the paint of the others."""
        colour, inside = _paint_spec(colour, "colour", ("pred", "label"), none=False), _paint_spec(inside, "inside", ("pred", "label"))
        return np.array([self.paint(colour, k, mark=True) for k in range(256)] + [self.paint(inside, k) for k in range(256)], dtype=np.uint32)

    def table_on(self, key, make, device):
        """The packed table of (method, options) on `device`: built and uploaded once, then the same tensor."""
        key = key + (torch.device(device),)
        t = self._tab_dev.get(key)
        if t is None:
            if _capturing(key[-1]):
                raise RuntimeError(f"mmsa.Renderer: the paint table of `{key[0]}` is not on the device yet and cannot be uploaded during a graph capture: run one "
                                   "call with these options before capturing")
            t = self._tab_dev[key] = torch.from_numpy(np.ascontiguousarray(make()).view(np.int32)).to(key[-1])
        return t

    def _picture(self, entry, head, table, B, h, w, device, source, source_reverse, mark_opacity, out):
        """The shared tail of every diagnostic entry: source, weights and `out` checked, then ONE launch."""
        mark_opacity = float(mark_opacity)
        if not 0 < mark_opacity <= 1.0:
            raise ValueError(f"mmsa.Renderer: mark_opacity {mark_opacity} must be in (0, 1]")
        form, Hs, Ws = self.check_source(source, B, h, w, device)
        if out is None:
            out = torch.empty(B, h, w, 3, dtype=torch.uint8, device=device)
        if not isinstance(out, torch.Tensor) or tuple(out.shape) != (B, h, w, 3) or out.dtype != torch.uint8 or out.device != device or not out.is_contiguous():
            raise RuntimeError(f"mmsa.Renderer: `out` must be a contiguous uint8 {(B, h, w, 3)} tensor on {device}")
        pp = self.preprocess
        tensor = form == "tensor"
        lib.call(entry, *head, table.data_ptr(), table.numel(), None if form is None else source.data_ptr(), {None: 0, "raw": 1, "tensor": 2}[form],
                 int(source.shape[1]) if tensor else 0, Hs, Ws, int(bool(source_reverse)), self._c_mean if tensor else None, self._c_std if tensor else None,
                 int(pp.to_rgb[0]) if tensor else 0, int(pp.div255[0]) if tensor else 0, self.opacity, self.one_minus, mark_opacity, 1 - mark_opacity,
                 out.data_ptr(), ops._stream())
        return out

    @staticmethod
    def _label_dims(labels, prep):
        if prep is None:
            raise ValueError("mmsa.Renderer: labels need prep= (the mmsa.LabelPrep that reads them)")
        labels = prep.check(labels)
        H, W = prep.resized(int(labels.shape[1]), int(labels.shape[2]))
        return labels, int(labels.shape[0]), int(H), int(W)

    @torch.no_grad()
    def labels(self, labels, prep, source=None, ignored=(0, 0, 0), out=None, source_reverse=False):
        """The ground-truth picture (what tools/color_gt_according_palette.py paints through show_result): raw uint8 labels [B, Hl, Wl] read through `prep`
        (LUT, and the nearest-neighbour tables where prep resizes) -> uint8 [B, h, w, 3].  A class gets its palette colour; a kept label out of range and
        an ignored one get `ignored` (a triple or None; colour 0 by default: the zero-initialised color_seg)."""
        labels, B, h, w = self._label_dims(labels, prep)
        C = _check_classes(prep.num_classes, 254, "labels")
        _paint_spec(ignored, "ignored", ())
        la = prep.launch_args(labels, B, h, w, labels.device)
        with torch.cuda.device(labels.device):
            tab = self.table_on(("labels", C, _key(ignored)), lambda: self.labels_table(C, ignored), labels.device)
            head = (None, 0, 0, la[0], B, h, w, la[1], la[2], la[3], C, la[4], la[5], 0, 0)
            return self._picture("mmsa_render_labels_u8", head, tab, B, h, w, labels.device, source, source_reverse, 1.0, out)

    @torch.no_grad()
    def errors(self, pred, labels, prep, source=None, wrong=(255, 0, 0), correct=None, ignored=None, mark_opacity=1.0, out=None, source_reverse=False):
        """The wrong-pixel picture.  With L the label code (a class < C, C = kept but out of range, 255 = ignored): a pixel is ignored iff L == 255, correct
        iff L < C and pred == L, wrong otherwise (L == C and pred == 255 included, as Evaluator counts them).  `wrong`: a triple, "label" or "pred", MARKED
        (blended with `mark_opacity`); `correct`: None, a triple or "pred"; `ignored`: None or a triple (both blended with the Renderer's opacity)."""
        pred = self.check_pred(pred)
        B, h, w = (int(v) for v in pred.shape)
        if prep is None:
            raise ValueError("mmsa.Renderer: labels need prep= (the mmsa.LabelPrep that reads them)")
        C = _check_classes(prep.num_classes, 254, "errors")
        _paint_spec(wrong, "wrong", ("label", "pred"), none=False), _paint_spec(correct, "correct", ("pred",)), _paint_spec(ignored, "ignored", ())
        la = prep.launch_args(labels, B, h, w, pred.device)
        with torch.cuda.device(pred.device):
            tab = self.table_on(("errors", _key(wrong), _key(correct), _key(ignored)), lambda: self.errors_table(wrong, correct, ignored), pred.device)
            head = (pred.data_ptr(), pred.stride(0), pred.stride(1), la[0], B, h, w, la[1], la[2], la[3], C, la[4], la[5], 1, int(isinstance(wrong, str) and wrong == "label"))
            return self._picture("mmsa_render_labels_u8", head, tab, B, h, w, pred.device, source, source_reverse, mark_opacity, out)

    @staticmethod
    def _check_values(values, what, shape=None, device=None):
        if not isinstance(values, torch.Tensor) or not values.is_cuda:
            raise RuntimeError(f"mmsa.Renderer: {what} must be a GPU tensor (there is no CPU path)")
        if values.dtype != torch.float32 or values.dim() != 3 or not values.is_contiguous() or values.numel() == 0:
            raise RuntimeError(f"mmsa.Renderer: {what} must be a contiguous float32 [B, h, w] map, got {values.dtype} {tuple(values.shape)}")
        if shape is not None and (tuple(values.shape) != tuple(shape) or values.device != device):
            raise RuntimeError(f"mmsa.Renderer: {what} has shape {tuple(values.shape)} on {values.device}, pred is {tuple(shape)} on {device}")
        return values

    @torch.no_grad()
    def heat(self, values, colormap, source=None, out=None, source_reverse=False):
        """The heat map of any float32 [B, h, w] score (a confidence / margin / entropy map, a probs[r] plane): the pixel gets colormap[k], k the bin of
        the value among N = len(colormap) bins by the clamp and the ONE float32 product of the calibration bins (NaN / negatives -> bin 0, above 1 ->
        bin N - 1), blended with the Renderer's opacity.  colormap: [N, 3] integers, 1 <= N <= 256 (`mmsa.render.HEAT`, `mmsa.render.colormap`)."""
        values = self._check_values(values, "values")
        B, h, w = (int(v) for v in values.shape)
        key = ("heat", _key(colormap))
        if key + (values.device,) not in self._tab_dev:
            _check_colormap(colormap, "colormap")                       # a colormap seen before was checked then: later calls only hash its bytes
        with torch.cuda.device(values.device):
            tab = self.table_on(key, lambda: self.heat_table(colormap), values.device)
            head = (values.data_ptr(), None, 0, 0, B, h, w, tab.numel(), 0)
            return self._picture("mmsa_render_values_f32", head, tab, B, h, w, values.device, source, source_reverse, 1.0, out)

    @torch.no_grad()
    def abstained(self, pred, conf, bins, min_bin=None, threshold=None, colour=(0, 0, 0), mark_opacity=1.0, source=None, out=None, source_reverse=False):
        """The picture of `mmsa.abstain(pred, conf, bins, min_bin)` without writing that map: a pixel whose confidence bin is >= min_bin is painted as
        __call__ paints it, the others get `colour`, MARKED: a triple, or a [bins, 3] colormap indexed by the pixel's bin.  Same clamp, bin and
        `threshold=` rule (a bin edge) as mmsa.abstain."""
        from . import evaluate as ev
        pred = self.check_pred(pred)
        B, h, w = (int(v) for v in pred.shape)
        conf = self._check_values(conf, "conf", pred.shape, pred.device)
        K = ev._check_bins(bins)
        if (min_bin is None) == (threshold is None):
            raise ValueError("mmsa.Renderer: abstained takes min_bin= or threshold=, one of them")
        if threshold is not None:
            min_bin = ev.threshold_bin(threshold, K)
        if isinstance(min_bin, bool) or not isinstance(min_bin, (int, np.integer)) or not 0 <= int(min_bin) <= K:
            raise ValueError(f"mmsa.Renderer: min_bin = {min_bin!r}; 0..{K} for {K} bins ({K} abstains everywhere)")
        key = ("abstained", K, _key(colour))
        if key + (pred.device,) not in self._tab_dev:
            _abstained_colours(K, colour)
        with torch.cuda.device(pred.device):
            tab = self.table_on(key, lambda: self.abstained_table(K, colour), pred.device)
            head = (conf.data_ptr(), pred.data_ptr(), pred.stride(0), pred.stride(1), B, h, w, K, int(min_bin))
            return self._picture("mmsa_render_values_f32", head, tab, B, h, w, pred.device, source, source_reverse, mark_opacity, out)

    @torch.no_grad()
    def band(self, pred=None, labels=None, prep=None, radius=1, border=False, colour=(255, 255, 255), inside="pred", where="pred", mark_opacity=1.0,
             num_classes=None, source=None, out=None, source_reverse=False):
        """The picture of the boundary band.  near_pred / near_label are EXACTLY mmsa.boundary_counts' (Chebyshev `radius` 1..32, clamp-to-edge, the
        zero-padded rule for border=True, an ignored label a code like any other), with P = min(pred, C), C = prep.num_classes, else num_classes, else the
        palette's length (C <= 253).  `where`: "pred" (the contours of the prediction), "label" (the trimap band of the ground truth) or "both" (their
        union); a pixel whose own label is ignored is never marked.  Marked pixels get `colour`, MARKED (a triple, "pred" or "label": the palette's colour of
        the pixel's code P / L); the others get `inside` (None, "pred", "label" or a triple)."""
        from . import evaluate as ev
        if pred is None and labels is None:
            raise ValueError("mmsa.Renderer: band needs pred=, labels= or both")
        if where not in WHERE:
            raise ValueError(f"mmsa.Renderer: where = {where!r}; 'pred', 'label' or 'both'")
        radius = ev.check_boundary_radius(radius, "mmsa.Renderer")
        _paint_spec(colour, "colour", ("pred", "label"), none=False), _paint_spec(inside, "inside", ("pred", "label"))
        for name, what in (("where", where), ("colour", colour), ("inside", inside)):
            if isinstance(what, str) and what in ("label", "both") and labels is None:
                raise ValueError(f"mmsa.Renderer: band {name}={what!r} needs labels=")
            if isinstance(what, str) and what in ("pred", "both") and pred is None:
                raise ValueError(f"mmsa.Renderer: band {name}={what!r} needs pred=")
        if pred is not None:
            pred = self.check_pred(pred)
            B, h, w = (int(v) for v in pred.shape)
            device = pred.device
        else:
            labels, B, h, w = self._label_dims(labels, prep)
            device = labels.device
        if labels is not None and prep is None:
            raise ValueError("mmsa.Renderer: labels need prep= (the mmsa.LabelPrep that reads them)")
        C = prep.num_classes if prep is not None else (int(num_classes) if num_classes is not None else int(self.palette.shape[0]))
        C = _check_classes(C, MAX_BAND_CLASSES, "band")
        la = prep.launch_args(labels, B, h, w, device) if labels is not None else (None, 0, 0, None, None, None)
        with torch.cuda.device(device):
            tab = self.table_on(("band", _key(colour), _key(inside)), lambda: self.band_table(colour, inside), device)
            head = ((None, 0, 0) if pred is None else (pred.data_ptr(), pred.stride(0), pred.stride(1))) + (
                la[0], B, h, w, la[1], la[2], la[3], C, la[4], la[5], radius, 1 if border else 0, WHERE[where], int(isinstance(colour, str) and colour == "label"), int(isinstance(inside, str) and inside == "label"))
            return self._picture("mmsa_render_band_u8", head, tab, B, h, w, device, source, source_reverse, mark_opacity, out)


PAINT, MARK = 1 << 24, 1 << 25      # bits of a paint-table entry above the 24 colour bits (csrc/render_diag.hip)
WHERE = {"pred": 1, "label": 2, "both": 3}
MAX_BAND_CLASSES = 253              # the band kernel marks a mixed window with the byte 0xFE: codes <= C must stay below it


def pack_paint(rgb, bgr, mark=False):
    """An RGB triple -> a table entry in the picture's channel order (`bgr`: reversed, as show_result reverses the palette), PAINT set, MARK on demand."""
    r, g, b = (int(v) for v in rgb)
    c0, c2 = (b, r) if bgr else (r, b)
    return c0 | (g << 8) | (c2 << 16) | PAINT | (MARK if mark else 0)


def _triple(c, name):
    a = np.asarray(c)
    if a.shape != (3,) or a.dtype.kind not in "iu" or a.min() < 0 or a.max() > 255:
        raise ValueError(f"mmsa.Renderer: {name} = {c!r}; an RGB triple of integers in 0..255 is expected")
    return tuple(int(v) for v in a)


def _paint_spec(what, name, words, none=True):
    """A paint argument -> None, a word of `words` or an RGB tuple; anything else is refused by name."""
    if what is None:
        if not none:
            raise ValueError(f"mmsa.Renderer: {name} = None; a colour is required")
        return None
    if isinstance(what, str):
        if what not in words:
            allowed = ", ".join(repr(v) for v in words) + (" or " if words else "") + "an RGB triple" + (" or None" if none else "")
            raise ValueError(f"mmsa.Renderer: {name} = {what!r}; {allowed} is expected")
        return what
    return _triple(what, name)


def _check_colormap(colormap, name):
    a = np.asarray(colormap)
    if a.ndim != 2 or a.shape[1] != 3 or a.dtype.kind not in "iu":
        raise ValueError(f"mmsa.Renderer: {name} must be an [N, 3] integer array, got shape {a.shape} of {a.dtype}")
    if not 1 <= a.shape[0] <= MAX_PALETTE:
        raise ValueError(f"mmsa.Renderer: {name} has {a.shape[0]} rows; 1..{MAX_PALETTE} are supported")
    if a.min() < 0 or a.max() > 255:
        raise ValueError(f"mmsa.Renderer: {name} values must be in 0..255")
    return [tuple(int(v) for v in row) for row in a]


def _abstained_colours(bins, colour):
    """`colour=` of `abstained` -> one RGB tuple per bin: a triple for all of them, or the rows of a [bins, 3] colormap."""
    if np.asarray(colour).ndim == 2:
        cols = _check_colormap(colour, "colour")
        if len(cols) != bins:
            raise ValueError(f"mmsa.Renderer: the colormap of the abstained pixels has {len(cols)} rows for {bins} bins")
        return cols
    return [_paint_spec(colour, "colour", (), none=False)] * bins


def _check_classes(C, most, what):
    if not 1 <= int(C) <= most:
        raise ValueError(f"mmsa.Renderer: {what} with {C} classes; 1..{most} are supported" + (" (the band kernel's 'mixed' byte is 0xFE)" if most == MAX_BAND_CLASSES else ""))
    return int(C)


def _key(what):
    """A hashable form of a paint argument for the table cache."""
    if what is None or isinstance(what, str):
        return what
    a = np.asarray(what)
    return (a.shape, a.dtype.str, a.tobytes())


def colormap(stops, n):
    """An integer piecewise-linear ramp: `n` RGB rows through the `stops` (>= 1 RGB triples at equal spacing), entry 0 = the first stop, entry n - 1 = the
    last (n == 1: the first).  Every channel is the exact rational value rounded half up by integer arithmetic alone -- no floats, so the table is the same
    on every machine.  -> uint8 [n, 3]."""
    st = [_triple(s, "a colormap stop") for s in stops]
    if isinstance(n, bool) or not isinstance(n, (int, np.integer)) or not 1 <= int(n) <= MAX_PALETTE or not st:
        raise ValueError(f"mmsa.render.colormap: n = {n!r} rows through {len(st)} stops; 1..{MAX_PALETTE} rows and at least one stop are expected")
    n, S = int(n), len(st)
    out = np.zeros((n, 3), dtype=np.uint8)
    for i in range(n):
        if n == 1 or S == 1:
            out[i] = st[0]
            continue
        d = n - 1
        p = i * (S - 1)                                 # position i / (n - 1) of the ramp, in units of 1 / d segments
        seg = min(p // d, S - 2)
        num = p - seg * d                               # 0 <= num <= d: the fraction num / d inside the segment
        for c in range(3):
            a, b = st[seg][c], st[seg + 1][c]
            out[i, c] = (2 * (a * d + (b - a) * num) + d) // (2 * d)
    return out


HEAT = colormap([(0, 0, 0), (255, 0, 0), (255, 255, 0), (255, 255, 255)], 256)      # black -> red -> yellow -> white


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
