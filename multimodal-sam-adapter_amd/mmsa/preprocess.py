"""The input side of the reference's test pipelines on device (segmentation/mmseg_custom/datasets/pipelines/transform.py):
[`Resize_multimodal` (1136-1167), opt-in] -> `Pad_multimodal` (2934-3010) -> `Normalize_multimodal` / `Normalize_multimodal_Muses` (2601-2825) -> `ImageToTensor` -> `Collectmod`,
from the frames the loaders return -- one HWC tensor [B, Hs, Ws, 3] per modality, uint8 or float32 -- to the float32 NCHW tensor the
network reads, in ONE launch (csrc/preprocess.hip): whole (`pp(rgb, aux)` -> [B, 6, H, W]) or directly as the windows of slide inference
(`pp.crops(...)` -> [n, 6, hc, wc]; the full-size normalised frame is never written).  `FrameFeeder` brings host frames to the device
through pinned staging buffers and a copy stream.

The arithmetic is the reference's float32 sequence, one rounding per step: a = x / 255 (where norm_by_max applies), (a - mean) * sinv with
sinv = float32(1 / float64(float32(std))) as mmcv.imnormalize_ computes it.  There is no CPU path."""
import ctypes

import numpy as np
import torch

from . import lib
from . import ops

VARIANTS = ("multimodal", "muses")
_DT = {torch.uint8: 0, torch.float32: 1}      # include/mmsa.h MMSA_PRE_U8 / MMSA_PRE_F32
MAX_WINDOWS = 64
_NP_DT = {np.dtype(np.uint8): torch.uint8, np.dtype(np.float32): torch.float32}

# pipeline steps from_pipeline() reads; everything else is refused by name
_LOADERS = ("LoadImageandModalities",)
_NORMALIZE = {"Normalize_multimodal": "multimodal", "Normalize_multimodal_Muses": "muses"}


def rescale_size(h, w, scale):
    """mmcv.imrescale's size for keep_ratio=True: the largest size inside `scale` (long edge, short edge), rounded half up."""
    long_e, short_e = max(scale), min(scale)
    f = min(long_e / max(h, w), short_e / min(h, w))
    return int(h * float(f) + 0.5), int(w * float(f) + 0.5)


def resize_axis_table(n_src, n_dst, fixed_point):
    """One axis of cv2.resize(INTER_LINEAR) as OpenCV's resize.cpp states it -> (first tap int32 [n_dst], coefficient pairs [n_dst, 2]).
    inv = double(n_dst) / n_src, scale = 1.0 / inv (not n_src / n_dst); f = float32((d + 0.5) * scale - 0.5), evaluated in double and rounded
    once; s = floor(f), f -= s; s < 0 -> (0, 0); s >= n_src - 1 -> (n_src - 1, 0): the second tap is then the same pixel.  Coefficients:
    int16 round-half-even of (1 - f) * 2048 and f * 2048 (the 8-bit fixed-point path), or float32 (1 - f, f)."""
    scale = 1.0 / (np.float64(n_dst) / np.float64(n_src))
    f = ((np.arange(n_dst, dtype=np.float64) + 0.5) * scale - 0.5).astype(np.float32)
    s = np.floor(f).astype(np.int32)
    f = f - s.astype(np.float32)
    low, high = s < 0, s >= n_src - 1
    s[low], f[low] = 0, 0
    s[high], f[high] = n_src - 1, 0
    pair = np.stack([np.float32(1) - f, f], 1)
    if fixed_point:
        pair = np.rint(pair * np.float32(2048)).astype(np.int16)       # cvRound: half to even; the products are exact in float32
    return s, np.ascontiguousarray(pair)


class Preprocess:
    """Normalisation (+ padding) of a bimodal frame with the keyword names of the reference's `Normalize_multimodal*` / `Pad_multimodal`.

    variant "multimodal": every modality is divided by 255 when `norm_by_max` (transform.py:2801-2804);
    variant "muses": only the modality named 'rgb' is (transform.py:2685-2694).
    `pad_size` = (H, W) of `Pad_multimodal(size=...)` applied BEFORE the normalisation (the FMB test pipelines): pixels below / right of the
    source are `pad_val`, then normalised.
    `resize` = dict(img_scale=(w, h), keep_ratio=True) of a `Resize_multimodal` step that comes FIRST (transform.py:1136-1167).  By default it is
    accepted only where it is the identity for the frames given; with `device_resize=True` the launch resizes (cv2.resize INTER_LINEAR as
    OpenCV's resize.cpp states it: 8-bit fixed point when both sources are uint8, float32 otherwise), then pads and normalises."""

    def __init__(self, mean, std, to_rgb, modalities_name, modalities_ch, norm_by_max=False, variant="multimodal", pad_size=None, pad_val=0,
                 resize=None, device_resize=False):
        if variant not in VARIANTS:
            raise ValueError(f"mmsa.Preprocess: variant '{variant}' is not one of {VARIANTS}")
        if list(modalities_ch) != [3, 3] or len(modalities_name) != 2:
            raise ValueError(f"mmsa.Preprocess: modalities_ch must be [3, 3] (two 3-channel modalities, what the TwinConvNeXt stem reads), got {list(modalities_ch)}")
        if len(mean) != 6 or len(std) != 6 or len(to_rgb) != 2:
            raise ValueError("mmsa.Preprocess: mean and std need 6 values, to_rgb one flag per modality")
        self.modalities_name, self.modalities_ch = list(modalities_name), [3, 3]
        self.norm_by_max, self.variant = bool(norm_by_max), variant
        self.mean = np.array(mean, dtype=np.float32)
        self.std = np.array(std, dtype=np.float32)
        if not np.isfinite(self.mean).all() or not np.isfinite(self.std).all() or (self.std == 0).any():
            raise ValueError(f"mmsa.Preprocess: mean / std must be finite and std free of zeros, got mean {list(mean)}, std {list(std)}")
        with np.errstate(over="ignore"):
            self.sinv = (1 / np.float64(self.std)).astype(np.float32)          # mmcv.imnormalize_: stdinv = 1 / np.float64(std), applied to float32 data
        if not np.isfinite(self.sinv).all() or (self.sinv == 0).any():
            raise ValueError(f"mmsa.Preprocess: 1 / std is not a finite, non-zero float32 for std {list(std)}")
        self.to_rgb = [bool(t) for t in to_rgb]
        if self.norm_by_max:
            self.div255 = [True, True] if variant == "multimodal" else [n == "rgb" for n in self.modalities_name]
        else:
            self.div255 = [False, False]
        self.pad_size = None if pad_size is None else (int(pad_size[0]), int(pad_size[1]))
        pv = [pad_val, pad_val] if np.isscalar(pad_val) else list(pad_val)
        if len(pv) != 2 or not np.isfinite(np.array(pv, dtype=np.float32)).all():
            raise ValueError("mmsa.Preprocess: pad_val is one finite number, or one per modality")
        self.pad_val = [float(v) for v in pv]
        if resize is not None:
            sc = resize.get("img_scale")
            if sc is None or len(sc) != 2 or isinstance(sc[0], (list, tuple)) or resize.get("ratio_range") is not None:
                raise NotImplementedError("mmsa.Preprocess: resize needs one img_scale=(w, h); a ratio range or several scales are not built")
            resize = dict(img_scale=(int(sc[0]), int(sc[1])), keep_ratio=bool(resize.get("keep_ratio", True)))
        self.resize = resize        # a Resize_multimodal step before the padding: the identity for the frames given unless device_resize
        self.device_resize = bool(device_resize)
        self._tables = {}           # (Hs, Ws, Hr, Wr, fixed_point, device) -> device tables, uploaded once
        self._c_mean = (ctypes.c_float * 6)(*self.mean.tolist())
        self._c_sinv = (ctypes.c_float * 6)(*self.sinv.tolist())
        self._c_div = (ctypes.c_int * 2)(*[int(v) for v in self.div255])
        self._c_swap = (ctypes.c_int * 2)(*[int(v) for v in self.to_rgb])
        self._c_pad = (ctypes.c_float * 2)(*self.pad_val)

    @classmethod
    def from_pipeline(cls, test_pipeline, resize=None):
        """Build from a reference config's `test_pipeline` (the list of dicts).  Recognised: the `LoadImageandModalities*` loaders (the caller's
        job: they produce what this object takes), `MultiScaleFlipAug` with one scale and flip=False, `Normalize_multimodal(_Muses)`,
        `Pad_multimodal(size=...)` before the normalisation, `ImageToTensor`, `Collectmod`, and `Resize_multimodal` as the first of them: where it
        is the identity for the frames given (checked per call against the source size), or, with resize="device", carried out by the launch.
        Any other step raises NotImplementedError naming it."""
        if resize not in (None, "device"):
            raise ValueError(f"mmsa.Preprocess.from_pipeline: resize={resize!r}; None (identity only) or 'device'")
        device_resize, resize = resize == "device", None
        norm = pad = None

        def walk(steps):
            nonlocal norm, pad, resize
            for st in steps:
                t = st.get("type")
                if isinstance(t, str) and t.startswith(_LOADERS):
                    continue
                if t == "MultiScaleFlipAug":
                    sc = st.get("img_scale")
                    if sc is not None and len(sc) and isinstance(sc[0], (list, tuple)) and len(sc) != 1:
                        raise NotImplementedError(f"MultiScaleFlipAug with {len(sc)} scales (multi-scale test-time augmentation is not built)")
                    if st.get("img_ratios") is not None:
                        raise NotImplementedError("MultiScaleFlipAug with img_ratios (multi-scale test-time augmentation is not built)")
                    if st.get("flip", False):
                        raise NotImplementedError("MultiScaleFlipAug with flip=True (flip test-time augmentation is not built)")
                    walk(st.get("transforms", []))
                elif t in _NORMALIZE:
                    if norm is not None:
                        raise NotImplementedError(f"a second {t} step")
                    norm = st
                elif t == "Pad_multimodal":
                    if norm is not None:
                        raise NotImplementedError("Pad_multimodal after the normalisation (the padding would be 0 AFTER normalising; the test pipelines pad first)")
                    if st.get("size") is None or st.get("size_divisor") is not None:
                        raise NotImplementedError("Pad_multimodal without a fixed size (size_divisor)")
                    if pad is not None:
                        raise NotImplementedError("a second Pad_multimodal step")
                    pad = st
                elif t == "Resize_multimodal":
                    if st.get("ratio_range") is not None or st.get("img_scale") is None or isinstance(st["img_scale"][0], (list, tuple)):
                        raise NotImplementedError("Resize_multimodal with a ratio range or several scales (only one fixed img_scale has a device form)")
                    if norm is not None or pad is not None or resize is not None:
                        raise NotImplementedError("Resize_multimodal after Pad_multimodal / the normalisation, or twice")
                    resize = dict(img_scale=tuple(st["img_scale"]), keep_ratio=bool(st.get("keep_ratio", True)))
                elif t in ("ImageToTensor", "Collectmod"):
                    continue
                else:
                    raise NotImplementedError(f"pipeline step '{t}' has no device form in mmsa.Preprocess")

        walk(test_pipeline)
        if norm is None:
            raise NotImplementedError("the pipeline has no Normalize_multimodal / Normalize_multimodal_Muses step")
        pp = cls(norm["mean"], norm["std"], norm["to_rgb"], norm["modalities_name"], norm["modalities_ch"], norm_by_max=norm.get("norm_by_max", False),
                 variant=_NORMALIZE[norm["type"]], pad_size=None if pad is None else pad["size"], pad_val=0 if pad is None else pad.get("pad_val", 0),
                 resize=resize, device_resize=device_resize)
        return pp

    # ---- geometry / checks ----
    def resized(self, Hs, Ws):
        """(Hr, Wr) of an Hs x Ws source after the Resize_multimodal step (the source size without one)."""
        if self.resize is None:
            return Hs, Ws
        sc = self.resize["img_scale"]
        new = rescale_size(Hs, Ws, sc) if self.resize["keep_ratio"] else (sc[1], sc[0])       # img_scale is (w, h)
        if new != (Hs, Ws):
            if not self.device_resize:
                raise NotImplementedError(f"Resize_multimodal(img_scale={sc}, keep_ratio={self.resize['keep_ratio']}) turns a {Hs} x {Ws} frame into {new[0]} x {new[1]}: "
                                          "only the identity is supported (the OpenCV bilinear resize is not built) unless the object is made with "
                                          "from_pipeline(..., resize='device') / device_resize=True")
            if Hs == 2 * new[0] and Ws == 2 * new[1]:
                raise NotImplementedError(f"Resize_multimodal from {Hs} x {Ws} to {new[0]} x {new[1]}: with both scale factors exactly 2, cv2.resize replaces "
                                          "INTER_LINEAR by its 2 x 2 area average (INTER_AREA), which is not built")
        return new

    def canvas(self, Hs, Ws):
        """(H, W) of the normalised frame for an Hs x Ws source: the pad size, or the (resized) source size."""
        Hr, Wr = self.resized(Hs, Ws)
        if self.pad_size is None:
            return Hr, Wr
        H, W = self.pad_size
        if H < Hr or W < Wr:
            raise RuntimeError(f"mmsa.Preprocess: pad size {H} x {W} is smaller than the {Hr} x {Wr} {'source' if (Hr, Wr) == (Hs, Ws) else 'resized frame'} "
                               "(padding only grows a frame)")
        return H, W

    def resize_tables(self, Hs, Ws, Hr, Wr, fixed_point, device):
        """The four device tables of the resizing launch (x taps, x coefficients, y taps, y coefficients), built in numpy, uploaded once per
        geometry and kept: a later call with the same geometry launches without any copy or allocation (and can be captured in a HIP graph)."""
        key = (Hs, Ws, Hr, Wr, bool(fixed_point), torch.device(device))
        tabs = self._tables.get(key)
        if tabs is None:
            if _capturing(key[-1]):
                raise RuntimeError(f"mmsa.Preprocess: the resize tables for {Hs} x {Ws} -> {Hr} x {Wr} are not on the device yet and cannot be uploaded "
                                   "during a graph capture: run one call with this geometry before capturing")
            xs, xc = resize_axis_table(Ws, Wr, fixed_point)
            ys, yc = resize_axis_table(Hs, Hr, fixed_point)
            tabs = tuple(torch.from_numpy(t).to(key[-1]) for t in (xs, xc, ys, yc))
            self._tables[key] = tabs
        return tabs

    def _resize_args(self, rgb, aux, Hr, Wr):
        fixed = rgb.dtype == torch.uint8 and aux.dtype == torch.uint8     # a pair with a float32 modality is float32 as a whole (loading.py:225)
        xs, xc, ys, yc = self.resize_tables(rgb.shape[1], rgb.shape[2], Hr, Wr, fixed, rgb.device)
        return (Hr, Wr, xs.data_ptr(), xc.data_ptr(), ys.data_ptr(), yc.data_ptr(), int(fixed))

    def check(self, rgb, aux):
        """The two sources as the kernels need them, or a RuntimeError: [B, Hs, Ws, 3], HWC contiguous, uint8 or float32, on one GPU."""
        for name, t in ((self.modalities_name[0], rgb), (self.modalities_name[1], aux)):
            if not isinstance(t, torch.Tensor) or not t.is_cuda:
                raise RuntimeError(f"mmsa.Preprocess: '{name}' must be a GPU tensor (there is no CPU path; FrameFeeder uploads host frames)")
            if t.dtype not in _DT:
                raise RuntimeError(f"mmsa.Preprocess: '{name}' is {t.dtype}; the loaders' uint8 or float32 is expected")
            if t.dim() != 4 or t.shape[3] != 3:
                raise RuntimeError(f"mmsa.Preprocess: '{name}' must be [B, H, W, 3] (HWC, 3 channels), got {tuple(t.shape)}")
            if not t.is_contiguous():
                raise RuntimeError(f"mmsa.Preprocess: '{name}' must be contiguous")
        if rgb.shape != aux.shape or rgb.device != aux.device:
            raise RuntimeError(f"mmsa.Preprocess: the two modalities differ in shape or device: {tuple(rgb.shape)} on {rgb.device}, {tuple(aux.shape)} on {aux.device}")
        return rgb, aux

    def _args(self, rgb, aux):
        B, Hs, Ws, _ = rgb.shape
        return (rgb.data_ptr(), _DT[rgb.dtype], aux.data_ptr(), _DT[aux.dtype], B, Hs, Ws, self._c_mean, self._c_sinv, self._c_div, self._c_swap, self._c_pad)

    # ---- the two launches ----
    @torch.no_grad()
    def __call__(self, rgb, aux, out=None):
        """[B, 6, H, W] float32: the tensor `Collectmod` hands to the model."""
        rgb, aux = self.check(rgb, aux)
        B, Hs, Ws, _ = rgb.shape
        H, W = self.canvas(Hs, Ws)
        with torch.cuda.device(rgb.device):
            if out is None:
                out = torch.empty(B, 6, H, W, device=rgb.device)
            _check_out(out, (B, 6, H, W), rgb.device)
            Hr, Wr = self.resized(Hs, Ws)
            if (Hr, Wr) == (Hs, Ws):
                lib.call("mmsa_preprocess_nhwc", *self._args(rgb, aux), out.data_ptr(), H, W, ops._stream())
            else:
                lib.call("mmsa_preprocess_resize_nhwc", *self._args(rgb, aux), out.data_ptr(), H, W, *self._resize_args(rgb, aux, Hr, Wr), ops._stream())
        return out

    @torch.no_grad()
    def crops(self, rgb, aux, jobs, crop_size, out=None):
        """[n, 6, hc, wc] float32: window k = `jobs[k]` = (image, (y1, x1, y2, x2)) of the padded, normalised frame (the job list of
        mmsa.inference: ED:205-212), at most 64 windows per call."""
        rgb, aux = self.check(rgb, aux)
        B, Hs, Ws, _ = rgb.shape
        H, W = self.canvas(Hs, Ws)
        n = len(jobs)
        if n > MAX_WINDOWS:
            raise RuntimeError(f"mmsa.Preprocess.crops: at most {MAX_WINDOWS} windows per call, got {n}")
        hc, wc = int(crop_size[0]), int(crop_size[1])
        tab = (ctypes.c_int * (3 * max(n, 1)))(*[int(v) for b, (y1, x1, _, _) in jobs for v in (b, y1, x1)])
        with torch.cuda.device(rgb.device):
            if out is None:
                out = torch.empty(n, 6, hc, wc, device=rgb.device)
            _check_out(out, (n, 6, hc, wc), rgb.device)
            Hr, Wr = self.resized(Hs, Ws)
            if (Hr, Wr) == (Hs, Ws):
                lib.call("mmsa_preprocess_crops", *self._args(rgb, aux), H, W, tab, n, out.data_ptr(), hc, wc, ops._stream())
            else:
                lib.call("mmsa_preprocess_resize_crops", *self._args(rgb, aux), H, W, tab, n, out.data_ptr(), hc, wc, *self._resize_args(rgb, aux, Hr, Wr),
                         ops._stream())
        return out


def _capturing(device):
    return device.type == "cuda" and torch.cuda.is_current_stream_capturing()


def _check_out(out, shape, device):
    if tuple(out.shape) != tuple(shape) or out.dtype != torch.float32 or out.device != device or not out.is_contiguous():
        raise RuntimeError(f"mmsa.Preprocess: `out` must be a contiguous float32 {tuple(shape)} tensor on {device}")


class FrameFeeder:
    """Host frames -> device pairs for `preprocess=`: `slots` pinned host staging buffers and device buffers per modality, one copy stream
    (modelled on mmsa.dist.LogitsGather).

    feed(rgb_np, aux_np): copies the arrays into the next slot's pinned buffers (the caller may reuse its arrays at once), enqueues the
    host-to-device copies on the copy stream, makes the CURRENT stream wait for that copy only, and returns the slot's device pair.  The
    consumers of a pair are whatever the caller enqueues on the current stream until the next feed(): feed() records an event behind them,
    and a slot's buffers are overwritten only after that event (the copy stream waits for it) and after the slot's previous upload has left
    the pinned buffer (the host waits for THAT copy's event).  No device-wide synchronisation anywhere.

    `shape` = (B, Hs, Ws) of the source frames; `dtypes` = torch dtypes of the two modalities (uint8 or float32)."""

    def __init__(self, pp, shape, slots=2, dtypes=(torch.uint8, torch.uint8), device=None):
        if slots < 1:
            raise ValueError("mmsa.FrameFeeder: at least one slot")
        if not torch.cuda.is_available():
            raise RuntimeError("mmsa.FrameFeeder: no GPU (there is no CPU path)")
        B, Hs, Ws = (int(v) for v in shape)
        pp.canvas(Hs, Ws)                                   # refuses a geometry the preprocess object cannot take
        for dt in dtypes:
            if dt not in _DT:
                raise RuntimeError(f"mmsa.FrameFeeder: dtype {dt}; uint8 or float32 is expected")
        self.pp, self.shape, self.slots = pp, (B, Hs, Ws, 3), slots
        self.device = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        self.host = [tuple(torch.empty(self.shape, dtype=dt).pin_memory() for dt in dtypes) for _ in range(slots)]
        self.dev = [tuple(torch.empty(self.shape, dtype=dt, device=self.device) for dt in dtypes) for _ in range(slots)]
        self.stream = torch.cuda.Stream(device=self.device)
        self.copied = [None] * slots          # event behind the slot's last upload (copy stream)
        self.consumed = [None] * slots        # event behind the slot's last consumers (the caller's stream)
        self.k = 0

    def feed(self, rgb_np, aux_np):
        main = torch.cuda.current_stream(self.device)
        if self.k > 0:                                      # everything enqueued since the previous feed() read the previous slot
            prev = (self.k - 1) % self.slots
            ev = torch.cuda.Event()
            ev.record(main)
            self.consumed[prev] = ev
        slot = self.k % self.slots
        if self.copied[slot] is not None:
            self.copied[slot].synchronize()                 # host: the pinned buffer's previous contents have left (an event, not the device)
        for h, a in zip(self.host[slot], (rgb_np, aux_np)):
            a = np.asarray(a)
            if a.ndim == 3:
                a = a[None]
            if tuple(a.shape) != self.shape or _NP_DT.get(a.dtype) != h.dtype:
                raise RuntimeError(f"mmsa.FrameFeeder: expected {self.shape} {h.dtype} frames, got {tuple(a.shape)} {a.dtype}")
            np.copyto(h.numpy(), a)
        if self.consumed[slot] is not None:
            self.stream.wait_event(self.consumed[slot])     # device: the slot's last consumers are done with its device buffers
        with torch.cuda.stream(self.stream):
            for h, d in zip(self.host[slot], self.dev[slot]):
                d.copy_(h, non_blocking=True)
            ev = torch.cuda.Event()
            ev.record(self.stream)
        self.copied[slot] = ev
        main.wait_event(ev)                                 # the current stream waits for THIS copy only
        self.k += 1
        return self.dev[slot]
