"""Torch / numpy restatement of what `rescale=True` adds to the reference's slide and whole inference (segmentors/encoder_decoder.py:227-233,
314-325: one more bilinear resize, align_corners=False, of the averaged logits to `ori_shape`) -- TEST INFRASTRUCTURE ONLY.  Pinned by
tests/golden/rescale.npz, which tools/oracle/make_golden.py::gen_rescale produces by calling the reference's own, unmodified methods."""
import numpy as np
import torch
import torch.nn.functional as F

from oracle import ref_segmentor as RS

NUM_CLASSES, TOY_SEED = 5, 79      # toy_encode_decode(NUM_CLASSES, seed=TOY_SEED) of gen_rescale


def frame(hw, seed=35):
    """The seeded frame of gen_rescale: white noise plus one offset per channel."""
    g = torch.Generator().manual_seed(seed)
    return torch.randn(1, 6, hw[0], hw[1], generator=g) + torch.randn(1, 6, 1, 1, generator=g)


def case_of(cfg):
    """A fixture's `<tag>_cfg` row -> (frame (h, w), crop or None, stride or None, ori_shape)."""
    c = [int(v) for v in cfg]
    return (c[0], c[1]), ((c[2], c[3]) if c[2] else None), ((c[4], c[5]) if c[2] else None), (c[6], c[7])


def rescaled_logits(encode_decode_fn, img, ori_shape, crop_size=None, stride=None, num_classes=NUM_CLASSES):
    y = encode_decode_fn(img) if crop_size is None else RS.slide_inference(encode_decode_fn, img, crop_size, stride, num_classes)
    return F.interpolate(y, size=tuple(ori_shape), mode="bilinear", align_corners=False)


def near_ties(y, tol):
    """Pixels whose top-two margin is within 2 * tol * max|y|: the ones a class map within `tol` of y may decide differently -> bool [B, h, w]."""
    top = y.topk(2, dim=1).values
    return (top[:, 0] - top[:, 1]) <= 2 * tol * y.abs().max()


def taps(n_src, n_dst):
    """One axis of the second resize as the kernels compute it in float32: src = (dst + 0.5) * (float(n_src) / float(n_dst)) - 0.5 clamped at 0 ->
    (first tap, second tap) int arrays [n_dst]."""
    r = np.float32(n_src) / np.float32(n_dst)
    s = (np.arange(n_dst, dtype=np.float32) + np.float32(0.5)) * r - np.float32(0.5)
    s = np.maximum(s, np.float32(0))
    t0 = np.minimum(s.astype(np.int64), n_src - 1)
    return t0, np.minimum(t0 + 1, n_src - 1)


def touches_uncovered(count, Hd, Wd):
    """count [B, H, W] (windows per canvas pixel) -> bool [B, Hd, Wd]: output pixels one of whose four canvas taps no window covers."""
    y0, y1 = taps(count.shape[1], Hd)
    x0, x1 = taps(count.shape[2], Wd)
    z = count == 0
    return z[:, y0][:, :, x0] | z[:, y0][:, :, x1] | z[:, y1][:, :, x0] | z[:, y1][:, :, x1]
