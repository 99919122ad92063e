"""numpy restatement of the calibration bins of mmsa.evaluate (mmsa_eval_calibration, csrc/calibrate.hip), in int64 with np.add.at, and a seeded case
generator.  The reference project has no calibration step: the definitions are this project's own (include/mmsa.h), stated here:

  takes part   iff the transformed label l (label_map / reduce_zero_label / ignore_index, as tests/eval_ref.py states them) is kept and l < C;
  correct      iff pred == l (a prediction of 255 never is);
  clamp        c = float32 confidence, NaN and negative values -> 0.0, values above 1 -> 1.0;
  bin          k = min(K - 1, trunc(float32(c) * float32(K))): ONE float32 product;
  conf_sum     q = floor(c * 2^24), exact;
  bins         int64 [3, K]: rows total, correct, conf_sum.

The checker of tests/test_calibration_gpu.py (np.array_equal on int64) and of tests/test_calibration_cpu.py, where a brute-force loop in Python
integers and fractions pins it."""
import numpy as np

from tests import eval_ref as ER

SPECIALS = np.array([np.nan, -1.0, 2.0, 0.0, 1.0, 1e-40, np.nextafter(np.float32(1), np.float32(0)), np.inf, -np.inf, -0.0], dtype=np.float32)


def clamp(conf):
    c = np.asarray(conf, dtype=np.float32)
    with np.errstate(invalid="ignore"):
        return np.where(c > 0, np.minimum(c, np.float32(1)), np.float32(0)).astype(np.float32)


def bin_index(conf, K):
    """The bin of every confidence (after the clamp): one float32 product, truncated, capped at K - 1."""
    prod = clamp(conf) * np.float32(K)
    assert prod.dtype == np.float32
    return np.minimum(K - 1, prod.astype(np.int64))


def fixed_point(conf):
    return np.floor(clamp(conf).astype(np.float64) * 2.0 ** 24).astype(np.int64)          # float32 * 2^24 is exact in float64


def participates(label, C, **kw):
    """(mask of the pixels that take part, transformed label) of a raw label map."""
    lab, keep = ER.transform_labels(label, **kw)
    return keep & (lab.astype(np.int64) < C), lab


def bins_of(pred, conf, label, C, K, **kw):
    """One image (or any array of pixels) -> int64 [3, K]."""
    part, lab = participates(label, C, **kw)
    k, q = bin_index(conf, K), fixed_point(conf)
    good = part & (pred.astype(np.int64) == lab.astype(np.int64))
    out = np.zeros((3, K), dtype=np.int64)
    np.add.at(out[0], k[part], 1)
    np.add.at(out[1], k[good], 1)
    np.add.at(out[2], k[part], q[part])
    return out


def bins_of_batch(pred, conf, label, C, K, slots=None, n_slots=None, **kw):
    B = pred.shape[0]
    slots = list(range(B)) if slots is None else slots
    out = np.zeros((max(slots) + 1 if n_slots is None else n_slots, 3, K), dtype=np.int64)
    for b in range(B):
        out[slots[b]] += bins_of(pred[b], conf[b], label[b], C, K, **kw)
    return out


def ece_float64(pred, conf, label, C, K, **kw):
    """The ECE in float64 from the UNQUANTISED (clamped) confidences: what the bins' ECE is within 2^-24 of."""
    part, lab = participates(label, C, **kw)
    k, c = bin_index(conf, K)[part], clamp(conf)[part].astype(np.float64)
    good = (pred.astype(np.int64) == lab.astype(np.int64))[part]
    n, ece = k.size, 0.0
    for j in range(K):
        sel = k == j
        if sel.any():
            ece += sel.sum() / n * abs(good[sel].mean() - c[sel].mean())
    return ece


def make_case(seed, H, W, C, K, B=1, out_of_range=None):
    """Seeded (pred uint8, conf float32, label uint8), each [B, H, W]: predictions uniform in [0, C) with 2 % at 255; labels equal to the prediction for
    about 60 % of the pixels, else another draw, 5 % ignored (255) and 3 % out of range; confidences uniform in [0, 1) with 20 % replaced by exact edges
    j / K (j = 0 .. K), 0 where the prediction is 255; the first len(SPECIALS) pixels of every image carry SPECIALS on a pixel that takes part and is
    correct under the plain LUT (needs H * W >= 10)."""
    rng = np.random.default_rng(seed)
    pred = rng.integers(0, C, size=(B, H, W)).astype(np.uint8)
    pred[rng.random((B, H, W)) < 0.02] = 255
    label = np.where(rng.random((B, H, W)) < 0.6, pred, rng.integers(0, C, size=(B, H, W))).astype(np.uint8)
    r = rng.random((B, H, W))
    label[r < 0.05] = 255
    label[(r >= 0.05) & (r < 0.08)] = min(C + 5, 254) if out_of_range is None else out_of_range
    conf = rng.random((B, H, W), dtype=np.float32)
    edges = (rng.integers(0, K + 1, size=(B, H, W)).astype(np.float64) / K).astype(np.float32)
    conf = np.where(rng.random((B, H, W)) < 0.2, edges, conf).astype(np.float32)
    conf[pred == 255] = 0
    n = len(SPECIALS)
    assert H * W >= n
    cls = (np.arange(n) % C).astype(np.uint8)
    for a, v in ((pred, cls), (label, cls), (conf, SPECIALS)):
        a.reshape(B, -1)[:, :n] = v
    return pred, conf, label
