"""numpy restatement of the per-bin confusion counts of mmsa.evaluate (mmsa_eval_selective, csrc/selective.hip) and of the thresholded map
(mmsa_abstain_u8), in int64 with np.add.at, and a seeded generator of patchy cases.  The reference project has no such step: the definitions are this
project's own (include/mmsa.h), and both halves are the existing restatements, imported:

  label side        tests/eval_ref.py `transform_labels`: l = transformed label; ignored pixels are counted nowhere; row = min(l, C), col = min(pred, C);
  confidence side   tests/calibration_ref.py `bin_index`: clamp, ONE float32 product, truncated, capped at K - 1;
  counts            int64 [K, C + 1, C + 1], counts[k, row, col] += 1 for every pixel that is not ignored (row C included);
  abstain           pred where bin >= min_bin, 255 elsewhere.

The checker of tests/test_selective_gpu.py (np.array_equal on int64 / uint8) and of tests/test_selective_cpu.py, where a brute-force loop pins it."""
import numpy as np

from tests import calibration_ref as CR
from tests import eval_ref as ER


def counts_of(pred, conf, label, C, K, **kw):
    """One image (or any array of pixels) -> int64 [K, C + 1, C + 1]."""
    lab, keep = ER.transform_labels(label, **kw)
    k = CR.bin_index(conf, K)
    row, col = np.minimum(lab.astype(np.int64), C), np.minimum(pred.astype(np.int64), C)
    out = np.zeros((K, C + 1, C + 1), dtype=np.int64)
    np.add.at(out, (k[keep], row[keep], col[keep]), 1)
    return out


def counts_of_batch(pred, conf, label, C, K, slots=None, n_slots=None, **kw):
    B = pred.shape[0]
    slots = list(range(B)) if slots is None else slots
    out = np.zeros((max(slots) + 1 if n_slots is None else n_slots, K, C + 1, C + 1), dtype=np.int64)
    for b in range(B):
        out[slots[b]] += counts_of(pred[b], conf[b], label[b], C, K, **kw)
    return out


def abstain_of(pred, conf, K, min_bin):
    return np.where(CR.bin_index(conf, K) >= min_bin, pred, np.uint8(255)).astype(np.uint8)


def abstained_counts(counts, k0):
    """Identity 3: the plain confusion counts of abstain_of(pred, conf, K, k0), from the per-bin counts [K, C + 1, C + 1]."""
    out = counts[k0:].sum(0)
    out[:, -1] += counts[:k0].sum((0, 2))
    return out


GPU_PAIRS = ((2, 1), (2, 64), (25, 15), (25, 64), (63, 15), (63, 16), (126, 2), (126, 64))     # (C, K): see tests/test_selective_gpu.py for the bin groups
GPU_WIDTHS = (1, 255, 257, 1021)
VARIANTS = (dict(), dict(reduce_zero_label=True), dict(label_map={2: 1, 1: 0}), dict(ignore_index=0))
OFFSETS = ((0, 0), (1, 1), (3, 2), (2, 0), (0, 3), (2, 2), (3, 3))       # base pointers of pred and label: aligned, equally and differently misaligned


def gpu_cases(C, K):
    """The cases of tests/test_selective_gpu.py::test_counts_equal_the_restatement for one (C, K), shared with tests/test_selective_cpu.py, which checks
    on the host what the GPU test asserts of their data: (B, H, W, kw, po, lo, co, seed).  B in 1..3 and every width; the label variants, the pred /
    label base-pointer offsets and the float4 phase of the confidence pointer cycle.  The plain LUT goes with W = 1 and W = 1021: at 64 bins a 37 x 255
    image has 4 to 5 out-of-range labels per bin on average and some bin would have none, at 37 x 1021 it has 17 to 18."""
    k = 7 * GPU_PAIRS.index((C, K))
    for B in (1, 2, 3):
        for wi, W in enumerate(GPU_WIDTHS):
            kw = VARIANTS[0] if wi in (0, 3) else VARIANTS[1 + k % 3]
            yield B, (37 if W > 1 else 300), W, kw, OFFSETS[k % 7][0], OFFSETS[k % 7][1], 4 * ((k + k // 4) % 4), 7000 + 131 * C + K + k
            k += 1


def make_patchy_case(seed, H, W, C, K, B=1, top=0.9):
    """Seeded (pred uint8, conf float32, label uint8), each [B, H, W], shaped like a trained model's output: tests/eval_ref.py's patches of classes for pred
    and label (with its ignored, out-of-range and uncovered pixels), ONE confidence per 16 x 16 block, `top` of the blocks inside the top bin and the rest
    uniform in [0, 1)."""
    pred, label = ER.make_case(seed, H, W, C, B=B)
    rng = np.random.default_rng(seed + 1)
    hb, wb = (H + 15) // 16, (W + 15) // 16
    lo = np.float32((K - 1) / K) + np.float32(0.25 / K)                         # well inside the top bin
    block = np.where(rng.random((B, hb, wb)) < top, lo + rng.random((B, hb, wb), dtype=np.float32) * np.float32(0.5 / K),
                     rng.random((B, hb, wb), dtype=np.float32)).astype(np.float32)
    conf = np.repeat(np.repeat(block, 16, 1), 16, 2)[:, :H, :W].copy()
    return pred, conf, label
