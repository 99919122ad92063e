"""The output side of the reference's `tools/test.py` loop on device: what `dataset.pre_eval` -> `intersect_and_union` -> `pre_eval_to_metrics` /
`total_area_to_metrics` do with a class map (segmentation/mmseg_custom/datasets/DELIVER.py:194-259, apis/evaluation/metrics_micro.py:26-86, 451-526).

The device keeps ONE integer matrix per count slot, int64 [C + 1, C + 1], counts[label class, predicted class]; index C = "a value outside [0, C) that is
not ignored" (what torch.histc(min=0, max=C-1) drops from one of its histograms only), ignored pixels are counted nowhere.  The reference's four
histograms follow from it (`areas_of`).  `label_map`, `reduce_zero_label` and `ignore_index` are one 256-byte LUT applied to the raw label byte; the
nearest-neighbour label resize of `Resize_multimodal._resize_seg` (datasets/pipelines/transform.py:1169-1188) is a pair of per-axis index tables.
Counting is either a pass of its own over a stored map (`confusion`, mmsa_eval_confusion_u8) or part of the class-map kernel (`labels=` / `evaluator=`
of mmsa.inference's class-map calls, mmsa_slide_argmax_eval).  Only `Evaluator.areas()` copies anything to the host: (C + 1)^2 integers per slot.

Deviation from the reference, on purpose: it sums per-image float32 histograms in float32 (metrics_micro.py:416-419), exact only below 2^24 pixels per
class and case; the int64 counts here are exact at any size, and the metrics are formed in float64.  There is no CPU path for the counting.

Calibration of the confidence map (the probability of the predicted class, `confidence=` of the class-map calls) is the second half: `calibration` /
`Calibration` reduce (class map, confidence map, label map) to int64 [3, K] reliability bins per slot -- total, correct, and the confidence sum in 24-bit
fixed point (mmsa_eval_calibration, csrc/calibrate.hip) -- from which `reliability_of`, `ece_of`, `mce_of` and `risk_coverage_of` form the reliability
diagram, the expected / maximum calibration error and accuracy against coverage in float64 on the host.  The reference has no such step.

Selective evaluation joins the two: `selective` / `SelectiveEvaluator` keep ONE confusion matrix PER CONFIDENCE BIN, int64 [K, C + 1, C + 1] per slot
(mmsa_eval_selective, csrc/selective.hip), with the label side of the confusion counts and the confidence side of the reliability bins, both verbatim:
their sum over the bins is the Evaluator's matrix, the rows < C of bin k give Calibration's total[k] / correct[k], and the suffix sums over the bins are
the confusion counts of the map with the pixels below a confidence threshold taken out.  `selective_metrics_of` forms the reference's metrics at every
such threshold in float64 -- mIoU against coverage -- and `abstain` (mmsa_abstain_u8) writes the thresholded map (255 where the bin is below) that
those counts describe, from the same clamp and bin.  The reference has no such step either.

Temperature scaling closes the loop from a poor ECE to a better confidence: `temperature_sweep` / `TemperatureSweep` reduce a LOGITS canvas (what
`mmsa.inference.inference` returns) against the labels, for a whole grid of temperatures in one launch (mmsa_temperature_sweep_nchw, csrc/temperature.hip),
to int64 [J, 4, K] per slot -- per temperature, Calibration's three rows of the confidence max_c softmax(x / T)_c, and the NLL of the label's class in 20-bit
fixed point.  `best()` names the grid's minimum of the NLL or of the ECE; a second, narrower `geometric_grid` around it refines; there is no iterative
optimiser.  The fitted T then goes to `temperature=` of the class-map entries of mmsa.inference, whose confidence maps everything above reads unchanged.

Top-k evaluation asks at which rank of a top-k map (`topk=` of the class-map entries: uint8 class planes [K, B, H, W]) the label's class stands: `topk_counts` /
`TopKEvaluator` reduce (class planes, label map) to int64 [C, K + 1] per slot (mmsa_eval_topk_u8, csrc/topk_eval.hip), with the label side of the confusion
counts verbatim -- column r is the diagonal of the confusion matrix of plane r, column K "not among the K" -- from which `topk_accuracy_of` and
`topk_recall_of` form the top-1 .. top-K pixel accuracy (the first is the Evaluator's aAcc) and the per-class recall@j in float64 on the host.

Boundary evaluation asks how good the contours are: `boundary_counts` / `BoundaryEvaluator` reduce (class map, label map) to int64 [4, C + 1, C + 1] per slot
(mmsa_eval_boundary_u8, csrc/boundary.hip) -- the confusion matrix split into the zones 2 * near_label + near_pred, "near" = within a Chebyshev radius of a pixel
with another code -- whose zone sum is the Evaluator's matrix; `trimap_counts_of` (zones 2 + 3: the band around the label boundaries, fed to `areas_of` /
`area_metrics`) and `boundary_iou_of` (Cheng et al., CVPR 2021) form the trimap metrics and the Boundary IoU in float64 on the host.

Euclidean boundary evaluation rests on one more primitive, the exact distance map of a code map: `boundary_distance` writes, per pixel, the squared Euclidean
distance to the nearest pixel of the image with another code as uint16, up to a cap of 255 pixels (mmsa_boundary_distance_u8, csrc/distance.hip).  A band at any
radius is a threshold on two such maps (`boundary_counts_d2`, mmsa_eval_boundary_d2: the four zones above, so every `_of` function above reads them), several radii
are several pointwise launches over one pair of maps, and `boundary_displacement` (mmsa_eval_boundary_displacement) bins every contour pixel of one map by its
distance to the other map's contour, int64 [2, C + 1, cap + 2] per slot -- from which `boundary_f_of` / `boundary_f_curve_of` form the boundary F-score at a
tolerance (Csurka et al.; the DAVIS F measure) and `boundary_distance_percentile_of` the Hausdorff percentile HD95 in float64 on the host.
`EuclideanBoundaryEvaluator` is a BoundaryEvaluator that owns both buffers.

Segment-level evaluation asks what no pixel-weighted number answers: how many of the objects were found at all, by size, and how many of the painted blobs
are real.  Its unit is the segment, a connected component of one code: `components` writes, per pixel, the smallest linear index of its component as int32
(mmsa_components_u8, csrc/components.hip), read from a code map exactly as `boundary_distance` reads one.  `component_areas` and `suppress_small` (the class map
without its blobs below an area) are pointwise passes on top, and `segment_counts` / `SegmentEvaluator` reduce (class map, label map, the two root maps) to int64
[2, C, 24, bins + 1] per slot (mmsa_eval_segments): the label segments (side 0) and the prediction segments (side 1) by class, power-of-two size bucket and the
share of the segment that is covered by a correct pixel -- from which `segment_rate_of` forms the segment recall and precision at a coverage threshold and
`segment_f_of` their harmonic mean in float64 on the host.

Panoptic quality asks which prediction segment IS which label segment: `segment_pairs` fills a hash table on the device with the intersection of every (label
segment, prediction segment) pair that shares a correct pixel (mmsa_segment_pairs, csrc/pairs.hip; `PairTable`, the compact pair list), `panoptic_counts` /
`PanopticEvaluator` match the pairs by IoU > 1/2 -- unique, tested in integers -- and reduce them to int64 [C, 24, 4] per slot (mmsa_eval_panoptic): TP, FP, FN
and the fixed-point IoU sum by class and size bucket, from which `panoptic_quality_of` forms PQ = SQ * RQ per class and `panoptic_summary_of` their means in
float64 on the host.

`suppress_small`, `select_segments` and `abstain` paint what they remove with one byte.  `fill_nearest` hands such a map back full: every hole takes the value
of the nearest kept pixel of its image within a cap of up to 255 pixels, ties to the topmost and then the leftmost (mmsa_fill_nearest_u8, csrc/fill.hip: the
two launches of `boundary_distance` with a value carried along); `suppress_small(…, nearest=cap)` and `select_segments(…, nearest=cap)` end with it.

`majority_filter` is the mode filter of a class map: every target pixel takes the most frequent voter value of its (2 r + 1)^2 window, r <= 32, a tie kept by
the own value or else resolved to the smallest (mmsa_majority_filter_u8, csrc/majority.hip: one launch, per value present in a tile the rows as ballot masks,
popcounts and a sliding column sum).  It removes salt-and-pepper pixels, straightens contours and, with `where="holes"`, fills holes by vote.

`vote_filter` is the same filter with weighted votes, r <= 16: a voter's vote falls with the L1 difference of its pixel of a guide frame (raw uint8, 1 or 3
channels) from the centre's, through a range table (`vote_range_table`, or one of the caller's), and rises with its quantised confidence; the largest integer
sum wins (mmsa_vote_filter_u8, csrc/vote.hip: one launch, a per-lane column of sums in LDS over dense value slots).  Contours snap to the guide's edges.

`SegmentTracker` follows the segments of a `SegmentTable` along a stream: `track_pairs` fills the pair table with the intersection of every (current segment,
previous segment) pair (mmsa_track_pairs, csrc/track.hip), and `update()` matches them by IoU > 1/2 and hands every segment a persistent track id, its age
and its predecessor (mmsa_track_update): int32 [B, capacity, 4] per frame, new ids in raster order of the first pixel, no host sync."""
import ctypes
import math
import warnings
from collections import OrderedDict
from fractions import Fraction

import numpy as np
import torch

from . import lib
from . import ops
from .preprocess import _capturing, rescale_size

IGNORE = 255            # LUT code of an ignored label byte (csrc/eval_hist.h MMSA_EVAL_IGNORE)
MAX_IMAGES = 64         # images per launch (the slot table travels in the launch arguments)
FUSED_DEFAULT = False   # measured (profiles/evaluate.txt): the class map followed by the standalone pass is 4-9 us faster than the fused launch, beyond
                        # the yardstick's spread: two launches by default; the fused entry is reached with fused=True / return_map=False

_METRICS = ("mIoU", "mDice", "mFscore", "microIoU")

MAX_BINS = 64           # confidence bins per launch (csrc/calibrate.hip CAL_MAX_BINS)
DEFAULT_BINS = 15       # the usual reliability diagram
CONF_ONE = 1 << 24      # the fixed-point unit of a bin's confidence sum: conf_sum = sum of floor(conf * 2^24)
BIN_CAPACITY = 1 << 39  # participating pixels per bin and slot before the int64 confidence sum can overflow (2^39 * 2^24 = 2^63)

MAX_TEMPERATURES = 16   # temperatures per sweep launch (csrc/temperature.hip SWEEP_MAX_TEMPS: their sums of exponentials live in registers)
NLL_ONE = 1 << 20       # the fixed-point unit of a sweep's NLL sum: nll_sum = sum of floor(min(max(nll, 0), NLL_CAP) * 2^20)
NLL_CAP = 1024          # a pixel's NLL is capped here (NaN counts as the cap)

MAX_SELECTIVE_CLASSES = 126        # csrc/eval_hist.h MMSA_EVAL_MAX_CLASSES: one bin's (C + 1)^2 uint32 cells must fit a workgroup's 64 KiB of LDS
MAX_SELECTIVE_BYTES = 1 << 30      # the largest count buffer a SelectiveEvaluator allocates (64 slots x 64 bins x 127^2 cells x 8 bytes is 528 MB)


# ---- host-side restatements (numpy) ----
def label_bytes(ignore_index=255, label_map=None, reduce_zero_label=False):
    """What the reference's sequence (metrics_micro.py:66-74) makes of each of the 256 label byte values -> (transformed uint8 [256], kept bool [256]):
    the `label_map` entries one after the other in dict order (a later entry sees what an earlier one wrote), then `reduce_zero_label` in uint8
    arithmetic (0 -> 255, minus 1 with wrap-around, 254 -> 255), then the compare with `ignore_index`."""
    t = np.arange(256, dtype=np.uint8)
    for old, new in (label_map or {}).items():
        if not 0 <= int(new) <= 255:
            raise ValueError(f"mmsa.evaluate: label_map maps {old} to {new}, which a uint8 label cannot hold")
        t[t == old] = new
    if reduce_zero_label:
        t[t == 0] = 255
        t = t - np.uint8(1)
        t[t == 254] = 255
    return t, t != ignore_index


def label_lut(num_classes, ignore_index=255, label_map=None, reduce_zero_label=False):
    """The device LUT uint8 [256]: class 0 .. C - 1, C = kept but outside [0, C), IGNORE = dropped by the ignore mask."""
    C = int(num_classes)
    if not 2 <= C <= 254:
        raise ValueError(f"mmsa.evaluate: num_classes {num_classes}; a uint8 class map has 2..254 classes")
    t, keep = label_bytes(ignore_index, label_map, reduce_zero_label)
    return np.where(keep, np.minimum(t, C), IGNORE).astype(np.uint8)


def nearest_axis_table(n_src, n_dst):
    """One axis of cv2.resize(INTER_NEAREST) as OpenCV's resize.cpp states it: src = min(floor(d * (1.0 / (double(n_dst) / n_src))), n_src - 1), int32 [n_dst]."""
    ifx = 1.0 / (np.float64(n_dst) / np.float64(n_src))
    return np.minimum(np.floor(np.arange(n_dst, dtype=np.float64) * ifx).astype(np.int64), n_src - 1).astype(np.int32)


def areas_of(counts):
    """int64 [..., C + 1, C + 1] counts -> (area_intersect, area_union, area_pred_label, area_label), each int64 [..., C] (metrics_micro.py:78-86)."""
    counts = np.asarray(counts, dtype=np.int64)
    C = counts.shape[-1] - 1
    inter = np.diagonal(counts, axis1=-2, axis2=-1)[..., :C].copy()
    pred = counts.sum(-2)[..., :C]
    label = counts.sum(-1)[..., :C]
    return inter, pred + label - inter, pred, label


def area_metrics(area_intersect, area_union, area_pred_label, area_label, metric=("mIoU",), nan_to_num=None, beta=1):
    """`total_area_to_metrics` (metrics_micro.py:451-526) in float64 on integer areas [C]: 'aAcc' and, per metric, 'IoU' / 'Acc', 'Dice' / 'Acc',
    'Fscore' / 'Precision' / 'Recall' per class.  0 / 0 is NaN as in the reference; `nan_to_num` replaces it afterwards (np.nan_to_num)."""
    metric = [metric] if isinstance(metric, str) else list(metric)
    if not set(metric).issubset(_METRICS):
        raise KeyError(f"metrics {metric} is not supported")
    i, u, p, l = (np.asarray(a, dtype=np.float64) for a in (area_intersect, area_union, area_pred_label, area_label))
    with np.errstate(divide="ignore", invalid="ignore"):
        out = OrderedDict(aAcc=np.float64(i.sum()) / np.float64(l.sum()))
        for m in metric:
            if m in ("mIoU", "microIoU"):
                out["IoU"], out["Acc"] = i / u, i / l
            elif m == "mDice":
                out["Dice"], out["Acc"] = 2 * i / (p + l), i / l
            elif m == "mFscore":
                prec, rec = i / p, i / l
                out["Fscore"] = (1 + beta ** 2) * (prec * rec) / ((beta ** 2 * prec) + rec)
                out["Precision"], out["Recall"] = prec, rec
    if nan_to_num is not None:
        out = OrderedDict((k, np.nan_to_num(v, nan=nan_to_num)) for k, v in out.items())
    return out


def _is_int(x, lo, hi):
    """`x` is an int (numpy's too; no bool) in lo .. hi."""
    return not (isinstance(x, bool) or not isinstance(x, (int, np.integer)) or not lo <= int(x) <= hi)


def _round_percent(v):
    """v x 100 rounded to two places, / 100: how every summary rounds."""
    return np.round(v * 100, 2) / 100.0


def summary_of(metrics):
    """The summary `evaluate` forms from such a dict (DELIVER.py:327-367): nanmean per entry, x 100 rounded to two places, / 100; every key but
    'aAcc' gets the 'm' prefix."""
    return OrderedDict((k if k == "aAcc" else "m" + k, _round_percent(np.nanmean(v))) for k, v in metrics.items())


# ---- calibration metrics from the integer bins (numpy, float64) ----
def _bins3(bins):
    """int64 [3, K] (rows total, correct, conf_sum) of one slot, checked; OverflowError where a bin has reached the capacity of its confidence sum."""
    b = np.asarray(bins)
    if b.ndim != 2 or b.shape[0] != 3 or b.shape[1] < 1 or b.dtype.kind not in "iu":
        raise ValueError(f"mmsa.evaluate: calibration bins are an integer [3, K] array (total, correct, conf_sum), got {b.dtype} {b.shape}")
    b = b.astype(np.int64, copy=False)
    if (b[0] >= BIN_CAPACITY).any():
        raise OverflowError(f"mmsa.evaluate: a calibration bin holds {int(b[0].max())} pixels; from 2^39 on its int64 confidence sum may have wrapped "
                            "(read and reset() the Calibration more often, or split the run over slots)")
    return b


def reliability_of(bins):
    """The reliability diagram of int64 [3, K] bins -> OrderedDict(edges float64 [K + 1] = k / K, count int64 [K], accuracy = correct / total and
    confidence = conf_sum / (2^24 total), float64 [K], NaN in an empty bin).  The per-bin confidence lies below the float64 mean of the same
    confidences by less than 2^-24 (every term is truncated to 24 fractional bits)."""
    b = _bins3(bins)
    K = b.shape[1]
    t = b[0].astype(np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        return OrderedDict(edges=np.arange(K + 1, dtype=np.float64) / K, count=b[0].copy(), accuracy=b[1].astype(np.float64) / t,
                           confidence=b[2].astype(np.float64) / (np.float64(CONF_ONE) * t))


def _gaps(bins):
    """(weights total_k / N, |accuracy_k - confidence_k|) over the NON-EMPTY bins; two empty arrays when N == 0."""
    r = reliability_of(bins)
    full = r["count"] > 0
    n = np.float64(max(int(r["count"].sum()), 1))
    return r["count"][full].astype(np.float64) / n, np.abs(r["accuracy"][full] - r["confidence"][full])


def ece_of(bins):
    """Expected calibration error: sum over the non-empty bins of (total_k / N) |accuracy_k - confidence_k|, float64; NaN when N == 0.  Within 2^-24 of
    the ECE formed in float64 from the unquantised confidences (the weights sum to 1, each gap moves by less than 2^-24)."""
    w, g = _gaps(bins)
    return np.float64(np.nan) if g.size == 0 else np.float64(np.sum(w * g))


def mce_of(bins):
    """Maximum calibration error: the largest |accuracy_k - confidence_k| over the non-empty bins; NaN when N == 0."""
    _, g = _gaps(bins)
    return np.float64(np.nan) if g.size == 0 else np.float64(g.max())


def accuracy_of(bins):
    """sum(correct) / sum(total): the reference's aAcc (labels outside [0, C) take no part); NaN when N == 0."""
    b = _bins3(bins)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.float64(b[1].sum()) / np.float64(b[0].sum())


def mean_confidence_of(bins):
    """sum(conf_sum) / (2^24 sum(total)); NaN when N == 0.  Summed as Python integers: K bins below 2^63 each may pass 2^63 together."""
    b = _bins3(bins)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.float64(sum(int(v) for v in b[2])) / (np.float64(CONF_ONE) * np.float64(b[0].sum()))


def risk_coverage_of(bins):
    """Accuracy against coverage -> (coverage float64 [K], selective_accuracy float64 [K]): entry k keeps the bins k .. K - 1 (confidence >= k / K),
    coverage_k = kept / N, selective_accuracy_k = correct among the kept / kept (NaN where nothing is kept).  Entry 0 is (1, accuracy)."""
    b = _bins3(bins)
    kept = np.cumsum(b[0][::-1])[::-1].astype(np.float64)
    good = np.cumsum(b[1][::-1])[::-1].astype(np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        return kept / np.float64(b[0].sum()), good / kept


def calibration_summary_of(bins):
    """ECE, MCE, aAcc and the mean confidence in PERCENT, rounded to two places as `summary_of` rounds (np.round(v * 100, 2)); NaN when N == 0."""
    vals = (("ECE", ece_of(bins)), ("MCE", mce_of(bins)), ("aAcc", accuracy_of(bins)), ("mConf", mean_confidence_of(bins)))
    return OrderedDict((k, np.round(v * 100, 2)) for k, v in vals)


# ---- temperature scaling: the scalar the kernels take, the grids, and the metrics of a sweep's integers (numpy, float64) ----
def inv_temperature(T):
    """The inverse temperature the `_t` kernels and the sweep multiply by: float32(1 / float64(T)) -> a Python float that holds that float32 exactly.
    T must be finite and positive and the float32 must come out finite and positive (T = 1e-40 or 1e50 do not), else ValueError."""
    if isinstance(T, bool) or not isinstance(T, (int, float, np.integer, np.floating)):
        raise ValueError(f"mmsa.evaluate: temperature = {T!r}; a finite number > 0 is expected")
    t = np.float64(T)
    if not np.isfinite(t) or not t > 0:
        raise ValueError(f"mmsa.evaluate: temperature = {T!r}; a finite number > 0 is expected")
    with np.errstate(over="ignore", under="ignore"):
        it = np.float32(np.float64(1.0) / t)
    if not np.isfinite(it) or not it > 0:
        raise ValueError(f"mmsa.evaluate: temperature = {T!r}: its inverse {float(np.float64(1.0) / t)!r} is not a finite positive float32")
    return float(it)


SCORES = {"max": 0, "margin": 1, "entropy": 2}      # `score=` of the class-map entries -> `kind` of the score launches (0: the confidence launches)


def inv_log_classes(C):
    """The factor of the entropy score 1 - H / log C (csrc/softmax_px.h): float32(1 / log(float64(C))) -> a Python float that holds that float32 exactly; 0 for
    one class, whose entropy is 0 and whose score is 1."""
    if not _is_int(C, 1, math.inf):
        raise ValueError(f"mmsa.evaluate: {C!r} classes; a positive integer is expected")
    return 0.0 if int(C) == 1 else float(np.float32(np.float64(1.0) / np.log(np.float64(int(C)))))


def geometric_grid(lo, hi, J):
    """J temperatures from lo to hi with a constant ratio, float64 [J] (J == 1: [lo]); both ends are exact.  0 < lo <= hi, 1 <= J <= 16.  A first sweep
    over a wide grid and a second over geometric_grid(T / r, T * r, J) around its best() is the whole fit."""
    if not _is_int(J, 1, MAX_TEMPERATURES):
        raise ValueError(f"mmsa.evaluate: J = {J!r}; 1..{MAX_TEMPERATURES} temperatures per sweep")
    lo, hi = np.float64(lo), np.float64(hi)
    if not (np.isfinite(lo) and np.isfinite(hi) and 0 < lo <= hi):
        raise ValueError(f"mmsa.evaluate: a temperature grid needs finite 0 < lo <= hi, got {float(lo)!r}, {float(hi)!r}")
    J = int(J)
    if J == 1:
        return np.array([lo], dtype=np.float64)
    g = lo * (hi / lo) ** (np.arange(J, dtype=np.float64) / (J - 1))
    g[0], g[-1] = lo, hi
    return g


def _sweep4(sweep):
    """int64 [J, 4, K] (per temperature: total, correct, conf_sum, nll_sum) of one slot, checked."""
    s = np.asarray(sweep)
    if s.ndim != 3 or s.shape[1] != 4 or s.shape[0] < 1 or s.shape[2] < 1 or s.dtype.kind not in "iu":
        raise ValueError(f"mmsa.evaluate: a temperature sweep is an integer [J, 4, K] array (total, correct, conf_sum, nll_sum per temperature), got {s.dtype} {s.shape}")
    s = s.astype(np.int64, copy=False)
    if s.size and int(s.min()) < 0:
        raise OverflowError("mmsa.evaluate: a cell of the temperature sweep is negative: an int64 sum has wrapped (read and reset() the TemperatureSweep more often)")
    return s


def sweep_bins_of(sweep, j):
    """Calibration's int64 [3, K] bins at temperature j of an int64 [J, 4, K] sweep: what reliability_of / ece_of / mce_of / risk_coverage_of take."""
    s = _sweep4(sweep)
    if not _is_int(j, 0, s.shape[0] - 1):
        raise ValueError(f"mmsa.evaluate: temperature index j = {j!r}; 0..{s.shape[0] - 1}")
    return s[int(j), :3].copy()


def sweep_nll_of(sweep):
    """The mean NLL per temperature, float64 [J]: sum_k nll_sum / (2^20 * sum_k total); NaN when nothing took part.  Below the float64 mean of the
    float32 per-pixel values by less than 2^-20 (every term is truncated to 20 fractional bits).  Summed as Python integers."""
    s = _sweep4(sweep)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.array([np.float64(sum(int(v) for v in one[3])) / (np.float64(NLL_ONE) * np.float64(one[0].sum())) for one in s], dtype=np.float64)


def sweep_ece_of(sweep):
    """`ece_of` per temperature, float64 [J]."""
    s = _sweep4(sweep)
    return np.array([ece_of(one[:3]) for one in s], dtype=np.float64)


def sweep_best_of(sweep, temperatures, by="nll"):
    """(T, j) of the grid's minimum of the mean NLL (`by`="nll") or of the ECE ("ece"); the FIRST minimum wins.  ValueError when nothing took part."""
    if by not in ("nll", "ece"):
        raise ValueError(f"mmsa.evaluate: best(by={by!r}); 'nll' or 'ece'")
    v = sweep_nll_of(sweep) if by == "nll" else sweep_ece_of(sweep)
    t = np.asarray(temperatures, dtype=np.float64)
    if t.shape != v.shape:
        raise ValueError(f"mmsa.evaluate: {t.size} temperatures for a sweep of {v.size}")
    if np.isnan(v).any():
        raise ValueError("mmsa.evaluate: the sweep has no participating pixel (or a NaN metric): there is no best temperature")
    j = int(np.argmin(v))
    return float(t[j]), j


# ---- selective evaluation from the per-bin confusion counts (numpy; integers, then float64) ----
def _counts3(counts):
    """int64 [K, C + 1, C + 1] of one slot, checked; OverflowError where a cell is negative (an int64 count that has wrapped)."""
    c = np.asarray(counts)
    if c.ndim != 3 or c.shape[0] < 1 or c.shape[1] != c.shape[2] or c.shape[1] < 3 or c.dtype.kind not in "iu":
        raise ValueError(f"mmsa.evaluate: selective counts are an integer [K, C + 1, C + 1] array, got {c.dtype} {c.shape}")
    if c.dtype.kind == "u" and c.size and int(c.max()) > np.iinfo(np.int64).max:
        raise OverflowError(f"mmsa.evaluate: a selective count of {int(c.max())} does not fit int64")
    c = c.astype(np.int64, copy=False)
    if c.size and int(c.min()) < 0:
        raise OverflowError("mmsa.evaluate: a selective count is negative: an int64 cell has wrapped (read and reset() the SelectiveEvaluator more often)")
    return c


def _sum_bins(c):
    """c.sum(0) of checked counts [k, C + 1, C + 1] in int64.  Where the float64 estimate of the largest sum comes near 2^63 the cells are summed as
    Python integers instead, and OverflowError is raised if one of them has passed it."""
    if c.shape[0] == 0 or float(c.astype(np.float64).sum(0).max()) < 2.0 ** 62:
        return c.sum(0)
    s = c.astype(object).sum(0)
    if int(s.max()) > np.iinfo(np.int64).max:
        raise OverflowError(f"mmsa.evaluate: the selective counts of one cell sum to {int(s.max())} over the bins, which int64 cannot hold")
    return s.astype(np.int64)


def _suffix_sums(c):
    """S[k] = c[k:].sum(0) of checked counts, int64 [K, C + 1, C + 1]; no cell of an S[k] exceeds S[0]'s, which _sum_bins checks."""
    _sum_bins(c)
    return np.cumsum(c[::-1], axis=0)[::-1].copy()


def selective_counts_of(counts, min_bin=0):
    """The confusion counts of the pixels kept at `min_bin`: counts[min_bin:].sum(0), int64 [C + 1, C + 1]; min_bin == K keeps nothing.  (The map
    `abstain` writes at min_bin has these counts with the row sums of counts[:min_bin] added into column C: its abstained pixels predict 255.)"""
    c = _counts3(counts)
    K = c.shape[0]
    if not _is_int(min_bin, 0, K):
        raise ValueError(f"mmsa.evaluate: min_bin = {min_bin!r}; 0..{K} for {K} bins")
    return _sum_bins(c[int(min_bin):])


def selective_areas_of(counts):
    """(area_intersect, area_union, area_pred_label, area_label) per threshold, int64 [K, C] each: entry k keeps the bins k .. K - 1 (`areas_of` on the
    suffix sums)."""
    return areas_of(_suffix_sums(_counts3(counts)))


def selective_metrics_of(counts, metric=("mIoU",), nan_to_num=None, beta=1):
    """The reference's metrics against coverage from int64 [K, C + 1, C + 1] counts -> OrderedDict: 'coverage' float64 [K] (entry k keeps the bins
    k .. K - 1; kept / all pixels whose label row is < C: numerator and denominator of `risk_coverage_of`), `area_metrics`' entries stacked per
    threshold ('aAcc' [K], 'IoU' / 'Acc' / ... [K, C]) and their np.nanmean per threshold ('mIoU', 'mAcc', ... [K]).  Entry 0 is
    area_metrics(*areas_of(counts.sum(0))); a threshold that keeps nothing gives NaN.  'aAcc' at threshold k is sum(intersect) / sum(area_label[:C])
    over the kept pixels -- `risk_coverage_of`'s selective accuracy, since kept pixels of the label rows < C are exactly Calibration's `total`."""
    c = _counts3(counts)
    C = c.shape[1] - 1
    S = _suffix_sums(c)
    kept = S[:, :C, :].sum((1, 2))
    areas = areas_of(S)
    per = [area_metrics(*(a[k] for a in areas), metric=metric, nan_to_num=nan_to_num, beta=beta) for k in range(S.shape[0])]
    with np.errstate(divide="ignore", invalid="ignore"):
        out = OrderedDict(coverage=kept.astype(np.float64) / np.float64(kept[0]))
    for key in per[0]:
        out[key] = np.stack([np.asarray(m[key], dtype=np.float64) for m in per])
    for key in list(per[0]):
        if key != "aAcc":
            with warnings.catch_warnings():
                warnings.simplefilter("ignore", RuntimeWarning)                   # "Mean of empty slice": a threshold where every class is NaN gives NaN
                out["m" + key] = np.nanmean(out[key], axis=1)
    return out


AUC_METRICS = ("risk", "mIoU", "aAcc")


def selective_auc_of(counts, metric="risk"):
    """The area under a selective curve of int64 [K, C + 1, C + 1] counts, one float64: `metric` = 'risk' (1 - aAcc: the AURC, lower is better), 'mIoU' or
    'aAcc' (higher is better) against coverage, from the K points `selective_metrics_of` gives at the thresholds k / K.  The rule:
      thresholds whose coverage is 0 are dropped (they keep nothing; their metric is NaN);
      the others are taken in threshold order, which is coverage descending from coverage 1 at k = 0 (empty bins repeat a point: zero width);
      the metric is integrated over coverage with the trapezoid rule between neighbouring points;
      from the smallest non-zero coverage down to coverage 0 the curve is extended FLAT with that point's value (the bins cannot order the pixels inside
        the top bin, so every coverage below it is served by a random subset of it, whose expected metric -- for aAcc and risk -- is the bin's own).
    A NaN metric at a kept point makes the result NaN, and so does a curve without a kept point (no pixel took part).  The value is a mean of the metric over
    coverage in [0, 1]: a score that ranks the errors last has a smaller AURC / a larger area under mIoU on the same maps."""
    if metric not in AUC_METRICS:
        raise ValueError(f"mmsa.evaluate: selective_auc_of(metric={metric!r}); one of {AUC_METRICS}")
    m = selective_metrics_of(counts, metric=("mIoU",))
    cov = m["coverage"]
    val = 1.0 - m["aAcc"] if metric == "risk" else m[metric]
    keep = cov > 0                                                        # False for NaN (nothing took part at all)
    cov, val = cov[keep], np.asarray(val, dtype=np.float64)[keep]
    if cov.size == 0:
        return np.float64("nan")
    area = np.float64(0.0)
    for i in range(cov.size - 1):
        area += (cov[i] - cov[i + 1]) * (val[i] + val[i + 1]) / 2.0
    return np.float64(area + cov[-1] * val[-1])


def reliability_counts_of(counts):
    """Calibration's first two rows from the per-bin confusion counts: int64 [..., 2, K] (total, correct) of [..., K, C + 1, C + 1] counts -- total[k] = the
    sum of the rows < C of bin k, correct[k] = the trace of its [:C, :C] block."""
    c = np.asarray(counts)
    if c.ndim < 3 or c.shape[-1] != c.shape[-2] or c.shape[-1] < 3 or c.dtype.kind not in "iu":
        raise ValueError(f"mmsa.evaluate: selective counts are an integer [..., K, C + 1, C + 1] array, got {c.dtype} {c.shape}")
    c = c.astype(np.int64, copy=False)
    C = c.shape[-1] - 1
    return np.stack([c[..., :C, :].sum((-2, -1)), np.trace(c[..., :C, :C], axis1=-2, axis2=-1)], axis=-2)


def bin_of(conf, bins):
    """The bin of confidences as the device forms it (csrc/conf_bin.h): clamp (NaN, negatives, -0.0 -> 0; above 1 -> 1), ONE float32 product, truncated,
    capped at bins - 1 -> int64 array."""
    c = np.asarray(conf, dtype=np.float32)
    with np.errstate(invalid="ignore"):
        c = np.where(c > 0, np.minimum(c, np.float32(1)), np.float32(0)).astype(np.float32)
    return np.minimum(int(bins) - 1, (c * np.float32(bins)).astype(np.int64))


def bin_edge(j, bins):
    """The lower edge of bin j as the device sees it: the smallest float32 confidence whose bin is >= j (j / bins, or its float32 neighbour where the
    product rounds); 0 <= j <= bins - 1."""
    e = np.float32(j / bins)
    while e > 0 and bin_of(np.nextafter(e, np.float32(0)), bins) >= j:
        e = np.nextafter(e, np.float32(0))
    while bin_of(e, bins) < j:
        e = np.nextafter(e, np.float32(1))
    return e


def threshold_bin(threshold, bins):
    """`threshold=` of `abstain` -> min_bin.  The threshold (rounded to float32) goes through the SAME float32 product as a confidence, and must be a bin
    edge: the smallest float32 of its bin, so that 'bin >= min_bin' and 'confidence >= threshold' are the same pixels and the map agrees with the
    per-bin counts.  Anything else raises ValueError naming the nearest edges."""
    K = _check_bins(bins)
    if isinstance(threshold, bool) or not isinstance(threshold, (int, float, np.integer, np.floating)) or not 0 <= float(threshold) <= 1:
        raise ValueError(f"mmsa.evaluate: threshold = {threshold!r}; a confidence in [0, 1] is expected")
    t = np.float32(threshold)
    j = int(bin_of(t, K))
    if t != bin_edge(j, K):
        lo, hi = float(bin_edge(j, K)), (float(bin_edge(j + 1, K)) if j + 1 < K else None)
        nxt = f"{hi!r} (min_bin {j + 1})" if hi is not None else f"min_bin={K} (abstain everywhere)"
        raise ValueError(f"mmsa.evaluate: threshold {float(threshold)!r} is not a bin edge of {K} bins: the map would keep a part of bin {j} that the per-bin "
                         f"counts cannot split; the nearest edges are {lo!r} (min_bin {j}) and {nxt}")
    return j


# ---- the label side of a launch ----
class LabelPrep:
    """How a raw uint8 label map [B, Hl, Wl] is read against a prediction: the LUT of `label_map` / `reduce_zero_label` / `ignore_index`, and `resize` =
    dict(seg_scale=(w, h) or img_scale=(w, h), keep_ratio=True) of a `Resize_multimodal` step the ground truth goes through (transform.py:1169-1188:
    `seg_scale` where given, else the image scale; mmcv.imrescale / imresize with interpolation='nearest').  LUT and index tables are built in numpy,
    uploaded once per device / geometry and kept on the object: a later call with the same geometry allocates and copies nothing and can be captured."""

    def __init__(self, num_classes, ignore_index=255, label_map=None, reduce_zero_label=False, resize=None):
        self.num_classes = int(num_classes)
        self.ignore_index, self.label_map, self.reduce_zero_label = ignore_index, dict(label_map or {}), bool(reduce_zero_label)
        self.lut = label_lut(num_classes, ignore_index, label_map, reduce_zero_label)
        if resize is not None:
            sc = resize.get("seg_scale")
            if sc is None or list(sc) == [None]:
                sc = resize.get("img_scale")
            if isinstance(sc, list) and len(sc) == 1:
                sc = sc[0]
            if sc is None or len(sc) != 2 or isinstance(sc[0], (list, tuple)) or resize.get("ratio_range") is not None:
                raise NotImplementedError("mmsa.LabelPrep: resize needs one seg_scale=(w, h) or img_scale=(w, h); a ratio range or several scales are not built")
            resize = dict(scale=(int(sc[0]), int(sc[1])), keep_ratio=bool(resize.get("keep_ratio", True)))
        self.resize = resize
        self._lut_dev = {}      # device -> LUT
        self._tables = {}       # (Hl, Wl, H, W, device) -> (ymap, xmap)

    @classmethod
    def from_pipeline(cls, test_pipeline, num_classes, ignore_index=255, label_map=None, reduce_zero_label=False):
        """From a reference config's `test_pipeline`.  The ground truth goes through `transforms[1 : index of MultiScaleFlipAug]` behind LoadAnnotations
        (DELIVER.py:199-203): a `Resize_multimodal` there resizes it (seg_scale / img_scale / keep_ratio are read); a `Pad_multimodal` there leaves it
        as it is (without an image in `results` its `_pad_img` raises before 'pad_shape' exists, `_pad_seg` then raises too, and both are swallowed:
        transform.py:2968-3011).  Any other step there raises NotImplementedError naming it."""
        idx = next((k for k, st in enumerate(test_pipeline) if st.get("type") == "MultiScaleFlipAug"), None)
        if idx is None:
            raise NotImplementedError("mmsa.LabelPrep.from_pipeline: the pipeline has no MultiScaleFlipAug step (the ground-truth steps are the ones in front of it)")
        resize = None
        for st in test_pipeline[1:idx]:
            t = st.get("type")
            if t == "Resize_multimodal":
                if resize is not None:
                    raise NotImplementedError("a second Resize_multimodal step in front of MultiScaleFlipAug")
                if st.get("ratio_range") is not None or st.get("img_scale") is None or isinstance(st["img_scale"][0], (list, tuple)):
                    raise NotImplementedError("Resize_multimodal with a ratio range or several scales (only one fixed scale has a device form)")
                resize = dict(img_scale=tuple(st["img_scale"]), seg_scale=st.get("seg_scale"), keep_ratio=bool(st.get("keep_ratio", True)))
            elif t == "Pad_multimodal":
                continue
            else:
                raise NotImplementedError(f"pipeline step '{t}' in front of MultiScaleFlipAug has no device form in mmsa.LabelPrep")
        return cls(num_classes, ignore_index=ignore_index, label_map=label_map, reduce_zero_label=reduce_zero_label, resize=resize)

    def resized(self, Hl, Wl):
        """(H, W) of an Hl x Wl label map after the resize step (its own size without one)."""
        if self.resize is None:
            return Hl, Wl
        sc = self.resize["scale"]
        return rescale_size(Hl, Wl, sc) if self.resize["keep_ratio"] else (sc[1], sc[0])

    def check(self, labels, device=None):
        if not isinstance(labels, torch.Tensor) or not labels.is_cuda:
            raise RuntimeError("mmsa.evaluate: labels must be a GPU tensor (there is no CPU path)")
        if labels.dtype != torch.uint8:
            raise RuntimeError(f"mmsa.evaluate: labels are {labels.dtype}; raw uint8 label maps are expected")
        if labels.dim() != 3 or not labels.is_contiguous():
            raise RuntimeError(f"mmsa.evaluate: labels must be a contiguous [B, H, W] tensor, got {tuple(labels.shape)}")
        if device is not None and labels.device != device:
            raise RuntimeError(f"mmsa.evaluate: labels are on {labels.device}, the prediction on {device}")
        return labels

    def tables(self, Hl, Wl, H, W, device):
        """(ymap, xmap) int32 device tables of the nearest-neighbour resize Hl x Wl -> H x W, or (None, None) where the sizes are equal."""
        if (Hl, Wl) == (H, W):
            return None, None
        key = (Hl, Wl, H, W, torch.device(device))
        tabs = self._tables.get(key)
        if tabs is None:
            if _capturing(key[-1]):
                raise RuntimeError(f"mmsa.LabelPrep: the label tables for {Hl} x {Wl} -> {H} x {W} are not on the device yet and cannot be uploaded during a "
                                   "graph capture: run one call with this geometry before capturing")
            tabs = tuple(torch.from_numpy(nearest_axis_table(s, d)).to(key[-1]) for s, d in ((Hl, H), (Wl, W)))
            self._tables[key] = tabs
        return tabs

    def lut_on(self, device):
        device = torch.device(device)
        t = self._lut_dev.get(device)
        if t is None:
            if _capturing(device):
                raise RuntimeError("mmsa.LabelPrep: the label LUT is not on the device yet and cannot be uploaded during a graph capture: run one call before capturing")
            t = self._lut_dev[device] = torch.from_numpy(self.lut).to(device)
        return t

    def launch_args(self, labels, B, H, W, device):
        """The label-side arguments of both entries for a [B, H, W] prediction: (label, Hl, Wl, lut, ymap, xmap)."""
        labels = self.check(labels, device)
        Hl, Wl = int(labels.shape[1]), int(labels.shape[2])
        if labels.shape[0] != B:
            raise RuntimeError(f"mmsa.evaluate: {labels.shape[0]} label maps for {B} predictions")
        if self.resized(Hl, Wl) != (H, W):
            how = "" if self.resize is None else f" (resized to {self.resized(Hl, Wl)[0]} x {self.resized(Hl, Wl)[1]} by scale={self.resize['scale']}, keep_ratio={self.resize['keep_ratio']})"
            raise RuntimeError(f"mmsa.evaluate: size mismatch: the label maps are {Hl} x {Wl}{how}, the prediction is {H} x {W}")
        ymap, xmap = self.tables(Hl, Wl, H, W, device)
        return (labels.data_ptr(), Hl, Wl, self.lut_on(device).data_ptr(), None if ymap is None else ymap.data_ptr(), None if xmap is None else xmap.data_ptr())


def _slot_args(slots, B, n_slots):
    slots = list(range(B)) if slots is None else [int(s) for s in slots]
    if len(slots) != B:
        raise RuntimeError(f"mmsa.evaluate: {len(slots)} slots for {B} images")
    if B > MAX_IMAGES:
        raise RuntimeError(f"mmsa.evaluate: at most {MAX_IMAGES} images per call, got {B}")
    if any(not 0 <= s < n_slots for s in slots):
        raise RuntimeError(f"mmsa.evaluate: slots {slots} outside the {n_slots} count slots")
    return (ctypes.c_int * B)(*slots)


def _check_buffer(buf, name, shape, device):
    """`buf` is a pass's result buffer: a contiguous int64 [n_slots, *shape] tensor on `device`."""
    if (not isinstance(buf, torch.Tensor) or buf.dtype != torch.int64 or buf.dim() != len(shape) + 1 or tuple(buf.shape[1:]) != tuple(shape)
            or buf.device != device or not buf.is_contiguous()):
        raise RuntimeError(f"mmsa.evaluate: {name} must be a contiguous int64 [n_slots, {', '.join(str(v) for v in shape)}] tensor on {device}")
    return buf


def _check_out(out, dtype, shape, device):
    """A caller's out= of an entry that writes a whole map: a contiguous tensor of this dtype and shape on `device`."""
    if not isinstance(out, torch.Tensor) or out.dtype != dtype or tuple(out.shape) != tuple(shape) or out.device != device or not out.is_contiguous():
        raise RuntimeError(f"mmsa.evaluate: out must be a contiguous {str(dtype).replace('torch.', '')} {tuple(shape)} tensor on {device}")
    return out


def _check_scratch(scratch, dtype, n, device=None, avoid=None, count=None):
    """A caller's scratch=: a contiguous tensor of `dtype` with at least n elements (`count`: how the message spells n), on `device` where one is given (None:
    the device is looked at later), and not the tensor `avoid`, the call's `out`."""
    if (not isinstance(scratch, torch.Tensor) or scratch.dtype != dtype or scratch.numel() < n or not scratch.is_contiguous()
            or (device is not None and scratch.device != device) or (avoid is not None and scratch.data_ptr() == avoid.data_ptr())):
        raise RuntimeError(f"mmsa.evaluate: scratch must be a contiguous {str(dtype).replace('torch.', '')} tensor of at least {count or n} elements"
                           f"{'' if device is None else f' on {device}'}{'' if avoid is None else ', and not `out`'}")
    return scratch


def _slot_launch(prep, labels, B, H, W, device, buf, name, shape, slots, default=True):
    """What every launch into an int64 [n_slots, *shape] buffer does before its `lib.call`, in the caller's device guard: the label side of a [B, H, W]
    map checked, the buffer `name` allocated where none is given (zeroed, max(slots) + 1 slots; `default=False`: an entry without that default) and
    checked, the slots checked against it -> (LabelPrep.launch_args, the buffer, the slot table)."""
    largs = prep.launch_args(labels, B, H, W, device)
    if buf is None and default:
        n_slots = B if slots is None else max(int(s) for s in slots) + 1
        buf = torch.zeros(n_slots, *shape, dtype=torch.int64, device=device)
    _check_buffer(buf, name, shape, device)
    return largs, buf, _slot_args(slots, B, buf.shape[0])


def _check_pred(pred):
    if not isinstance(pred, torch.Tensor) or not pred.is_cuda:
        raise RuntimeError("mmsa.evaluate: pred must be a GPU tensor (there is no CPU path)")
    if pred.dtype != torch.uint8:
        raise RuntimeError(f"mmsa.evaluate: pred is {pred.dtype}; a uint8 class map is expected")
    if pred.dim() != 3 or not pred.is_contiguous():
        raise RuntimeError(f"mmsa.evaluate: pred must be a contiguous [B, H, W] tensor, got {tuple(pred.shape)}")
    return pred


def _check_confmap(conf, pred):
    """The confidence map of `pred`: a contiguous float32 [B, H, W] GPU tensor on pred's device with pred's shape (what `confidence=` returns)."""
    if not isinstance(conf, torch.Tensor) or not conf.is_cuda:
        raise RuntimeError("mmsa.evaluate: conf must be a GPU tensor (there is no CPU path)")
    if conf.dtype != torch.float32:
        raise RuntimeError(f"mmsa.evaluate: conf is {conf.dtype}; a float32 confidence map is expected")
    if conf.device != pred.device:
        raise RuntimeError(f"mmsa.evaluate: conf is on {conf.device}, pred on {pred.device}")
    if tuple(conf.shape) != tuple(pred.shape):
        raise RuntimeError(f"mmsa.evaluate: conf has shape {tuple(conf.shape)}, pred is [B, H, W] = {tuple(pred.shape)}")
    if not conf.is_contiguous():
        raise RuntimeError("mmsa.evaluate: conf must be contiguous (its layout is the class map's)")
    return conf


def _check_bins(bins):
    if not _is_int(bins, 1, MAX_BINS):
        raise ValueError(f"mmsa.evaluate: bins = {bins!r}; 1..{MAX_BINS} confidence bins are supported")
    return int(bins)


def _check_selective_classes(C):
    if C > MAX_SELECTIVE_CLASSES:
        raise RuntimeError(f"mmsa.evaluate: {C} classes; selective evaluation supports 2..{MAX_SELECTIVE_CLASSES} (one bin's (C + 1)^2 uint32 histogram must "
                           "fit a workgroup's 64 KiB of LDS)")
    return C


def _default_bins(bins, buf, k_axis, ndim):
    """`bins=` of an entry with confidence bins: K itself, by default that of the buffer given (axis `k_axis` of its `ndim` axes), or 15."""
    if bins is None:
        bins = int(buf.shape[k_axis]) if isinstance(buf, torch.Tensor) and buf.dim() == ndim else DEFAULT_BINS
    return _check_bins(bins)


@torch.no_grad()
def confusion(pred, labels, prep, counts=None, slots=None):
    """ADD the confusion counts of the uint8 class maps pred [B, H, W] against the raw labels [B, Hl, Wl] into counts[slots[b]] (one launch,
    mmsa_eval_confusion_u8) -> counts, int64 [n_slots, C + 1, C + 1] on the device.  `slots` defaults to 0 .. B - 1 (per-image counts, as `pre_eval`
    returns them); `counts` defaults to a zeroed buffer of max(slots) + 1 slots."""
    pred = _check_pred(pred)
    B, H, W = (int(v) for v in pred.shape)
    C = prep.num_classes
    with torch.cuda.device(pred.device):
        largs, counts, tab = _slot_launch(prep, labels, B, H, W, pred.device, counts, "counts", (C + 1, C + 1), slots)
        lib.call("mmsa_eval_confusion_u8", pred.data_ptr(), largs[0], B, H, W, largs[1], largs[2], largs[3], C, largs[4], largs[5], tab, counts.shape[0],
                 counts.data_ptr(), ops._stream())
    return counts


@torch.no_grad()
def calibration(pred, conf, labels, prep, bins=None, cal=None, slots=None):
    """ADD the reliability bins of the uint8 class maps pred [B, H, W] and their float32 confidence maps conf [B, H, W] against the raw labels
    [B, Hl, Wl] into cal[slots[b]] (one launch, mmsa_eval_calibration) -> cal, int64 [n_slots, 3, K] on the device, rows total / correct / conf_sum.
    A pixel takes part iff its transformed label is a class (< C); it is correct iff pred equals it; its bin is min(K - 1, int(float32(c) * float32(K)))
    of its confidence c clamped to [0, 1] (NaN -> 0); conf_sum adds floor(c * 2^24).  `bins` = K defaults to cal's, or to 15; `slots` defaults to
    0 .. B - 1 (per-image bins); `cal` defaults to a zeroed buffer of max(slots) + 1 slots."""
    pred = _check_pred(pred)
    conf = _check_confmap(conf, pred)
    B, H, W = (int(v) for v in pred.shape)
    C = prep.num_classes
    bins = _default_bins(bins, cal, 2, 3)
    with torch.cuda.device(pred.device):
        largs, cal, tab = _slot_launch(prep, labels, B, H, W, pred.device, cal, "cal", (3, bins), slots)
        lib.call("mmsa_eval_calibration", pred.data_ptr(), conf.data_ptr(), largs[0], B, H, W, largs[1], largs[2], largs[3], C, largs[4], largs[5], tab,
                 cal.shape[0], bins, cal.data_ptr(), ops._stream())
    return cal


@torch.no_grad()
def selective(pred, conf, labels, prep, bins=None, counts=None, slots=None):
    """ADD one confusion matrix per confidence bin of the uint8 class maps pred [B, H, W] and their float32 confidence maps conf [B, H, W] against the raw
    labels [B, Hl, Wl] into counts[slots[b]] (one launch, mmsa_eval_selective) -> counts, int64 [n_slots, K, C + 1, C + 1] on the device:
    counts[s, k, row, col] += 1 for every pixel whose label is not ignored, row / col as in `confusion` (index C = outside [0, C)), k as in `calibration`
    (min(K - 1, int(float32(c) * float32(K))) of the confidence clamped to [0, 1], NaN -> 0).  `bins` = K defaults to counts', or to 15; `slots` defaults
    to 0 .. B - 1 (per-image counts); `counts` defaults to a zeroed buffer of max(slots) + 1 slots."""
    pred = _check_pred(pred)
    conf = _check_confmap(conf, pred)
    B, H, W = (int(v) for v in pred.shape)
    C = _check_selective_classes(prep.num_classes)
    bins = _default_bins(bins, counts, 1, 4)
    with torch.cuda.device(pred.device):
        largs, counts, tab = _slot_launch(prep, labels, B, H, W, pred.device, counts, "counts", (bins, C + 1, C + 1), slots)
        lib.call("mmsa_eval_selective", pred.data_ptr(), conf.data_ptr(), largs[0], B, H, W, largs[1], largs[2], largs[3], C, largs[4], largs[5], tab,
                 counts.shape[0], bins, counts.data_ptr(), ops._stream())
    return counts


def _check_logits(logits):
    if not isinstance(logits, torch.Tensor) or not logits.is_cuda:
        raise RuntimeError("mmsa.evaluate: logits must be a GPU tensor (there is no CPU path)")
    if logits.dtype != torch.float32:
        raise RuntimeError(f"mmsa.evaluate: logits are {logits.dtype}; a float32 logits canvas is expected")
    if logits.dim() != 4 or not logits.is_contiguous():
        raise RuntimeError(f"mmsa.evaluate: logits must be a contiguous [B, C, H, W] tensor, got {tuple(logits.shape)}")
    return logits


def _inv_temperatures(temperatures):
    """`temperatures` (a sequence of 1..16 numbers) -> the inverse temperatures as Python floats, each checked by `inv_temperature`."""
    ts = [temperatures] if isinstance(temperatures, (int, float, np.integer, np.floating)) and not isinstance(temperatures, bool) else list(temperatures)
    if not 1 <= len(ts) <= MAX_TEMPERATURES:
        raise ValueError(f"mmsa.evaluate: {len(ts)} temperatures; 1..{MAX_TEMPERATURES} per sweep (sweep a longer grid in parts)")
    return [inv_temperature(t) for t in ts]


@torch.no_grad()
def temperature_sweep(logits, labels, prep, temperatures, bins=None, out=None, slots=None):
    """ADD the sweep of the float32 logits canvas [B, C, H, W] against the raw labels [B, Hl, Wl] over `temperatures` (1..16) into out[slots[b]] (one
    launch, mmsa_temperature_sweep_nchw) -> out, int64 [n_slots, J, 4, K] on the device: per temperature j, rows total / correct / conf_sum (what
    `calibration` gives for the canvas path's class map and its confidence at T_j, bit for bit) and nll_sum = the sum of floor(min(max(nll, 0), 1024) * 2^20),
    nll = -log softmax(x / T_j)[label class].  A pixel takes part iff its transformed label is a class (< C).  `bins` = K defaults to out's, or to 15;
    `slots` defaults to 0 .. B - 1 (per-image sweeps); `out` defaults to a zeroed buffer of max(slots) + 1 slots."""
    logits = _check_logits(logits)
    B, C, H, W = (int(v) for v in logits.shape)
    if C != prep.num_classes:
        raise RuntimeError(f"mmsa.evaluate: the logits have {C} classes, the LabelPrep {prep.num_classes}")
    its = _inv_temperatures(temperatures)
    J = len(its)
    bins = _default_bins(bins, out, 3, 4)
    with torch.cuda.device(logits.device):
        largs, out, tab = _slot_launch(prep, labels, B, H, W, logits.device, out, "out", (J, 4, bins), slots)
        lib.call("mmsa_temperature_sweep_nchw", logits.data_ptr(), largs[0], B, C, H, W, largs[1], largs[2], largs[3], largs[4], largs[5], tab, out.shape[0],
                 (ctypes.c_float * J)(*its), J, bins, out.data_ptr(), ops._stream())
    return out


@torch.no_grad()
def abstain(pred, conf, bins, min_bin=None, out=None, threshold=None):
    """The class map thresholded by confidence (one launch, mmsa_abstain_u8) -> uint8 [B, H, W]: pred where the confidence's bin (of `bins`, as in
    `selective` / `calibration`) is >= `min_bin`, 255 elsewhere.  0 <= min_bin <= bins: 0 copies, `bins` abstains everywhere.  `threshold=` in place
    of min_bin: a confidence in [0, 1] that is a bin edge (`threshold_bin`); any other is refused, since the per-bin counts cannot describe its map.
    `out`: the uint8 tensor to write, pred's shape; it may be pred itself (in place); a new tensor by default.
    `fill_nearest(out, hole=255)` then gives the abstained pixels the class of the nearest kept pixel."""
    pred = _check_pred(pred)
    conf = _check_confmap(conf, pred)
    K = _check_bins(bins)
    if (min_bin is None) == (threshold is None):
        raise ValueError("mmsa.evaluate: abstain takes min_bin= or threshold=, one of them")
    if threshold is not None:
        min_bin = threshold_bin(threshold, K)
    if not _is_int(min_bin, 0, K):
        raise ValueError(f"mmsa.evaluate: min_bin = {min_bin!r}; 0..{K} for {K} bins ({K} abstains everywhere)")
    with torch.cuda.device(pred.device):
        out = torch.empty_like(pred) if out is None else _check_out(out, torch.uint8, pred.shape, pred.device)
        if pred.numel():
            lib.call("mmsa_abstain_u8", pred.data_ptr(), conf.data_ptr(), pred.numel(), K, int(min_bin), out.data_ptr(), ops._stream())
    return out


@torch.no_grad()
def slide_argmax_eval(lg, n, windows, out, B, H, W, hc, wc, unc, labels, prep, counts, slots=None):
    """mmsa_slide_argmax on the head-resolution logits lg [n, C, hs, ws] AND the counts of its class map in one launch; `out` = None writes no map."""
    C = int(lg.shape[1])
    if C != prep.num_classes:
        raise RuntimeError(f"mmsa.evaluate: the head has {C} classes, the LabelPrep {prep.num_classes}")
    largs, counts, tab = _slot_launch(prep, labels, B, H, W, lg.device, counts, "counts", (C + 1, C + 1), slots, default=False)
    lib.call("mmsa_slide_argmax_eval", lg.data_ptr(), n, C, lg.shape[2], lg.shape[3], windows, None if out is None else out.data_ptr(), B, H, W, hc, wc,
             unc.data_ptr(), largs[0], largs[1], largs[2], largs[3], largs[4], largs[5], tab, counts.shape[0], counts.data_ptr(), ops._stream())


class _SlotOwner:
    """A pass's int64 [n_slots, ...] buffer with one slot per image or per case, and its bookkeeping: Evaluator's and SelectiveEvaluator's counts,
    Calibration's bins, and so on.  A subclass names itself (`_who`, `_one`, `_read`) and the public attribute that holds the buffer (`_attr`), states the
    shape of one slot (`_trailing()`) and hands `_add` the entry that launches its pass; buffer, slots, reading and resetting are here."""
    _who, _read, _one, _attr = "Evaluator", "areas()", "an Evaluator", "counts"
    n_bins = None               # the passes with a confidence map set it

    def _init_slots(self, cases, images):
        self.cases = None if cases is None else list(cases)
        self.n_slots = int(images) if self.cases is None else len(self.cases)
        if self.n_slots < 1:
            raise ValueError(f"mmsa.{self._who}: at least one slot")
        self.used = 0           # per-image mode: slots taken so far

    def _init_buffer(self, device):
        """The buffer is made by the first add, or here where a device is given."""
        setattr(self, self._attr, None)
        if device is not None:
            self._buffer(torch.device(device))

    def _trailing(self):
        """The shape of one slot of the buffer: every owner states its own."""
        raise NotImplementedError

    def _buffer(self, device):
        buf = getattr(self, self._attr)
        if buf is None:
            if _capturing(device):
                raise RuntimeError(f"mmsa.{self._who}: the {self._attr[:-1]} buffer cannot be allocated during a graph capture: construct the {self._who} "
                                   "with device=")
            buf = torch.zeros(self.n_slots, *self._trailing(), dtype=torch.int64, device=device)
            setattr(self, self._attr, buf)
        elif buf.device != device:
            raise RuntimeError(f"mmsa.{self._who}: the {self._attr} live on {buf.device}, this batch on {device}")
        return buf

    def _add(self, lead, B, case, slots, launch, *args, guard=True):
        """The add() of every owner, behind its check of `lead` (the tensor that names the device): the buffer (made under the device guard; add_fused
        makes it without; one that exists needs none), the slots of the next B images, `launch(*args, buffer, slots)` -- every entry ends in these two --
        and the slots taken once it has gone through."""
        if guard and getattr(self, self._attr) is None:
            with torch.cuda.device(lead.device):
                buf = self._buffer(lead.device)
        else:
            buf = self._buffer(lead.device)
        launch(*args, buf, self.slots_for(B, case, slots))
        self._taken(B, case, slots)
        return self

    def reset(self):
        buf = getattr(self, self._attr)
        if buf is not None:
            buf.zero_()
        self.used = 0

    def _host(self, attr=None, trailing=None):
        """The buffer (or the one `attr` names, of that trailing shape) on the host, int64 numpy [n, ...]: n = images added so far (per-image mode) / cases."""
        buf = getattr(self, attr or self._attr)
        if buf is None:
            return np.zeros((0 if self.cases is None else self.n_slots, *(trailing or self._trailing())), dtype=np.int64)
        h = buf.cpu().numpy()
        return h[:self.used] if self.cases is None else h

    def slots_for(self, B, case=None, slots=None):
        """The count slots the NEXT batch of B images gets (nothing is taken yet: add / add_fused take them once their launch has gone through).
        `slots=` names them outright (a captured call that must hit the same slots on every replay)."""
        if slots is not None:
            return [int(s) for s in slots]
        if self.cases is not None:
            if case not in self.cases:
                raise KeyError(f"mmsa.{self._who}: case {case!r} is not one of {self.cases}")
            return [self.cases.index(case)] * B
        if case is not None:
            raise KeyError(f"mmsa.{self._who}: case= needs {self._one} made with cases=[...]")
        if self.used + B > self.n_slots:
            raise RuntimeError(f"mmsa.{self._who}: {self.used} + {B} images but {self.n_slots} per-image slots (read {self._read}, reset(), or make it with images=)")
        return list(range(self.used, self.used + B))

    def _taken(self, B, case, slots):
        """A launch went through: in per-image mode its images now own their slots (a call that raised has consumed none)."""
        if slots is None and self.cases is None and case is None:
            self.used += B

    def _slot_index(self, slot):
        return self.cases.index(slot) if self.cases is not None and not isinstance(slot, int) else int(slot)

    def _pick(self, h, slot, check=None, total=None):
        """Of the host array h [n, ...]: the slot `slot` (index or case name), or with None the sum over every slot (`total(h)` where an owner sums with
        care).  `check` is called on every slot first, so that a slot at its capacity raises before a sum over slots could wrap."""
        if check is not None:
            for one in h:
                check(one)
        if slot is not None:
            return h[self._slot_index(slot)]
        return h.sum(0) if total is None else total(h)


class Evaluator(_SlotOwner):
    """Owns the count buffer of an evaluation run.  `cases` = None: one slot per IMAGE, in the order the images are added (what `pre_eval` returns per
    image), `images` slots in all; `cases` = a list of names: one slot per case, every image of an add(..., case=name) goes into that case's slot (the
    `case=[...]` breakdown of the DELIVER configs) with no extra launch.  Pass `device` to have the buffer before the first add (graph capture).
    Per-image mode holds `images` images (64 unless told otherwise): read areas() and reset() before it is full, or size it for the dataset."""

    def __init__(self, prep, cases=None, images=MAX_IMAGES, device=None):
        self.prep = prep
        self._init_slots(cases, images)
        self._init_buffer(device)

    def _trailing(self):
        return (self.prep.num_classes + 1, self.prep.num_classes + 1)

    def add(self, pred, labels, case=None, slots=None):
        """Count a batch of stored class maps (one launch)."""
        pred = _check_pred(pred)
        return self._add(pred, pred.shape[0], case, slots, confusion, pred, labels, self.prep)

    def add_fused(self, lg, plan, out, unc, labels, case=None, slots=None):
        """Class map + counts in one launch (mmsa.inference's class-map calls with labels= / evaluator=); `plan`: the frame's mmsa.inference.MapPlan."""
        return self._add(lg, plan.B, case, slots, slide_argmax_eval, lg, plan.n, plan.tab, out, plan.B, plan.H, plan.W, plan.hc, plan.wc, unc, labels,
                         self.prep, guard=False)

    def host_counts(self):
        """The counts on the host (the ONE device-to-host copy of an evaluation): int64 numpy [n, C + 1, C + 1], n = images added so far / cases."""
        return self._host()

    def areas(self):
        """(area_intersect, area_union, area_pred_label, area_label): int64 numpy [n, C] each, row per image (per case with cases=)."""
        return areas_of(self.host_counts())

    def metrics(self, metric=("mIoU",), nan_to_num=None, beta=1, slot=None):
        """`total_area_to_metrics` of the totals over every slot (the reference's 'global' entry) or of one slot (index or case name), in float64."""
        return area_metrics(*(self._pick(a, slot) for a in self.areas()), metric=metric, nan_to_num=nan_to_num, beta=beta)

    def summary(self, metric=("mIoU",), nan_to_num=None, beta=1, slot=None):
        """aAcc / mIoU / mAcc / ... as `evaluate` forms them from the per-class values: nanmean, rounded to two places of a percent."""
        return summary_of(self.metrics(metric, nan_to_num, beta, slot))


class Calibration(_SlotOwner):
    """Owns the reliability bins of a calibration run, as Evaluator owns the confusion counts: int64 [n_slots, 3, K] on the device (`.bins`; rows total,
    correct, conf_sum), `bins` = K confidence bins of width 1 / K.  `cases` = None: one slot per IMAGE in the order the images are added, `images` slots in
    all; `cases` = a list of names: one slot per case (the `case=[...]` breakdown of the DELIVER configs, where calibration drifts).  Pass `device` to
    have the buffer before the first add, and `slots=` to add(), for a call that is captured in a HIP graph.  Only host_bins() copies anything to the
    host: 3 K integers per slot; every metric is formed from them in float64, of one slot (`slot=` index or case name) or of the sum over all slots
    (`slot=None`), and raises OverflowError once a bin holds 2^39 pixels.  Across ranks: mmsa.dist.allreduce_counts(cal.bins)."""
    _who, _read, _one, _attr = "Calibration", "host_bins()", "a Calibration", "bins"

    def __init__(self, prep, bins=DEFAULT_BINS, cases=None, images=MAX_IMAGES, device=None):
        self.prep = prep
        self.n_bins = _check_bins(bins)
        self._init_slots(cases, images)
        self._init_buffer(device)

    def _trailing(self):
        return (3, self.n_bins)

    def add(self, pred, conf, labels, case=None, slots=None):
        """Bin a batch of stored class maps and their confidence maps (one launch; no host sync, no allocation once the buffer exists)."""
        _check_confmap(conf, _check_pred(pred))
        return self._add(pred, pred.shape[0], case, slots, calibration, pred, conf, labels, self.prep, self.n_bins)

    def host_bins(self):
        """The bins on the host (the ONE device-to-host copy of a calibration run): int64 numpy [n, 3, K], n = images added so far / cases."""
        return self._host()

    def _of(self, slot):
        """int64 [3, K] of one slot (index or case name), or of the sum over every slot.  A slot at its capacity raises here, before a sum over slots
        could wrap; a sum whose totals stay below 2^39 has confidence sums below 2^63."""
        return self._pick(self.host_bins(), slot, _bins3)

    def reliability(self, slot=None):
        """`reliability_of` the slot's bins: edges, count, accuracy and confidence per bin."""
        return reliability_of(self._of(slot))

    def ece(self, slot=None):
        return ece_of(self._of(slot))

    def mce(self, slot=None):
        return mce_of(self._of(slot))

    def accuracy(self, slot=None):
        """sum(correct) / sum(total): the unrounded aAcc of Evaluator.metrics on the same maps."""
        return accuracy_of(self._of(slot))

    def mean_confidence(self, slot=None):
        return mean_confidence_of(self._of(slot))

    def risk_coverage(self, slot=None):
        """(coverage [K], selective_accuracy [K]): entry k keeps the pixels of the bins k .. K - 1."""
        return risk_coverage_of(self._of(slot))

    def summary(self, slot=None):
        """ECE / MCE / aAcc / mConf in percent, rounded to two places."""
        return calibration_summary_of(self._of(slot))


class SelectiveEvaluator(_SlotOwner):
    """Owns the per-bin confusion counts of a selective evaluation run, as Evaluator owns the confusion counts and Calibration the reliability bins: int64
    [n_slots, K, C + 1, C + 1] on the device (`.counts`), `bins` = K confidence bins of width 1 / K.  `cases` / `images` / `device` and `slots=` of add():
    as for Calibration.  Only host_counts() copies anything to the host (81 KB per slot at 25 classes and 15 bins); everything else is formed from those
    integers: `min_bin=` keeps the bins min_bin .. K - 1 (the pixels `abstain` leaves in the map), and at min_bin=0 metrics / summary / areas are the
    Evaluator's.  A buffer above 1 GiB is refused.  Across ranks: mmsa.dist.allreduce_counts(se.counts)."""
    _who, _read, _one, _attr = "SelectiveEvaluator", "host_counts()", "a SelectiveEvaluator", "counts"

    def __init__(self, prep, bins=DEFAULT_BINS, cases=None, images=MAX_IMAGES, device=None):
        self.prep = prep
        self.n_bins = _check_bins(bins)
        C = _check_selective_classes(prep.num_classes)
        self._init_slots(cases, images)
        nbytes = self.n_slots * self.n_bins * (C + 1) * (C + 1) * 8
        if nbytes > MAX_SELECTIVE_BYTES:
            raise ValueError(f"mmsa.SelectiveEvaluator: {self.n_slots} slots x {self.n_bins} bins x {C + 1} x {C + 1} int64 counts are {nbytes} bytes, above "
                             f"the {MAX_SELECTIVE_BYTES} (1 GiB) a count buffer may take: fewer slots (cases= or images=) or fewer bins")
        self._init_buffer(device)

    def _trailing(self):
        return (self.n_bins, self.prep.num_classes + 1, self.prep.num_classes + 1)

    def add(self, pred, conf, labels, case=None, slots=None):
        """Count a batch of stored class maps and their confidence maps (one launch; no host sync, no allocation once the buffer exists)."""
        _check_confmap(conf, _check_pred(pred))
        return self._add(pred, pred.shape[0], case, slots, selective, pred, conf, labels, self.prep, self.n_bins)

    def host_counts(self):
        """The counts on the host (the ONE device-to-host copy of a run): int64 numpy [n, K, C + 1, C + 1], n = images added so far / cases."""
        return self._host()

    def _of(self, slot):
        """int64 [K, C + 1, C + 1] of one slot (index or case name), or of the sum over every slot."""
        return self._pick(self.host_counts(), slot, _counts3, lambda c: _sum_bins(c.reshape(c.shape[0], -1, c.shape[-1])).reshape(c.shape[1:]))

    def evaluator_counts(self):
        """The sum over the bins: Evaluator.host_counts() of the same maps, int64 [n, C + 1, C + 1]."""
        c = self.host_counts()
        return np.stack([selective_counts_of(one, 0) for one in c]) if len(c) else c.sum(1)

    def reliability_counts(self, slot=None):
        """`reliability_counts_of`: Calibration.host_bins()[:, :2] of the same maps, int64 [n, 2, K] (total, correct) -- or [2, K] of one slot."""
        c = self.host_counts()
        return reliability_counts_of(c if slot is None else c[self._slot_index(slot)])

    def areas(self, min_bin=0):
        """(area_intersect, area_union, area_pred_label, area_label) of the pixels kept at `min_bin`: int64 numpy [n, C] each, row per image / case."""
        c = self.host_counts()
        C = self.prep.num_classes
        kept = np.stack([selective_counts_of(one, min_bin) for one in c]) if len(c) else np.zeros((0, C + 1, C + 1), dtype=np.int64)
        return areas_of(kept)

    def metrics(self, min_bin=0, slot=None, metric=("mIoU",), nan_to_num=None, beta=1):
        """`total_area_to_metrics` of the pixels kept at `min_bin`, over every slot or of one slot; at min_bin=0 Evaluator.metrics of the same maps."""
        return area_metrics(*areas_of(selective_counts_of(self._of(slot), min_bin)), metric=metric, nan_to_num=nan_to_num, beta=beta)

    def summary(self, min_bin=0, slot=None, metric=("mIoU",), nan_to_num=None, beta=1, auc=False):
        """aAcc / mIoU / mAcc / ... of the pixels kept at `min_bin`, as Evaluator.summary rounds them.  `auc=True`: the entry 'AURC' is added, `auc()` of the
        risk over ALL bins (it does not depend on `min_bin`), rounded the same way; without it the summary is Evaluator.summary's, key for key."""
        s = summary_of(self.metrics(min_bin, slot, metric, nan_to_num, beta))
        if auc:
            s["AURC"] = _round_percent(self.auc("risk", slot))
        return s

    def coverage_curve(self, metric=("mIoU",), slot=None, nan_to_num=None, beta=1):
        """`selective_metrics_of`: coverage and every metric at every threshold k = 0 .. K - 1 (mIoU against coverage)."""
        return selective_metrics_of(self._of(slot), metric=metric, nan_to_num=nan_to_num, beta=beta)

    def auc(self, metric="risk", slot=None):
        """`selective_auc_of`: the area under coverage_curve()'s risk (AURC), mIoU or aAcc against coverage -- one number per score map, which is what says
        which of confidence, margin and entropy score ranks the errors best on the data counted."""
        return selective_auc_of(self._of(slot), metric)


class TemperatureSweep(_SlotOwner):
    """Owns the sweep buffer of a temperature fit, as Calibration owns the reliability bins: int64 [n_slots, J, 4, K] on the device (`.counts`; per
    temperature the rows total, correct, conf_sum, nll_sum), over the fixed grid `temperatures` (1..16; `geometric_grid`) and `bins` = K confidence bins.
    `cases` / `images` / `device` and `slots=` of add(): as for Calibration.  add() takes the LOGITS canvas of a batch (mmsa.inference.inference in any test
    mode, with or without rescale) and its raw labels: one launch, no host sync.  Only host() copies anything to the host: 4 J K integers per slot; every
    metric is formed from them in float64, of one slot (`slot=` index or case name) or of the sum over all slots.  Across ranks:
    mmsa.dist.allreduce_counts(sw.counts).  The fit is best(); refining it is a second TemperatureSweep over a narrower grid around it."""
    _who, _read, _one, _attr = "TemperatureSweep", "host()", "a TemperatureSweep", "counts"

    def __init__(self, prep, temperatures, bins=DEFAULT_BINS, cases=None, images=MAX_IMAGES, device=None):
        self.prep = prep
        self.inv_temperatures = _inv_temperatures(temperatures)
        self.temperatures = np.array([float(t) for t in (temperatures if np.ndim(temperatures) else [temperatures])], dtype=np.float64)
        self.n_bins = _check_bins(bins)
        self._init_slots(cases, images)
        self._init_buffer(device)

    def _trailing(self):
        return (len(self.inv_temperatures), 4, self.n_bins)

    def add(self, logits, labels, case=None, slots=None):
        """Sweep a batch's logits canvas [B, C, H, W] against its labels (one launch; no host sync, no allocation once the buffer exists)."""
        logits = _check_logits(logits)
        return self._add(logits, logits.shape[0], case, slots, temperature_sweep, logits, labels, self.prep, self.temperatures, self.n_bins)

    def host(self):
        """The sweeps on the host (the ONE device-to-host copy of a fit): int64 numpy [n, J, 4, K], n = images added so far / cases."""
        return self._host()

    def _of(self, slot):
        """int64 [J, 4, K] of one slot (index or case name), or of the sum over every slot."""
        return self._pick(self.host(), slot, _sweep4)

    def bins(self, j, slot=None):
        """Calibration's int64 [3, K] bins at temperature j: what reliability_of / ece_of / mce_of / risk_coverage_of take."""
        return sweep_bins_of(self._of(slot), j)

    def nll(self, slot=None):
        """The mean NLL of the label's class per temperature, float64 [J]."""
        return sweep_nll_of(self._of(slot))

    def ece(self, slot=None):
        """The expected calibration error per temperature, float64 [J]."""
        return sweep_ece_of(self._of(slot))

    def best(self, by="nll", slot=None):
        """(T, j): the grid's temperature with the smallest mean NLL (`by`="nll") or ECE ("ece"); the first minimum wins."""
        return sweep_best_of(self._of(slot), self.temperatures, by)

    def summary(self, slot=None):
        """Per temperature: T, the mean NLL rounded to four places, ECE and aAcc in percent rounded to two; and the best T by either measure."""
        s = self._of(slot)
        out = OrderedDict(T=self.temperatures.copy(), NLL=np.round(sweep_nll_of(s), 4), ECE=np.round(sweep_ece_of(s) * 100, 2),
                          aAcc=np.round(accuracy_of(s[0, :3]) * 100, 2))
        for by in ("nll", "ece"):
            try:
                out["best_" + by] = sweep_best_of(s, self.temperatures, by)[0]
            except ValueError:
                out["best_" + by] = np.float64(np.nan)
        return out


# ---- top-k evaluation: at which rank of a top-k class map the label's class stands (csrc/topk_eval.hip) ----
MAX_TOPK = 8            # ranks of a top-k map (csrc/softmax_px.h TOPK_MAX: the rank list of a pixel lives in registers)


def check_topk(k, who="mmsa.evaluate"):
    """`k`, the number of ranks of a top-k map: an int in 1..MAX_TOPK."""
    if not _is_int(k, 1, MAX_TOPK):
        raise ValueError(f"{who}: topk = {k!r}; 1..{MAX_TOPK} ranks are supported")
    return int(k)


def _check_rank_planes(classes):
    """The class planes of a top-k map: a contiguous uint8 [K, B, H, W] GPU tensor, rank-major (`TopK.classes`)."""
    if not isinstance(classes, torch.Tensor) or not classes.is_cuda:
        raise RuntimeError("mmsa.evaluate: classes must be a GPU tensor (there is no CPU path)")
    if classes.dtype != torch.uint8:
        raise RuntimeError(f"mmsa.evaluate: classes are {classes.dtype}; uint8 class planes are expected")
    if classes.dim() != 4 or not classes.is_contiguous():
        raise RuntimeError(f"mmsa.evaluate: classes must be a contiguous [K, B, H, W] tensor (rank-major), got {tuple(classes.shape)}")
    if not 1 <= classes.shape[0] <= MAX_TOPK:
        raise RuntimeError(f"mmsa.evaluate: {classes.shape[0]} rank planes; 1..{MAX_TOPK} are supported")
    return classes


@torch.no_grad()
def topk_counts(classes, labels, prep, counts=None, slots=None):
    """ADD the rank counts of the uint8 class planes classes [K, B, H, W] of a top-k map against the raw labels [B, Hl, Wl] into counts[slots[b]] (one
    launch, mmsa_eval_topk_u8) -> counts, int64 [n_slots, C, K + 1] on the device: a pixel takes part iff its transformed label l is a class (< C), and adds
    1 at [slot, l, r], r = the first rank whose class equals l, K where none does.  Column r is the diagonal of `confusion(classes[r], ...)`, row l sums to
    row l of plane 0's matrix.  `slots` defaults to 0 .. B - 1 (per-image counts); `counts` defaults to a zeroed buffer of max(slots) + 1 slots."""
    classes = _check_rank_planes(classes)
    K, B, H, W = (int(v) for v in classes.shape)
    C = prep.num_classes
    with torch.cuda.device(classes.device):
        largs, counts, tab = _slot_launch(prep, labels, B, H, W, classes.device, counts, "counts", (C, K + 1), slots)
        lib.call("mmsa_eval_topk_u8", classes.data_ptr(), K, largs[0], B, H, W, largs[1], largs[2], largs[3], C, largs[4], largs[5], tab, counts.shape[0],
                 counts.data_ptr(), ops._stream())
    return counts


def topk_accuracy_of(counts):
    """int64 [..., C, K + 1] rank counts -> the top-1 .. top-K pixel accuracies, float64 [..., K]: the cumulative column sums over the participating
    pixels.  0 / 0 is NaN."""
    c = np.asarray(counts, dtype=np.int64)
    hit = np.cumsum(c.sum(-2)[..., :-1], axis=-1).astype(np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        return hit / np.float64(c.sum((-2, -1)))[..., None]


def topk_recall_of(counts):
    """int64 [..., C, K + 1] rank counts -> the per-class recall@1 .. recall@K, float64 [..., C, K]; NaN for a class without pixels."""
    c = np.asarray(counts, dtype=np.int64)
    hit = np.cumsum(c[..., :-1], axis=-1).astype(np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        return hit / c.sum(-1).astype(np.float64)[..., None]


class TopKEvaluator(_SlotOwner):
    """Owns the rank counts of a top-k evaluation run, as Evaluator owns the confusion counts: int64 [n_slots, C, k + 1] on the device (`.counts`).
    `cases` / `images` / `device` as in Evaluator.  accuracy()[0] is Evaluator's aAcc of plane 0; mmsa.dist.allreduce_counts(te.counts) is the one collective of
    a multi-GPU run."""
    _who, _read, _one, _attr = "TopKEvaluator", "accuracy()", "a TopKEvaluator", "counts"

    def __init__(self, prep, k, cases=None, images=MAX_IMAGES, device=None):
        self.prep = prep
        self.k = check_topk(k, "mmsa.TopKEvaluator")
        self._init_slots(cases, images)
        self._init_buffer(device)

    def _trailing(self):
        return (self.prep.num_classes, self.k + 1)

    def add(self, classes, labels, case=None, slots=None):
        """Count the class planes [k, B, H, W] of a batch of top-k maps (one launch)."""
        classes = _check_rank_planes(classes)
        if classes.shape[0] != self.k:
            raise RuntimeError(f"mmsa.TopKEvaluator: {classes.shape[0]} rank planes, this evaluator counts {self.k}")
        return self._add(classes, int(classes.shape[1]), case, slots, topk_counts, classes, labels, self.prep)

    def host_counts(self):
        """The counts on the host (the ONE device-to-host copy): int64 numpy [n, C, k + 1], n = images added so far / cases."""
        return self._host()

    def _of(self, slot):
        return self._pick(self.host_counts(), slot)

    def accuracy(self, slot=None):
        """The top-j pixel accuracy for j = 1 .. k, float64 [k], over every slot or of one slot (index or case name)."""
        return topk_accuracy_of(self._of(slot))

    def recall(self, slot=None):
        """The per-class recall@j, float64 [C, k]; NaN for a class without pixels."""
        return topk_recall_of(self._of(slot))

    def summary(self, slot=None):
        """OrderedDict top1 .. topk (pixel accuracy) and mRecall1 .. mRecallk (nanmean over the classes), rounded as `Evaluator.summary` rounds."""
        acc, rec = self.accuracy(slot), self.recall(slot)
        out = OrderedDict()
        with warnings.catch_warnings():
            warnings.simplefilter("ignore", RuntimeWarning)
            for j in range(self.k):
                out[f"top{j + 1}"] = _round_percent(acc[j])
            for j in range(self.k):
                out[f"mRecall{j + 1}"] = _round_percent(np.nanmean(rec[:, j]))
        return out


# ---- boundary evaluation: the confusion counts split by nearness to a label boundary and to a prediction boundary (csrc/boundary.hip) ----
MAX_BOUNDARY_RADIUS = 32      # csrc/boundary.hip BOUNDARY_MAX_RADIUS: the usual trimap widths, and 0.5 % - 2 % of the diagonal up to 1024 x 1024
MAX_BOUNDARY_CLASSES = 82     # csrc/boundary.hip BOUNDARY_MAX_CLASSES: one zone's (C + 1)^2 uint32 histogram next to the tiles of radius 32 in 64 KiB of LDS
_BOUNDARY_TILE_W = 64
_BOUNDARY_LDS = 65536


def check_boundary_radius(radius, who="mmsa.evaluate"):
    if not _is_int(radius, 1, MAX_BOUNDARY_RADIUS):
        raise ValueError(f"{who}: radius = {radius!r}; 1..{MAX_BOUNDARY_RADIUS} pixels (Chebyshev) are supported")
    return int(radius)


def _check_boundary_classes(C, who="mmsa.evaluate"):
    if C > MAX_BOUNDARY_CLASSES:
        raise RuntimeError(f"{who}: {C} classes; boundary evaluation supports 2..{MAX_BOUNDARY_CLASSES} (one zone's (C + 1)^2 uint32 histogram must fit a "
                           f"workgroup's 64 KiB of LDS next to the tiles of radius {MAX_BOUNDARY_RADIUS})")
    return C


def boundary_launch_shape(num_classes, radius):
    """The launch mmsa_eval_boundary_u8 makes for `num_classes` and `radius`, by the arithmetic of csrc/boundary.hip -> (zone groups, LDS bytes of a
    workgroup, tile rows, tile columns): the tile is 64 columns x 64 rows up to radius 16 and 32 rows above, staged with a halo of `radius` for both maps
    (row pitch 17 + radius // 2 dwords) next to 16 dwords per staged row of row-pass bytes, the 256-byte LUT and 4 / groups zone histograms; the groups
    are the fewest of 1, 2, 4 that stay inside 64 KiB."""
    C, r = _check_boundary_classes(int(num_classes)), check_boundary_radius(radius)
    th = 64 if r <= 16 else 32
    tiles = 2 * (th + 2 * r) * (_BOUNDARY_TILE_W // 4 + r // 2 + 1 + _BOUNDARY_TILE_W // 4) * 4
    for groups in (1, 2, 4):
        lds = (4 // groups) * (C + 1) * (C + 1) * 4 + tiles + 256
        if lds <= _BOUNDARY_LDS:
            break
    return groups, lds, th, _BOUNDARY_TILE_W


@torch.no_grad()
def boundary_counts(pred, labels, prep, radius, border=False, counts=None, slots=None):
    """ADD the boundary counts of the uint8 class maps pred [B, H, W] against the raw labels [B, Hl, Wl] into counts[slots[b]] (one launch,
    mmsa_eval_boundary_u8) -> counts, int64 [n_slots, 4, C + 1, C + 1] on the device.  With L the transformed label code (a class, C = kept but out of range,
    255 = ignored) and P = min(pred, C): a pixel is near a label boundary iff some pixel of the image within Chebyshev distance `radius` has another L (an
    ignored label counts as a neighbour), near a prediction boundary likewise for P; `border=True` also puts every pixel closer than `radius` to the image
    border near both (the zero-padded erosion).  Every pixel whose own label is not ignored adds 1 at [slot, 2 * near_label + near_pred, min(L, C), P]:
    counts.sum(1) is `confusion(pred, labels, prep)`, bit for bit.  `slots` defaults to 0 .. B - 1; `counts` to a zeroed buffer of max(slots) + 1 slots."""
    pred = _check_pred(pred)
    radius = check_boundary_radius(radius)
    B, H, W = (int(v) for v in pred.shape)
    C = _check_boundary_classes(prep.num_classes)
    with torch.cuda.device(pred.device):
        largs, counts, tab = _slot_launch(prep, labels, B, H, W, pred.device, counts, "counts", (4, C + 1, C + 1), slots)
        lib.call("mmsa_eval_boundary_u8", pred.data_ptr(), largs[0], B, H, W, largs[1], largs[2], largs[3], C, largs[4], largs[5], tab, counts.shape[0],
                 radius, 1 if border else 0, counts.data_ptr(), ops._stream())
    return counts


def _zones(counts):
    c = np.asarray(counts)
    if c.ndim < 3 or c.shape[-3] != 4 or c.shape[-1] != c.shape[-2] or c.shape[-1] < 3 or c.dtype.kind not in "iu":
        raise ValueError(f"mmsa.evaluate: boundary counts are an integer [..., 4, C + 1, C + 1] array, got {c.dtype} {c.shape}")
    return c.astype(np.int64, copy=False)


def boundary_zone_sum_of(counts):
    """int64 [..., 4, C + 1, C + 1] boundary counts -> their sum over the zones, int64 [..., C + 1, C + 1]: the confusion counts of the whole map."""
    return _zones(counts).sum(-3)


def trimap_counts_of(counts, interior=False):
    """int64 [..., 4, C + 1, C + 1] boundary counts -> the confusion counts of the band around the label boundaries (zones 2 + 3), int64 [..., C + 1, C + 1]:
    what `areas_of` / `area_metrics` turn into the trimap aAcc / IoU / Acc.  `interior=True`: zones 0 + 1, the rest of the map."""
    c = _zones(counts)
    return c[..., 0, :, :] + c[..., 1, :, :] if interior else c[..., 2, :, :] + c[..., 3, :, :]


def boundary_iou_of(counts):
    """int64 [..., 4, C + 1, C + 1] boundary counts -> the Boundary IoU per class (Cheng et al., CVPR 2021), float64 [..., C]: with G_c the pixels of label c
    near a label boundary (row c of zones 2 + 3), Pd_c the pixels predicted c near a prediction boundary (column c of zones 1 + 3; pixels with an ignored
    label are in no count, as `intersect_and_union` masks them) and I_c = counts[3][c][c], BIoU_c = I_c / (G_c + Pd_c - I_c); 0 / 0 is NaN."""
    c = _zones(counts)
    C = c.shape[-1] - 1
    G = (c[..., 2, :, :] + c[..., 3, :, :]).sum(-1)[..., :C]
    Pd = (c[..., 1, :, :] + c[..., 3, :, :]).sum(-2)[..., :C]
    I = np.diagonal(c[..., 3, :, :], axis1=-2, axis2=-1)[..., :C]
    with np.errstate(divide="ignore", invalid="ignore"):
        return I.astype(np.float64) / (G + Pd - I).astype(np.float64)


class BoundaryEvaluator(_SlotOwner):
    """Owns the boundary counts of an evaluation run, as Evaluator owns the confusion counts: int64 [n_slots, 4, C + 1, C + 1] on the device (`.counts`), zone
    2 * near_label + near_pred at Chebyshev `radius` (`boundary_counts`).  `cases` / `images` / `device` and `slots=` of add(): as for Evaluator.  Only
    host_counts() copies anything to the host; the trimap metrics and the Boundary IoU are formed from those integers in float64.  Across ranks:
    mmsa.dist.allreduce_counts(be.counts)."""
    _who, _read, _one, _attr = "BoundaryEvaluator", "host_counts()", "a BoundaryEvaluator", "counts"

    def __init__(self, prep, radius, border=False, cases=None, images=MAX_IMAGES, device=None):
        self.prep = prep
        self.radius = check_boundary_radius(radius, "mmsa.BoundaryEvaluator")
        self.border = bool(border)
        _check_boundary_classes(prep.num_classes, "mmsa.BoundaryEvaluator")
        self._init_slots(cases, images)
        self._init_buffer(device)

    def _trailing(self):
        return (4, self.prep.num_classes + 1, self.prep.num_classes + 1)

    def add(self, pred, labels, case=None, slots=None):
        """Count a batch of stored class maps (one launch; no host sync, no allocation once the buffer exists)."""
        pred = _check_pred(pred)
        return self._add(pred, int(pred.shape[0]), case, slots, boundary_counts, pred, labels, self.prep, self.radius, self.border)

    def host_counts(self):
        """The counts on the host (the ONE device-to-host copy): int64 numpy [n, 4, C + 1, C + 1], n = images added so far / cases."""
        return self._host()

    def _of(self, slot):
        return self._pick(self.host_counts(), slot)

    def evaluator_counts(self):
        """The sum over the zones: Evaluator.host_counts() of the same maps, int64 [n, C + 1, C + 1]."""
        return boundary_zone_sum_of(self.host_counts())

    def trimap_metrics(self, slot=None, metric=("mIoU",), nan_to_num=None, beta=1):
        """`area_metrics` of the band around the label boundaries (zones 2 + 3), over every slot or of one slot (index or case name)."""
        return area_metrics(*areas_of(trimap_counts_of(self._of(slot))), metric=metric, nan_to_num=nan_to_num, beta=beta)

    def interior_metrics(self, slot=None, metric=("mIoU",), nan_to_num=None, beta=1):
        """`area_metrics` of the pixels away from the label boundaries (zones 0 + 1)."""
        return area_metrics(*areas_of(trimap_counts_of(self._of(slot), interior=True)), metric=metric, nan_to_num=nan_to_num, beta=beta)

    def boundary_iou(self, slot=None):
        """`boundary_iou_of`: the Boundary IoU per class, float64 [C]; NaN for a class with no pixel in either band."""
        return boundary_iou_of(self._of(slot))

    def summary(self, slot=None):
        """OrderedDict aAcc, mIoU (the whole map: Evaluator's numbers), trimap_aAcc, trimap_mIoU, mBIoU (nanmean over the classes) and band (the share of the
        counted pixels in zones 2 + 3), rounded as `Evaluator.summary` rounds."""
        c = self._of(slot)
        band = trimap_counts_of(c)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore", RuntimeWarning)
            whole = summary_of(area_metrics(*areas_of(boundary_zone_sum_of(c))))
            tri = summary_of(area_metrics(*areas_of(band)))
            with np.errstate(divide="ignore", invalid="ignore"):
                share = np.float64(band.sum()) / np.float64(c.sum())
            return OrderedDict(aAcc=whole["aAcc"], mIoU=whole["mIoU"], trimap_aAcc=tri["aAcc"], trimap_mIoU=tri["mIoU"],
                               mBIoU=_round_percent(np.nanmean(self.boundary_iou(slot))), band=_round_percent(share))


# ---- Euclidean boundary evaluation: exact squared distance maps of the code maps, and what is counted from two of them (csrc/distance.hip) ----
# For a code map M (the label codes L or the prediction codes P of the boundary pass above) D2(p) = the smallest (qy - py)^2 + (qx - px)^2 over the pixels q OF
# THE IMAGE with M(q) != M(p): an integer >= 1, kept where it is <= cap^2 and FAR elsewhere; `border=True` also bounds it by db^2, db = min(y, x, H - 1 - y,
# W - 1 - x) + 1 (the first pixel outside the image).  "Near at Euclidean radius rho" is D2 <= floor(rho^2); the adjacent pixel is at distance 1, and two
# coincident contours give D2 in {1, 2}: TOLERANCES COUNT FROM 1.  With the Chebyshev band `near(., d)` of the boundary pass: D2 <= 2 <=> near(., 1);
# near(., d) => D2 <= 2 d^2; D2 <= d^2 => near(., d).
MAX_DISTANCE_CAP = 255             # csrc/distance.hip DIST_MAX_CAP: cap^2 = 65025 is the largest value a uint16 map holds below FAR
DISTANCE_FAR = 65535               # csrc/distance.hip DIST_FAR: "further than cap", and "no other code in the image"
MAX_EUCLIDEAN_CLASSES = 126        # csrc/distance.hip DIST_MAX_CLASSES: one zone's (C + 1)^2 uint32 histogram in a workgroup's 64 KiB of LDS
MAX_DISPLACEMENT_CELLS = 16320     # csrc/distance.hip DIST_MAX_SIDE_CELLS: (C + 1) * (cap + 2) uint32 cells of one side of the displacement histogram in LDS
_CODE_LUTS = {}                    # (codes, device) -> the device LUT of a distance launch
_DISTANCE_SCRATCH = {}             # (device, stream) -> the uint16 row-run plane of boundary_distance calls without scratch=


def check_distance_cap(cap, who="mmsa.evaluate"):
    if not _is_int(cap, 1, MAX_DISTANCE_CAP):
        raise ValueError(f"{who}: cap = {cap!r}; 1..{MAX_DISTANCE_CAP} pixels are supported (cap^2 must fit the uint16 distance map)")
    return int(cap)


def euclidean_threshold(radius=None, radius2=None, who="mmsa.evaluate"):
    """`radius` (an int or float in [1, 255]) or `radius2` (an int in 1..65025), one of them -> (t, smallest cap): t = floor(radius^2) formed exactly (the float's
    own value, squared as a fraction), or radius2 itself; the smallest cap is ceil(radius), for radius2 the smallest integer k with k^2 >= radius2."""
    if (radius is None) == (radius2 is None):
        raise ValueError(f"{who}: radius= or radius2=, one of them")
    if radius2 is not None:
        if not _is_int(radius2, 1, MAX_DISTANCE_CAP ** 2):
            raise ValueError(f"{who}: radius2 = {radius2!r}; an integer squared radius in 1..{MAX_DISTANCE_CAP ** 2} is expected")
        t = int(radius2)
        return t, math.isqrt(t - 1) + 1
    if isinstance(radius, bool) or not isinstance(radius, (int, float, np.integer, np.floating)) or not 1 <= float(radius) <= MAX_DISTANCE_CAP:
        raise ValueError(f"{who}: radius = {radius!r}; 1..{MAX_DISTANCE_CAP} pixels (Euclidean; an int or a float) are supported")
    r = Fraction(int(radius)) if isinstance(radius, (int, np.integer)) else Fraction(float(radius))
    return math.floor(r * r), math.ceil(r)


def _check_displacement_size(C, cap, who="mmsa.evaluate"):
    if (C + 1) * (cap + 2) > MAX_DISPLACEMENT_CELLS:
        raise RuntimeError(f"{who}: {C} classes at cap {cap}: (C + 1) * (cap + 2) = {(C + 1) * (cap + 2)} cells per side of the displacement histogram; at most "
                           f"{MAX_DISPLACEMENT_CELLS} are supported (one side's uint32 histogram must fit a workgroup's 64 KiB of LDS): 62 classes at cap 255, "
                           "246 at cap 64")


def _check_euclidean_classes(C, who="mmsa.evaluate"):
    if C > MAX_EUCLIDEAN_CLASSES:
        raise RuntimeError(f"{who}: {C} classes; Euclidean boundary evaluation supports 2..{MAX_EUCLIDEAN_CLASSES} (one zone's (C + 1)^2 uint32 histogram must "
                           "fit a workgroup's 64 KiB of LDS)")
    return C


def _check_map(t, name, dtype, what, like=None, shape_only=False):
    """A stored map of a Euclidean pass: a contiguous [B, H, W] GPU tensor of `dtype`; with `like`, of that tensor's shape and device.  Type, dtype and shape
    are looked at before the device (`shape_only`: and the device not at all), so that they are refused without one."""
    if not isinstance(t, torch.Tensor):
        raise RuntimeError(f"mmsa.evaluate: {name} must be a tensor, got {type(t).__name__}")
    if t.dtype != dtype:
        raise RuntimeError(f"mmsa.evaluate: {name} is {t.dtype}; {what} is expected")
    if t.dim() != 3 or not t.is_contiguous():
        raise RuntimeError(f"mmsa.evaluate: {name} must be a contiguous [B, H, W] tensor, got {tuple(t.shape)}")
    if like is not None and tuple(t.shape) != tuple(like.shape):
        raise RuntimeError(f"mmsa.evaluate: {name} has shape {tuple(t.shape)}, the map is [B, H, W] = {tuple(like.shape)}")
    if shape_only:
        return t
    if not t.is_cuda:
        raise RuntimeError(f"mmsa.evaluate: {name} must be a GPU tensor (there is no CPU path)")
    if like is not None and t.device != like.device:
        raise RuntimeError(f"mmsa.evaluate: {name} is on {t.device}, the map on {like.device}")
    return t


def code_lut(num_classes=None, prep=None):
    """The 256-byte LUT a distance launch compares codes through, uint8 numpy [256]: v -> min(v, C) for a stored class map (`num_classes`), or the label LUT
    of `prep` with every value in [C, 254] mapped to C (255 stays: an ignored label is a code like any other)."""
    if prep is not None:
        lut = np.asarray(prep.lut, dtype=np.uint8)
        return np.where(lut == IGNORE, IGNORE, np.minimum(lut, prep.num_classes)).astype(np.uint8)
    C = int(num_classes)
    if not 1 <= C <= 254:
        raise ValueError(f"mmsa.evaluate: num_classes {num_classes}; a uint8 class map has 1..254 classes")
    return np.minimum(np.arange(256), C).astype(np.uint8)


def _table_on(cache, table, device, what):
    """The 256-byte numpy `table` of a launch on `device`: uploaded once per (bytes, device) and kept in `cache`; an upload during a graph capture is refused."""
    key = (table.tobytes(), torch.device(device))
    t = cache.get(key)
    if t is None:
        if _capturing(key[1]):
            raise RuntimeError(f"mmsa.evaluate: {what} is not on the device yet and cannot be uploaded during a graph capture: run one call before capturing")
        t = cache[key] = torch.from_numpy(table).to(key[1])
    return t


def _cached_planes(cache, n, count, device, what, dtype=torch.int32, instead="the buffers"):
    """`count` buffers of `dtype` with at least n elements each, kept in `cache` per device and stream; a new allocation during a graph capture is refused
    (`instead`: what the caller can pass to need none)."""
    key = (torch.device(device), ops._stream())
    t = cache.get(key)
    if t is None or t[0].numel() < n:
        if _capturing(key[0]):
            raise RuntimeError(f"mmsa.evaluate: {what} cannot be allocated during a graph capture: pass {instead}, or run one call of this size before "
                               "capturing")
        t = cache[key] = [torch.empty(n, dtype=dtype, device=key[0]) for _ in range(count)]
    return t


def _row_plane(n, device):
    """The uint16 plane of the row pass of a distance or a fill launch without scratch=: one buffer for both."""
    return _cached_planes(_DISTANCE_SCRATCH, n, 1, device, "the scratch plane of the distance launch", torch.uint16, "scratch=")[0]


def _code_keywords(who, num_classes, labels_prep, maps="a stored class map"):
    """num_classes= or labels_prep=, one of them: how an entry named by `who` reads its code map."""
    if (labels_prep is None) == (num_classes is None):
        raise ValueError(f"{who} takes num_classes= ({maps}) or labels_prep= (raw labels), one of them")


def _code_map_grid(map, labels_prep, size=None, num_classes=None, index32=None):
    """`map` = the uint8 tensor a code map is read from, [B, Hs, Ws] -> (map, (B, Hs, Ws, H, W)): a stored class map is its own grid, raw labels are read on the
    grid `labels_prep` resizes them to (`size=` may spell that grid out, nothing else).  Type, dtype, shape and sizes only, so that a bad call is refused without
    a device; the caller looks at the device next.  `num_classes`: a class count to check here too; `index32`: the name of an entry that indexes in 32 bits."""
    src = _check_map(map, "map", torch.uint8, "a uint8 class map or raw uint8 labels", shape_only=True)
    B, Hs, Ws = (int(v) for v in src.shape)
    if labels_prep is None:
        if size is not None and tuple(size) != (Hs, Ws):
            raise RuntimeError(f"mmsa.evaluate: size={tuple(size)} for a stored {Hs} x {Ws} class map: only labels are resized (labels_prep=)")
        H, W = Hs, Ws
        if num_classes is not None:
            code_lut(num_classes)
    else:
        H, W = labels_prep.resized(Hs, Ws) if size is None else (int(size[0]), int(size[1]))
        if labels_prep.resized(Hs, Ws) != (H, W):
            raise RuntimeError(f"mmsa.evaluate: size mismatch: the label maps are {Hs} x {Ws}, which the LabelPrep reads on a grid of "
                               f"{labels_prep.resized(Hs, Ws)[0]} x {labels_prep.resized(Hs, Ws)[1]}, not {H} x {W}")
    if B * H * W == 0:
        raise RuntimeError(f"mmsa.evaluate: an empty map {tuple(src.shape)}")
    if index32 is not None and B * H * W >= 1 << 31:
        raise RuntimeError(f"mmsa.evaluate: {B} x {H} x {W} pixels; {index32} indexes a batch in 32 bits (B * H * W < 2^31)")
    return src, (B, Hs, Ws, H, W)


def _code_map_args(src, grid, num_classes, labels_prep):
    """The leading arguments of a launch that reads a code map (src, B, Hs, Ws, lut, ymap, xmap, H, W), in the caller's device guard: the LUT and the
    nearest-neighbour tables are cached on the device, and a first upload during a graph capture is refused."""
    B, Hs, Ws, H, W = grid
    lut = _table_on(_CODE_LUTS, code_lut(num_classes, labels_prep), src.device, "the code LUT of the distance launch")
    ymap, xmap = (None, None) if labels_prep is None else labels_prep.tables(Hs, Ws, H, W, src.device)
    return (src.data_ptr(), B, Hs, Ws, lut.data_ptr(), None if ymap is None else ymap.data_ptr(), None if xmap is None else xmap.data_ptr(), H, W)


@torch.no_grad()
def boundary_distance(map, cap, border=False, *, labels_prep=None, num_classes=None, size=None, scratch=None, out=None):
    """The squared Euclidean distance of every pixel to the nearest pixel of its image with another code (two launches, mmsa_boundary_distance_u8) -> uint16
    [B, H, W] on the device: D2 where D2 <= cap^2, DISTANCE_FAR (65535) elsewhere -- further than `cap`, or an image of one code.  The adjacent pixel is at
    D2 = 1: distances count from 1.  `border=True` also bounds D2 by the squared distance to the first pixel outside the image.  Two uses, one of the keywords:
      num_classes=C     `map` is a stored uint8 class map [B, H, W]; the codes are P = min(map, C), as every boundary pass reads a prediction;
      labels_prep=prep  `map` holds raw uint8 labels [B, Hl, Wl]; the codes are the label codes L of `prep` (a class, C = kept but out of range, 255 = ignored: a
                        code like any other) on the grid `size=(H, W)` -- by default the size `prep` resizes an Hl x Wl label map to -- through the
                        nearest-neighbour tables of the label side.
    `out=` (uint16 [B, H, W]) and `scratch=` (a uint16 tensor of at least B * H * W elements, the row pass's plane) make the call allocation-free; without
    scratch= a buffer cached per device and stream is used, which a repeated call does not allocate again."""
    cap = check_distance_cap(cap)
    _code_keywords("mmsa.evaluate: boundary_distance", num_classes, labels_prep)
    src, grid = _code_map_grid(map, labels_prep, size)
    B, H, W = grid[0], grid[3], grid[4]
    _check_map(src, "map", torch.uint8, "a uint8 class map or raw uint8 labels")
    with torch.cuda.device(src.device):
        out = torch.empty(B, H, W, dtype=torch.uint16, device=src.device) if out is None else _check_out(out, torch.uint16, (B, H, W), src.device)
        scratch = _row_plane(B * H * W, src.device) if scratch is None else _check_scratch(scratch, torch.uint16, B * H * W, src.device, avoid=out)
        lib.call("mmsa_boundary_distance_u8", *_code_map_args(src, grid, num_classes, labels_prep), cap, 1 if border else 0, scratch.data_ptr(),
                 out.data_ptr(), ops._stream())
    return out


def _d2_launch(entry, pred, labels, prep, d2_pred, d2_label, scalar, buf, name, shape, slots):
    """One launch of a pointwise pass over (pred, labels, d2_pred, d2_label) into the int64 buffer `buf` [n_slots, *shape] -> the buffer."""
    for only in (True, False):      # dtypes and shapes of all three first, then the devices
        pred = _check_map(pred, "pred", torch.uint8, "a uint8 class map", shape_only=only)
        d2_pred = _check_map(d2_pred, "d2_pred", torch.uint16, "a uint16 distance map (mmsa.boundary_distance)", like=pred, shape_only=only)
        d2_label = _check_map(d2_label, "d2_label", torch.uint16, "a uint16 distance map (mmsa.boundary_distance)", like=pred, shape_only=only)
    B, H, W = (int(v) for v in pred.shape)
    C = prep.num_classes
    with torch.cuda.device(pred.device):
        largs, buf, tab = _slot_launch(prep, labels, B, H, W, pred.device, buf, name, shape, slots)
        lib.call(entry, pred.data_ptr(), largs[0], B, H, W, largs[1], largs[2], largs[3], C, largs[4], largs[5], tab, buf.shape[0], d2_pred.data_ptr(),
                 d2_label.data_ptr(), scalar, buf.data_ptr(), ops._stream())
    return buf


@torch.no_grad()
def boundary_counts_d2(pred, labels, prep, d2_pred, d2_label, t, counts=None, slots=None):
    """ADD the boundary counts at a Euclidean radius into counts[slots[b]] (one launch, mmsa_eval_boundary_d2) -> counts, int64 [n_slots, 4, C + 1, C + 1] on the
    device, `boundary_counts`' layout and meaning with near_label = (d2_label <= t), near_pred = (d2_pred <= t): every pixel whose own label is not ignored adds
    1 at [slot, 2 * near_label + near_pred, min(L, C), P].  d2_pred = boundary_distance(pred, cap, border, num_classes=C) and d2_label =
    boundary_distance(labels, cap, border, labels_prep=prep); t = floor(radius^2), an integer in 1..cap^2 (t = 2 is `boundary_counts` at radius 1, bit for
    bit; several radii are several of these launches over one pair of maps).  counts.sum(1) is `confusion(pred, labels, prep)`."""
    if not _is_int(t, 1, MAX_DISTANCE_CAP ** 2):
        raise ValueError(f"mmsa.evaluate: t = {t!r}; an integer squared radius in 1..{MAX_DISTANCE_CAP ** 2} is expected (floor(radius^2), at most cap^2 of the maps)")
    C = _check_euclidean_classes(prep.num_classes)
    return _d2_launch("mmsa_eval_boundary_d2", pred, labels, prep, d2_pred, d2_label, int(t), counts, "counts", (4, C + 1, C + 1), slots)


@torch.no_grad()
def boundary_displacement(pred, labels, prep, d2_pred, d2_label, cap, hist=None, slots=None):
    """ADD the displacement histogram of the two contours into hist[slots[b]] (one launch, mmsa_eval_boundary_displacement) -> hist, int64
    [n_slots, 2, C + 1, cap + 2] on the device.  For every pixel whose own label is not ignored: a label-boundary pixel (d2_label <= 2: another label code
    among its 8 neighbours) adds 1 at [slot, 0, min(L, C), k(d2_pred)], a prediction-boundary pixel (d2_pred <= 2) adds 1 at [slot, 1, P, k(d2_label)];
    k(d2) = the smallest integer k >= 1 with k^2 >= d2 -- the distance rounded UP to whole pixels, counted from 1: coincident contours land in bins 1 and 2
    (D2 = 1 or 2), bin 0 stays 0 -- and cap + 1 for DISTANCE_FAR.  `cap` is the cap the two maps were made with."""
    cap = check_distance_cap(cap)
    C = prep.num_classes
    _check_displacement_size(C, cap)
    return _d2_launch("mmsa_eval_boundary_displacement", pred, labels, prep, d2_pred, d2_label, cap, hist, "hist", (2, C + 1, cap + 2), slots)


def _displacement(hist):
    h = np.asarray(hist)
    if h.ndim < 3 or h.shape[-3] != 2 or h.shape[-2] < 2 or h.shape[-1] < 3 or h.dtype.kind not in "iu":
        raise ValueError(f"mmsa.evaluate: a displacement histogram is an integer [..., 2, C + 1, cap + 2] array, got {h.dtype} {h.shape}")
    return h.astype(np.int64, copy=False)


def _f_of(matched, total):
    """matched / total int64 [..., 2, rows]: side 0 (label-boundary pixels: recall), side 1 (prediction-boundary pixels: precision) -> precision, recall, F."""
    with np.errstate(divide="ignore", invalid="ignore"):
        prec = matched[..., 1, :].astype(np.float64) / total[..., 1, :].astype(np.float64)
        rec = matched[..., 0, :].astype(np.float64) / total[..., 0, :].astype(np.float64)
        return prec, rec, 2 * prec * rec / (prec + rec)


def boundary_f_curve_of(hist):
    """The boundary F-score (Csurka et al.; the DAVIS F measure; the "BF score") at EVERY tolerance 1 .. cap from int64 [..., 2, C + 1, cap + 2] displacement
    counts -> OrderedDict: 'tolerance' int64 [cap]; 'precision', 'recall', 'F' float64 [..., C, cap] per class c < C; 'precision_all', 'recall_all', 'F_all'
    float64 [..., cap], class-agnostic: every row, the out-of-range row C included.  At tolerance T the matched pixels are the bins 1 .. T -- of side 1 for the
    precision (prediction-boundary pixels within T of a label boundary), of side 0 for the recall -- over the sum of all bins; F = 2 P R / (P + R); 0 / 0 is
    NaN.  Tolerances count from 1: the adjacent pixel is at distance 1, coincident contours at 1 or sqrt(2) (bins 1 and 2)."""
    h = _displacement(hist)
    cap, C = h.shape[-1] - 2, h.shape[-2] - 1
    total = h.sum(-1)
    matched = np.cumsum(h[..., 1:cap + 1], axis=-1)                          # [..., 2, C + 1, cap]
    prec, rec, f = _f_of(np.moveaxis(matched, -1, -3), total[..., None, :, :])      # [..., cap, C + 1]
    pa, ra, fa = _f_of(np.moveaxis(matched.sum(-2), -1, -2)[..., None], total.sum(-1)[..., None, :, None])
    out = OrderedDict(tolerance=np.arange(1, cap + 1, dtype=np.int64))
    for k, v in (("precision", prec), ("recall", rec), ("F", f)):
        out[k] = np.moveaxis(v[..., :C], -2, -1)
    for k, v in (("precision_all", pa), ("recall_all", ra), ("F_all", fa)):
        out[k] = v[..., 0]
    return out


def boundary_f_of(hist, tolerance):
    """The boundary F-score at one tolerance (an integer in 1 .. cap, counted from 1: the adjacent pixel is at distance 1) from int64
    [..., 2, C + 1, cap + 2] displacement counts -> OrderedDict 'precision', 'recall', 'F' float64 [..., C] and 'precision_all', 'recall_all', 'F_all'
    float64 [...]: `boundary_f_curve_of` at that tolerance."""
    h = _displacement(hist)
    cap = h.shape[-1] - 2
    if not _is_int(tolerance, 1, cap):
        raise ValueError(f"mmsa.evaluate: tolerance = {tolerance!r}; an integer in 1..{cap} (the histogram's cap; tolerances count from 1) is expected")
    c = boundary_f_curve_of(h)
    return OrderedDict((k, v[..., int(tolerance) - 1]) for k, v in c.items() if k != "tolerance")


def boundary_distance_percentile_of(hist, q=0.95):
    """The symmetric Hausdorff percentile HD-q from int64 [2, C + 1, cap + 2] displacement counts of ONE slot (or of a sum over slots) -> OrderedDict
    'label_to_pred', 'pred_to_label' (per side, over every row: the smallest bin k whose cumulative count reaches q * total, compared exactly in integers) and
    'hd' = the larger of the two, float64: "at most k pixels", counted from 1 as the bins are; inf where that bin is cap + 1 (further than the cap); NaN for a
    side without boundary pixels (and then for 'hd')."""
    h = _displacement(hist)
    if h.ndim != 3:
        raise ValueError(f"mmsa.evaluate: boundary_distance_percentile_of takes the [2, C + 1, cap + 2] counts of one slot, got {h.shape}")
    if isinstance(q, bool) or not isinstance(q, (int, float, np.integer, np.floating)) or not 0 < float(q) <= 1:
        raise ValueError(f"mmsa.evaluate: q = {q!r}; a share in (0, 1] is expected")
    cap = h.shape[-1] - 2
    frac = Fraction(float(q))
    vals = []
    for side in range(2):
        bins = [int(v) for v in h[side].sum(0)]
        total, cum, k = sum(bins), 0, None
        for k, v in enumerate(bins):
            cum += v
            if total and cum * frac.denominator >= frac.numerator * total:
                break
        vals.append(np.float64(np.nan) if total == 0 else np.float64(np.inf) if k == cap + 1 else np.float64(k))
    return OrderedDict(label_to_pred=vals[0], pred_to_label=vals[1], hd=np.float64(np.nan) if np.isnan(vals).any() else np.float64(max(vals)))


class EuclideanBoundaryEvaluator(BoundaryEvaluator):
    """BoundaryEvaluator at a EUCLIDEAN radius of up to 255 pixels, with the boundary F-score and the Hausdorff percentiles next to it.  `radius` (an int or a
    float in [1, 255]; the band is D2 <= floor(radius^2), formed exactly) or `radius2=` (that integer outright); `cap` (default ceil(radius); cap >= ceil(radius),
    cap <= 255): how far the distance maps -- and with them the displacement histogram, the tolerances of boundary_f() and distance_percentile() -- reach.
    `.counts` is the parent's int64 [n_slots, 4, C + 1, C + 1] buffer, zone 2 * near_label + near_pred, and trimap_metrics / interior_metrics / boundary_iou /
    summary / evaluator_counts / host_counts read it as the parent's; radius2=2 counts what BoundaryEvaluator(radius=1) counts, bit for bit.  `.displacement`
    (displacement=True) is the second device buffer, int64 [n_slots, 2, C + 1, cap + 2] (`boundary_displacement`).  Every entry's `boundary=` takes it.  add()
    makes two distance launches into buffers cached per shape and stream, one zone-count launch and one histogram launch: no host sync, and no allocation
    once the buffers of a shape exist.  Across ranks: mmsa.dist.allreduce_counts(be.counts) and allreduce_counts(be.displacement).  Tolerances and bins count
    from 1 (the adjacent pixel is at distance 1).  Up to 126 classes; with the histogram (C + 1) * (cap + 2) <= 16320."""
    _who, _read, _one = "EuclideanBoundaryEvaluator", "host_counts()", "a EuclideanBoundaryEvaluator"
    metric = "euclidean"

    def __init__(self, prep, radius=None, cap=None, border=False, displacement=True, cases=None, images=MAX_IMAGES, device=None, *, radius2=None):
        who = "mmsa.EuclideanBoundaryEvaluator"
        self.prep = prep
        self.radius2, least = euclidean_threshold(radius, radius2, who)
        self.tolerance = least      # the default tolerance of boundary_f(): ceil(radius)
        self.radius = radius if radius is not None else math.sqrt(self.radius2)
        self.cap = least if cap is None else check_distance_cap(cap, who)
        if self.cap < least:
            raise ValueError(f"{who}: cap = {cap} is below ceil(radius) = {least}: the distance maps would not reach the band's edge")
        self.border = bool(border)
        self.with_displacement = bool(displacement)
        C = _check_euclidean_classes(prep.num_classes, who)
        if self.with_displacement:
            _check_displacement_size(C, self.cap, who)
        self._init_slots(cases, images)
        self.displacement = None
        self._maps = {}         # (B, H, W, device, stream) -> (d2_pred, d2_label, scratch)
        self._init_buffer(device)

    def _trailing_displacement(self):
        return (2, self.prep.num_classes + 1, self.cap + 2)

    def _buffer(self, device):
        buf = super()._buffer(device)
        if self.with_displacement and self.displacement is None:
            self.displacement = torch.zeros(self.n_slots, *self._trailing_displacement(), dtype=torch.int64, device=buf.device)
        return buf

    def _maps_for(self, B, H, W, device):
        key = (B, H, W, device, ops._stream())
        m = self._maps.get(key)
        if m is None:
            if _capturing(device):
                raise RuntimeError(f"mmsa.{self._who}: the distance maps of a {B} x {H} x {W} batch cannot be allocated during a graph capture: run one add() "
                                   "of this shape before capturing")
            m = self._maps[key] = tuple(torch.empty(B, H, W, dtype=torch.uint16, device=device) for _ in range(3))
        return m

    def add(self, pred, labels, case=None, slots=None):
        """Count a batch of stored class maps: the distance maps of both sides (two launches each), the zone counts and, with displacement=True, the
        histogram; no host sync, no allocation once the buffers for the shape exist."""
        pred = _check_pred(pred)
        B, H, W = (int(v) for v in pred.shape)
        with torch.cuda.device(pred.device):
            self.prep.launch_args(labels, B, H, W, pred.device)      # the label side checked before the first launch
            return self._add(pred, B, case, slots, self._launches, pred, labels, guard=False)      # this guard serves

    def _launches(self, pred, labels, buf, use):
        """The launches of one add(), in its device guard, into the slots `use` of both buffers."""
        B, H, W = (int(v) for v in pred.shape)
        d2p, d2l, scratch = self._maps_for(B, H, W, pred.device)
        boundary_distance(pred, self.cap, self.border, num_classes=self.prep.num_classes, scratch=scratch, out=d2p)
        boundary_distance(labels, self.cap, self.border, labels_prep=self.prep, size=(H, W), scratch=scratch, out=d2l)
        boundary_counts_d2(pred, labels, self.prep, d2p, d2l, self.radius2, buf, use)
        if self.with_displacement:
            boundary_displacement(pred, labels, self.prep, d2p, d2l, self.cap, self.displacement, use)

    def reset(self):
        super().reset()
        if self.displacement is not None:
            self.displacement.zero_()

    def host_displacement(self):
        """The displacement histogram on the host: int64 numpy [n, 2, C + 1, cap + 2], n = images added so far / cases."""
        if not self.with_displacement:
            raise RuntimeError(f"mmsa.{self._who}: made with displacement=False: there is no displacement histogram (boundary F-score, Hausdorff percentiles)")
        return self._host("displacement", self._trailing_displacement())

    def _displacement_of(self, slot):
        return self._pick(self.host_displacement(), slot)

    def boundary_f(self, tolerance=None, slot=None):
        """`boundary_f_of` at `tolerance` (an integer in 1 .. cap, counted from 1; default: ceil(radius)), over every slot or
        of one slot."""
        return boundary_f_of(self._displacement_of(slot), self.tolerance if tolerance is None else tolerance)

    def boundary_f_curve(self, slot=None):
        """`boundary_f_curve_of`: precision, recall and F at every tolerance 1 .. cap."""
        return boundary_f_curve_of(self._displacement_of(slot))

    def distance_percentile(self, q=0.95, slot=None):
        """`boundary_distance_percentile_of`: the symmetric Hausdorff percentile, "at most k pixels"; inf beyond the cap."""
        return boundary_distance_percentile_of(self._displacement_of(slot), q)

    def summary(self, slot=None):
        """The parent's entries at the Euclidean band, then mBF (nanmean over the classes of the F-score at tolerance ceil(radius), rounded as the others)
        and HD95 in pixels (displacement=True), radius, radius2 and metric = 'euclidean'."""
        s = super().summary(slot)
        if self.with_displacement:
            with warnings.catch_warnings():
                warnings.simplefilter("ignore", RuntimeWarning)
                s["mBF"] = _round_percent(np.nanmean(self.boundary_f(slot=slot)["F"]))
            s["HD95"] = self.distance_percentile(0.95, slot)["hd"]
        s["radius"], s["radius2"], s["metric"] = self.radius, self.radius2, self.metric
        return s


# ---- segment-level evaluation: the connected components of the code maps, and what is counted from two of them (csrc/components.hip) ----
# For a code map M (the label codes L or the prediction codes P = min(pred, C) of the boundary passes above: an ignored label, 255, and C are codes like any
# other) two pixels of one image are connected iff they are 4- or 8-neighbours and hold the same code; a component -- a SEGMENT -- is a maximal connected set,
# and root(p) is the smallest linear index y * W + x of p's component within its own image.  Over every pixel whose own L is not 255 a label segment (side 0)
# and a prediction segment (side 1) collect their area and their hits (L < C and P == L): a prediction segment's area excludes ignored pixels, as every
# evaluator here does.  A segment of class c < C with area > 0 is counted once, at the size bucket s = min(23, floor(log2 area)) and the coverage bin
# k = floor(bins * hit / area): k == bins iff it is covered completely, and coverage >= j / bins iff k >= j.
SIZE_BUCKETS = 24                  # csrc/components.hip COMP_SIZE_BUCKETS: bucket s holds the areas 2^s .. 2^(s + 1) - 1, the last one everything from 2^23
MAX_SEGMENT_BINS = 64              # csrc/components.hip COMP_MAX_BINS
DEFAULT_SEGMENT_BINS = 10
_COMPONENT_SCRATCH = {}            # (device, stream) -> [root, area] int32 planes of suppress_small calls without root= / area=
_SEGMENT_SCRATCH = {}              # (device, stream) -> the int32 planes of segment_counts calls without scratch=


def check_connectivity(connectivity, who="mmsa.evaluate"):
    if not _is_int(connectivity, 4, 8) or int(connectivity) not in (4, 8):
        raise ValueError(f"{who}: connectivity = {connectivity!r}; 4 (edge neighbours) or 8 (edge and corner neighbours) is expected")
    return int(connectivity)


def check_segment_bins(bins, who="mmsa.evaluate"):
    if not _is_int(bins, 1, MAX_SEGMENT_BINS):
        raise ValueError(f"{who}: bins = {bins!r}; 1..{MAX_SEGMENT_BINS} coverage bins are supported")
    return int(bins)


def _check_int_plane(t, name, shape, device, what):
    if (not isinstance(t, torch.Tensor) or t.dtype != torch.int32 or tuple(t.shape) != tuple(shape) or not t.is_contiguous()
            or (device is not None and t.device != device)):
        raise RuntimeError(f"mmsa.evaluate: {name} must be a contiguous int32 {tuple(shape)} tensor{'' if device is None else f' on {device}'} ({what})")
    return t


@torch.no_grad()
def components(map, *, num_classes=None, labels_prep=None, size=None, connectivity=8, out=None):
    """The connected components of a code map (up to three launches, mmsa_components_u8) -> int32 [B, H, W] on the device: root[b, y, x] = the smallest linear
    index y * W + x of the pixel's component within its own image, so the output is canonical: the same bytes whatever the schedule.  Two pixels are connected
    iff they are 4- or 8-neighbours (`connectivity`) and hold the same code.  The map is read exactly as `boundary_distance` reads it, one of the keywords:
      num_classes=C     `map` is a stored uint8 class map [B, H, W]; the codes are P = min(map, C);
      labels_prep=prep  `map` holds raw uint8 labels [B, Hl, Wl]; the codes are the label codes L of `prep` (a class, C = kept but out of range, 255 = ignored: a
                        code like any other) on the grid `size=(H, W)` -- by default the size `prep` resizes an Hl x Wl label map to -- through the
                        nearest-neighbour tables of the label side.
    B * H * W < 2^31.  `out=` (int32 [B, H, W]) makes the call allocation-free: the launches work in it and need no scratch."""
    connectivity = check_connectivity(connectivity)
    _code_keywords("mmsa.evaluate: components", num_classes, labels_prep)
    src, grid = _code_map_grid(map, labels_prep, size, num_classes, index32="components")      # the class count too: before the device is looked at
    B, H, W = grid[0], grid[3], grid[4]
    _check_map(src, "map", torch.uint8, "a uint8 class map or raw uint8 labels")
    with torch.cuda.device(src.device):
        if out is None:
            out = torch.empty(B, H, W, dtype=torch.int32, device=src.device)
        else:
            _check_int_plane(out, "out", (B, H, W), src.device, "the root map")
        lib.call("mmsa_components_u8", *_code_map_args(src, grid, num_classes, labels_prep), connectivity, out.data_ptr(), ops._stream())
    return out


def _check_root(root, name="root", like=None, shape_only=False):
    return _check_map(root, name, torch.int32, "an int32 root map (mmsa.components)", like=like, shape_only=shape_only)


@torch.no_grad()
def component_areas(root, out=None):
    """The pixel count of every component at its root pixel, 0 elsewhere (one memset and one launch, mmsa_component_area) -> int32 [B, H, W] on the device.
    `root` is what `components` returns; a wave adds once per distinct root, so a component of half a frame costs no more than noise does."""
    root = _check_root(root, shape_only=True)
    if root.numel() == 0:
        raise RuntimeError(f"mmsa.evaluate: an empty map {tuple(root.shape)}")
    if out is not None:
        _check_int_plane(out, "out", root.shape, None, "the area plane")
    _check_root(root)
    B, H, W = (int(v) for v in root.shape)
    with torch.cuda.device(root.device):
        if out is None:
            out = torch.empty(B, H, W, dtype=torch.int32, device=root.device)
        elif out.device != root.device or out.data_ptr() == root.data_ptr():
            raise RuntimeError(f"mmsa.evaluate: out must live on {root.device}, and not be `root`")
        lib.call("mmsa_component_area", root.data_ptr(), B, H, W, out.data_ptr(), ops._stream())
    return out


@torch.no_grad()
def suppress_small(pred, min_area, *, num_classes, connectivity=8, fill=255, out=None, root=None, area=None, nearest=None):
    """The class map without its small blobs -> uint8 [B, H, W]: a pixel whose component (of the codes min(pred, C), at `connectivity`) has fewer than `min_area`
    pixels becomes `fill`, every other pixel is unchanged; min_area=1 is the identity.  The component launches, the area launch and one pointwise launch
    (mmsa_suppress_small_u8).  `out=` may be `pred` itself (in place); `root=` / `area=` (int32 [B, H, W] each) take the caller's planes -- they hold the root
    map and the areas afterwards -- so that a repeated call allocates nothing; without them buffers cached per device and stream are used.
    `nearest=cap` (None: the launches above alone): the removed blobs then take the class of what surrounds them, `fill_nearest(out, hole=fill, cap=nearest,
    out=out)` -- two more launches.  EVERY pixel that holds `fill` is filled, also one that held it before the call: a caller who wants 255 kept as void
    paints with another byte (fill=254).  `fill` must be no class: fill < num_classes with nearest= is a ValueError."""
    connectivity = check_connectivity(connectivity)
    if not _is_int(min_area, 1, (1 << 31) - 1):
        raise ValueError(f"mmsa.evaluate: min_area = {min_area!r}; an integer pixel count >= 1 is expected (1: nothing is removed)")
    if not _is_int(fill, 0, 255):
        raise ValueError(f"mmsa.evaluate: fill = {fill!r}; a byte 0..255 is expected")
    code_lut(num_classes)
    nearest = _check_nearest(nearest, fill, num_classes, "mmsa.evaluate: suppress_small")
    pred = _check_map(pred, "pred", torch.uint8, "a uint8 class map", shape_only=True)
    if pred.numel() == 0:
        raise RuntimeError(f"mmsa.evaluate: an empty map {tuple(pred.shape)}")
    if out is not None:
        _check_map(out, "out", torch.uint8, "a uint8 class map", like=pred, shape_only=True)
    for name, t in (("root", root), ("area", area)):
        if t is not None:
            _check_int_plane(t, name, pred.shape, None, "a caller's plane of suppress_small")
    _check_map(pred, "pred", torch.uint8, "a uint8 class map")
    B, H, W = (int(v) for v in pred.shape)
    n = B * H * W
    with torch.cuda.device(pred.device):
        if out is None:
            out = torch.empty_like(pred)
        else:
            _check_map(out, "out", torch.uint8, "a uint8 class map", like=pred)
        if root is None or area is None:
            cached = _cached_planes(_COMPONENT_SCRATCH, n, 2, pred.device, "the root and area planes of suppress_small")
            root = cached[0][:n].view(B, H, W) if root is None else root
            area = cached[1][:n].view(B, H, W) if area is None else area
        components(pred, num_classes=num_classes, connectivity=connectivity, out=root)
        component_areas(root, out=area)
        lib.call("mmsa_suppress_small_u8", pred.data_ptr(), root.data_ptr(), area.data_ptr(), B, H, W, int(min_area), int(fill), out.data_ptr(), ops._stream())
        if nearest is not None:
            fill_nearest(out, hole=int(fill), cap=nearest, out=out)
    return out


@torch.no_grad()
def segment_counts(pred, labels, prep, root_pred, root_label, bins=DEFAULT_SEGMENT_BINS, counts=None, scratch=None, slots=None):
    """ADD the segment counts of the uint8 class maps pred [B, H, W] against the raw labels into counts[slots[b]] (one memset and two launches,
    mmsa_eval_segments) -> counts, int64 [n_slots, 2, C, 24, bins + 1] on the device.  root_pred = components(pred, num_classes=C) and root_label =
    components(labels, labels_prep=prep, size=(H, W)), at one connectivity.  Every pixel whose own label code L is not 255 adds 1 to the area of its label
    segment (side 0) and of its prediction segment (side 1), and, where L < C and min(pred, C) == L, to their hits; then every segment with area > 0 and class
    c < C adds 1 at [slot, side, c, min(23, floor(log2 area)), floor(bins * hit / area)].  `scratch=` (an int32 tensor of at least 4 * B * H * W elements: the
    four planes area0, hit0, area1, hit1 at the root pixels, zeroed by the call and readable afterwards) makes the call allocation-free; without it a buffer
    cached per device and stream is used."""
    bins = check_segment_bins(bins)
    for only in (True, False):      # dtypes and shapes of all three first, then the devices
        pred = _check_map(pred, "pred", torch.uint8, "a uint8 class map", shape_only=only)
        root_pred = _check_root(root_pred, "root_pred", pred, only)
        root_label = _check_root(root_label, "root_label", pred, only)
    B, H, W = (int(v) for v in pred.shape)
    C = prep.num_classes
    n = 4 * B * H * W
    with torch.cuda.device(pred.device):
        if scratch is None:
            scratch = _cached_planes(_SEGMENT_SCRATCH, n, 1, pred.device, "the scratch planes of segment_counts")[0]
        else:
            _check_scratch(scratch, torch.int32, n, pred.device, count=f"4 * B * H * W = {n}")
        largs, counts, tab = _slot_launch(prep, labels, B, H, W, pred.device, counts, "counts", (2, C, SIZE_BUCKETS, bins + 1), slots)
        lib.call("mmsa_eval_segments", pred.data_ptr(), largs[0], B, H, W, largs[1], largs[2], largs[3], C, largs[4], largs[5], tab, counts.shape[0],
                 root_pred.data_ptr(), root_label.data_ptr(), bins, scratch.data_ptr(), counts.data_ptr(), ops._stream())
    return counts


def _segments(counts):
    c = np.asarray(counts)
    if c.ndim < 4 or c.shape[-4] != 2 or c.shape[-2] != SIZE_BUCKETS or c.shape[-1] < 2 or c.dtype.kind not in "iu":
        raise ValueError(f"mmsa.evaluate: segment counts are an integer [..., 2, C, {SIZE_BUCKETS}, bins + 1] array, got {c.dtype} {c.shape}")
    return c.astype(np.int64, copy=False)


def _area_bucket(v, name, lo):
    """An area limit -> its bucket edge: a power of two 2^s, lo <= s <= 23; anything else raises ValueError naming the nearest edges."""
    if not _is_int(v, 1, 1 << 62):
        raise ValueError(f"mmsa.evaluate: {name} = {v!r}; a pixel count (a power of two, the edge of a size bucket) is expected")
    v = int(v)
    s = v.bit_length() - 1
    if v != 1 << s or not lo <= s <= SIZE_BUCKETS - 1:
        below, above = max(lo, min(s, SIZE_BUCKETS - 1)), max(lo, min(s + 1, SIZE_BUCKETS - 1))
        raise ValueError(f"mmsa.evaluate: {name} = {v} is not the edge of a size bucket: the counts keep floor(log2 area) only and cannot split a bucket; the "
                         f"nearest edges are {1 << below} and {1 << above} (edges run from {1 << lo} to {1 << (SIZE_BUCKETS - 1)})")
    return s


def segment_totals_of(counts, min_area=1, max_area=None):
    """Fold the size buckets of int64 [..., 2, C, 24, bins + 1] segment counts -> int64 [..., 2, C, bins + 1]: the segments with min_area <= area < max_area
    (None: no upper limit).  Both limits must be powers of two, the edges of the buckets (at most 2^23, from where the last bucket holds everything)."""
    c = _segments(counts)
    s0 = _area_bucket(min_area, "min_area", 0)
    s1 = SIZE_BUCKETS if max_area is None else _area_bucket(max_area, "max_area", 1)
    if s1 <= s0:
        raise ValueError(f"mmsa.evaluate: max_area = {max_area} must be above min_area = {min_area}")
    return c[..., s0:s1, :].sum(-2)


def _coverage_bin(threshold, bins):
    if isinstance(threshold, bool) or not isinstance(threshold, (int, float, np.integer, np.floating, Fraction)) or not 0 <= threshold <= 1:
        raise ValueError(f"mmsa.evaluate: threshold = {threshold!r}; a coverage in [0, 1] is expected")
    k = round(float(threshold) * bins)
    if abs(float(threshold) * bins - k) > 1e-9:
        lo = math.floor(float(threshold) * bins)
        raise ValueError(f"mmsa.evaluate: threshold {float(threshold)!r} is not a bin edge of {bins} coverage bins (threshold * bins must be an integer): the "
                         f"counts cannot split bin {lo}; the nearest edges are {lo / bins!r} and {(lo + 1) / bins!r}")
    return int(k)


def segment_rate_of(counts, side, threshold=0.5, min_area=1, max_area=None):
    """The share of the segments of one side whose coverage is at least `threshold`, per class -> float64 [..., C]; 0 / 0 is NaN (a class without segments in
    that size range).  side 0: the label segments -- the segment RECALL, "was the object found"; side 1: the prediction segments -- the segment PRECISION, "is
    the blob real".  threshold * bins must be an integer: coverage >= k / bins holds iff the stored bin is >= k, so the rate is exact."""
    if isinstance(side, bool) or side not in (0, 1):
        raise ValueError(f"mmsa.evaluate: side = {side!r}; 0 (label segments: recall) or 1 (prediction segments: precision) is expected")
    t = segment_totals_of(counts, min_area, max_area)[..., int(side), :, :]
    k = _coverage_bin(threshold, t.shape[-1] - 1)
    with np.errstate(divide="ignore", invalid="ignore"):
        return t[..., k:].sum(-1).astype(np.float64) / t.sum(-1).astype(np.float64)


def segment_f_of(counts, threshold=0.5, min_area=1, max_area=None):
    """The harmonic mean of the segment precision and the segment recall per class -> float64 [..., C]; NaN where either is, and where both are 0."""
    r = segment_rate_of(counts, 0, threshold, min_area, max_area)
    p = segment_rate_of(counts, 1, threshold, min_area, max_area)
    with np.errstate(divide="ignore", invalid="ignore"):
        return 2 * p * r / (p + r)


class SegmentEvaluator(_SlotOwner):
    """Owns the segment counts of an evaluation run, as Evaluator owns the confusion counts: int64 [n_slots, 2, C, 24, bins + 1] on the device (`.counts`; side 0
    the label segments, side 1 the prediction segments, by class, size bucket min(23, floor(log2 area)) and coverage bin floor(bins * hit / area)).  Slots and
    cases as Evaluator's.  add() makes the two component launches (prediction and labels, at `connectivity`) and the count launch into buffers cached per shape
    and stream: no host sync, and no allocation once the buffers of a shape exist.  Every class-map entry's `segments=` takes it.  Across ranks:
    mmsa.dist.allreduce_counts(se.counts)."""
    _who, _read, _one = "SegmentEvaluator", "host_counts()", "a SegmentEvaluator"

    def __init__(self, prep, bins=DEFAULT_SEGMENT_BINS, connectivity=8, cases=None, images=MAX_IMAGES, device=None):
        who = "mmsa.SegmentEvaluator"
        self.prep = prep
        self.n_bins = check_segment_bins(bins, who)
        self.connectivity = check_connectivity(connectivity, who)
        if not 2 <= prep.num_classes <= 254:
            raise RuntimeError(f"{who}: {prep.num_classes} classes; a uint8 class map has 2..254")
        self._init_slots(cases, images)
        self._maps = {}         # (B, H, W, device, stream) -> (root_pred, root_label, scratch)
        self._init_buffer(device)

    def _trailing(self):
        return (2, self.prep.num_classes, SIZE_BUCKETS, self.n_bins + 1)

    def _maps_for(self, B, H, W, device):
        key = (B, H, W, device, ops._stream())
        m = self._maps.get(key)
        if m is None:
            if _capturing(device):
                raise RuntimeError(f"mmsa.{self._who}: the root maps of a {B} x {H} x {W} batch cannot be allocated during a graph capture: run one add() of "
                                   "this shape before capturing")
            m = self._maps[key] = (torch.empty(B, H, W, dtype=torch.int32, device=device), torch.empty(B, H, W, dtype=torch.int32, device=device),
                                   torch.empty(4, B, H, W, dtype=torch.int32, device=device))
        return m

    def add(self, pred, labels, case=None, slots=None):
        """Count a batch of stored class maps: the components of both sides and the segment counts; no host sync, no allocation once the buffers for the
        shape exist."""
        pred = _check_pred(pred)
        B, H, W = (int(v) for v in pred.shape)
        with torch.cuda.device(pred.device):
            self.prep.launch_args(labels, B, H, W, pred.device)      # the label side checked before the first launch
            return self._add(pred, B, case, slots, self._launches, pred, labels, guard=False)      # this guard serves

    def _launches(self, pred, labels, buf, use):
        B, H, W = (int(v) for v in pred.shape)
        root_pred, root_label, scratch = self._maps_for(B, H, W, pred.device)
        components(pred, num_classes=self.prep.num_classes, connectivity=self.connectivity, out=root_pred)
        components(labels, labels_prep=self.prep, size=(H, W), connectivity=self.connectivity, out=root_label)
        segment_counts(pred, labels, self.prep, root_pred, root_label, self.n_bins, buf, scratch, use)

    def host_counts(self):
        """The counts on the host (the ONE device-to-host copy): int64 numpy [n, 2, C, 24, bins + 1], n = images added so far / cases."""
        return self._host()

    def _of(self, slot):
        return self._pick(self.host_counts(), slot)

    def recall(self, threshold=0.5, min_area=1, max_area=None, slot=None):
        """The share of the LABEL segments covered to at least `threshold` by correct pixels, per class: float64 [C] (`segment_rate_of`, side 0)."""
        return segment_rate_of(self._of(slot), 0, threshold, min_area, max_area)

    def precision(self, threshold=0.5, min_area=1, max_area=None, slot=None):
        """The share of the PREDICTION segments covered to at least `threshold` by correct pixels, per class: float64 [C] (side 1)."""
        return segment_rate_of(self._of(slot), 1, threshold, min_area, max_area)

    def f1(self, threshold=0.5, min_area=1, max_area=None, slot=None):
        return segment_f_of(self._of(slot), threshold, min_area, max_area)

    def by_size(self, threshold=0.5, slot=None):
        """The rates per power-of-two size bucket -> OrderedDict: 'min_area' int64 [24] (2^s; the last bucket has no upper end), 'label_segments' /
        'pred_segments' int64 [24, C], 'recall' / 'precision' float64 [24, C] (NaN where a class has no segment of that size)."""
        c = self._of(slot)
        k = _coverage_bin(threshold, self.n_bins)
        total = np.moveaxis(c.sum(-1), -1, -2)                              # [2, 24, C]
        with np.errstate(divide="ignore", invalid="ignore"):
            rate = np.moveaxis(c[..., k:].sum(-1), -1, -2).astype(np.float64) / total.astype(np.float64)
        return OrderedDict(min_area=1 << np.arange(SIZE_BUCKETS, dtype=np.int64), label_segments=total[0], pred_segments=total[1], recall=rate[0],
                           precision=rate[1])

    def summary(self, slot=None):
        """The numbers of label and prediction segments (classes < C, area > 0) and mSR / mSP / mSF -- segment recall, precision and their harmonic mean at
        coverage 0.5, nanmean over the classes that have segments, rounded to two places of a percent; at an odd `bins` the threshold is the next edge
        above one half."""
        c = self._of(slot)
        thr = Fraction((self.n_bins + 1) // 2, self.n_bins)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore", RuntimeWarning)
            return OrderedDict(label_segments=int(c[0].sum()), pred_segments=int(c[1].sum()),
                               mSR=_round_percent(np.nanmean(segment_rate_of(c, 0, thr))), mSP=_round_percent(np.nanmean(segment_rate_of(c, 1, thr))),
                               mSF=_round_percent(np.nanmean(segment_f_of(c, thr))), threshold=float(thr), connectivity=self.connectivity)


# ---- panoptic quality: which prediction segment IS which label segment (csrc/pairs.hip) ----
# Segments, codes and roots are the section's above.  inter(p, g) = the hit pixels (L < C and P == L) with root_pred == p and root_label == g; p and g MATCH iff
# 3 * inter > area_p + area_g -- IoU > 1/2, strict, in integers -- and a segment has at most one match.  Over the segments of class c < C with area > 0 a
# matched pair is one TP (and adds floor(inter * 2^24 / union) to the IoU sum), an unmatched label segment one FN, an unmatched prediction segment one FP, at
# the size bucket of area_g (TP, FN) or area_p (FP): int64 [C, 24, 4] per slot.
PAIR_EMPTY = -1                    # an empty key of the pair table (all ones)
PAIR_MAX_PROBES = 128              # csrc/pairs.hip PAIR_MAX_PROBES: the slots a key looks at before it is dropped into `overflow`
PAIR_MAX_CAPACITY = 1 << 30        # csrc/pairs.hip PAIR_MAX_LOG2
IOU_ONE = 1 << 24                  # the fixed-point unit of the IoU sum (Calibration's CONF_ONE)
PQ_FIELDS = ("tp", "fp", "fn", "iou_sum")


def check_pair_capacity(capacity, who="mmsa.evaluate"):
    """The slots of a pair table: a power of two, 2 .. 2^30; anything else raises ValueError naming the neighbouring powers."""
    if not _is_int(capacity, 1, 1 << 62):
        raise ValueError(f"{who}: capacity = {capacity!r}; a number of table slots (a power of two, 2 .. 2^30) is expected")
    v = int(capacity)
    s = v.bit_length() - 1
    if v != 1 << s or not 2 <= v <= PAIR_MAX_CAPACITY:
        below, above = min(max(1 << s, 2), PAIR_MAX_CAPACITY), min(max(1 << (s + 1), 2), PAIR_MAX_CAPACITY)
        raise ValueError(f"{who}: capacity = {v} is not a power of two in 2 .. 2^30 (the slot of a key is the top bits of its hash); the neighbouring powers "
                         f"are {below} and {above}")
    return v


def default_pair_capacity(n):
    """The default slots for maps of n = B * H * W pixels: the next power of two >= n / 2 (at least 2).  A table must hold every distinct (label segment,
    prediction segment) pair that shares a hit pixel; maps of one-pixel segments that agree everywhere (n pairs) need capacity= spelled out."""
    return max(2, 1 << max(0, (int(n) + 1) // 2 - 1).bit_length())


class PairTable:
    """The pair table of `segment_pairs` on the device: keys int64 [capacity] (-1: empty; else ((b * H * W + root_label) << 31) | root_pred), counts int32
    [capacity] (the pair's hit pixels) and overflow int32 [1] (the hit pixels of keys that found no slot: the table was too small).  Which key sits in which
    slot depends on the schedule; the multiset of (key, count) does not.  `shape` = (B, H, W) of the maps it was filled from."""

    def __init__(self, keys, counts, overflow, shape=None):
        self.keys, self.counts, self.overflow, self.shape = keys, counts, overflow, shape

    @property
    def capacity(self):
        return int(self.keys.numel())

    @classmethod
    def empty(cls, capacity, device):
        capacity = check_pair_capacity(capacity)
        return cls(torch.empty(capacity, dtype=torch.int64, device=device), torch.empty(capacity, dtype=torch.int32, device=device),
                   torch.zeros(1, dtype=torch.int32, device=device))

    def _check(self, device):
        k, c, o = self.keys, self.counts, self.overflow
        ok = all(isinstance(t, torch.Tensor) and t.is_contiguous() and t.device == device for t in (k, c, o))
        if not ok or k.dtype != torch.int64 or c.dtype != torch.int32 or o.dtype != torch.int32 or k.dim() != 1 or c.shape != k.shape or o.numel() != 1:
            raise RuntimeError(f"mmsa.evaluate: a PairTable holds contiguous keys int64 [capacity], counts int32 [capacity] and overflow int32 [1] on {device}")
        check_pair_capacity(k.numel())
        return self

    def host(self):
        """The compact pair list -> int64 numpy arrays (image, root_label, root_pred, inter), sorted by (image, root_label, root_pred): two device-to-host
        copies and the overflow word.  Raises RuntimeError where the table overflowed: the list would be short."""
        lost = int(self.overflow.item())
        if lost:
            raise RuntimeError(f"mmsa.evaluate: the pair table of {self.capacity} slots overflowed ({lost} hit pixels were dropped): pass a larger capacity=")
        if self.shape is None:
            raise RuntimeError("mmsa.evaluate: a PairTable without its maps' shape= (B, H, W) cannot split a key into image and root")
        keys, counts = self.keys.cpu().numpy(), self.counts.cpu().numpy()
        used = keys != PAIR_EMPTY
        keys, counts = keys[used], counts[used].astype(np.int64)
        order = np.argsort(keys, kind="stable")
        keys, counts = keys[order], counts[order]
        HW = int(self.shape[1]) * int(self.shape[2])
        g = keys >> 31
        return g // HW, g % HW, keys & ((1 << 31) - 1), counts


def _check_pair_maps(pred, root_pred, root_label):
    for only in (True, False):      # dtypes and shapes of all three first, then the devices
        pred = _check_map(pred, "pred", torch.uint8, "a uint8 class map", shape_only=only)
        root_pred = _check_root(root_pred, "root_pred", pred, only)
        root_label = _check_root(root_label, "root_label", pred, only)
    if pred.numel() == 0:
        raise RuntimeError(f"mmsa.evaluate: an empty map {tuple(pred.shape)}")
    return pred, root_pred, root_label


def _check_classes_u8(C, who="mmsa.evaluate"):
    if not 2 <= C <= 254:
        raise RuntimeError(f"{who}: {C} classes; a uint8 class map has 2..254")
    return C


@torch.no_grad()
def segment_pairs(pred, labels, prep, root_pred, root_label, capacity=None, table=None):
    """The intersections of the (label segment, prediction segment) pairs of the uint8 class maps pred [B, H, W] and the raw labels (two memsets and one
    launch, mmsa_segment_pairs) -> PairTable on the device: the compact segment-pair list.  root_pred / root_label are `components`' of the two sides at one
    connectivity.  Every pixel whose label code L is a class and equals P = min(pred, C) adds 1 to the pair (root_label, root_pred) of its image.
    `capacity` (a power of two; default: the next one >= B * H * W / 2) sizes a new table whose overflow word starts at 0; `table=` (a PairTable of any
    capacity) is emptied and filled instead, allocation-free, and its overflow word is ADDED to (zero it to start anew).  Nothing is read back: look at
    `table.overflow`, or call `table.host()`, which raises where hit pixels were dropped."""
    if capacity is not None:
        capacity = check_pair_capacity(capacity)
    pred, root_pred, root_label = _check_pair_maps(pred, root_pred, root_label)
    B, H, W = (int(v) for v in pred.shape)
    C = _check_classes_u8(prep.num_classes)
    if B * H * W >= 1 << 31:
        raise RuntimeError(f"mmsa.evaluate: {B} x {H} x {W} pixels; a pair key holds a batch index in 31 bits (B * H * W < 2^31)")
    with torch.cuda.device(pred.device):
        largs = prep.launch_args(labels, B, H, W, pred.device)
        if table is None:
            table = PairTable.empty(default_pair_capacity(B * H * W) if capacity is None else capacity, pred.device)
        else:
            if not isinstance(table, PairTable):
                raise RuntimeError(f"mmsa.evaluate: table= takes an mmsa.evaluate.PairTable, got {type(table).__name__}")
            table._check(pred.device)
            if capacity is not None and capacity != table.capacity:
                raise RuntimeError(f"mmsa.evaluate: capacity={capacity} with a table of {table.capacity} slots")
        table.shape = (B, H, W)
        lib.call("mmsa_segment_pairs", pred.data_ptr(), largs[0], largs[1], largs[2], largs[3], C, largs[4], largs[5], root_pred.data_ptr(),
                 root_label.data_ptr(), B, H, W, table.keys.data_ptr(), table.counts.data_ptr(), table.capacity, table.overflow.data_ptr(), ops._stream())
    return table


@torch.no_grad()
def panoptic_counts(pred, labels, prep, root_pred, root_label, planes, table, counts=None, match=None, slots=None):
    """Match the pairs of `table` by IoU > 1/2 and ADD the TP / FP / FN counts and the IoU sum into counts[slots[b]] (one memset and two launches,
    mmsa_eval_panoptic) -> counts, int64 [n_slots, C, 24, 4] on the device ([.., c, s, :] = TP, FP, FN, sum of floor(IoU * 2^24) of the TPs; s = the size
    bucket of the label segment, of the prediction segment for an FP).  `planes` is the scratch `segment_counts` filled for the same maps (int32, at least
    4 * B * H * W elements: area0, hit0, area1, hit1), `table` what `segment_pairs` returned for them.  `match=` (int32 [2, B, H, W]; a new tensor by default)
    holds afterwards, at every label root, its prediction root and, at every prediction root, its label root; -1 elsewhere.  Nothing here looks at
    `table.overflow`: a table that overflowed gives short intersections -- PanopticEvaluator refuses to report from one."""
    pred, root_pred, root_label = _check_pair_maps(pred, root_pred, root_label)
    B, H, W = (int(v) for v in pred.shape)
    C = _check_classes_u8(prep.num_classes)
    n = 4 * B * H * W
    if (not isinstance(planes, torch.Tensor) or planes.dtype != torch.int32 or planes.numel() < n or planes.device != pred.device or not planes.is_contiguous()):
        raise RuntimeError(f"mmsa.evaluate: planes must be a contiguous int32 tensor of at least 4 * B * H * W = {n} elements on {pred.device} (the scratch of "
                           "segment_counts)")
    if not isinstance(table, PairTable):
        raise RuntimeError(f"mmsa.evaluate: table takes an mmsa.evaluate.PairTable, got {type(table).__name__}")
    table._check(pred.device)
    if match is not None:
        _check_int_plane(match, "match", (2, B, H, W), pred.device, "the match planes")
    with torch.cuda.device(pred.device):
        if match is None:
            match = torch.empty(2, B, H, W, dtype=torch.int32, device=pred.device)
        largs, counts, tab = _slot_launch(prep, labels, B, H, W, pred.device, counts, "counts", (C, SIZE_BUCKETS, 4), slots)
        lib.call("mmsa_eval_panoptic", pred.data_ptr(), largs[0], B, H, W, largs[1], largs[2], largs[3], C, largs[4], largs[5], tab, counts.shape[0],
                 root_pred.data_ptr(), root_label.data_ptr(), planes.data_ptr(), table.keys.data_ptr(), table.counts.data_ptr(), table.capacity,
                 match.data_ptr(), counts.data_ptr(), ops._stream())
    return counts


def _panoptic(counts):
    c = np.asarray(counts)
    if c.ndim < 3 or c.shape[-2] != SIZE_BUCKETS or c.shape[-1] != 4 or c.dtype.kind not in "iu":
        raise ValueError(f"mmsa.evaluate: panoptic counts are an integer [..., C, {SIZE_BUCKETS}, 4] array (TP, FP, FN, IoU sum), got {c.dtype} {c.shape}")
    return c.astype(np.int64, copy=False)


def panoptic_quality_of(counts, min_area=1, max_area=None):
    """int64 [..., C, 24, 4] panoptic counts -> OrderedDict per class: 'pq' = IoU sum / (TP + FP / 2 + FN / 2), 'sq' = IoU sum / TP, 'rq' = TP / (TP + FP / 2
    + FN / 2), float64 [..., C], 0 / 0 is NaN (a class without segments; 'sq': without a TP), and 'tp', 'fp', 'fn' int64 [..., C] -- over the segments with
    min_area <= area < max_area (powers of two, the bucket edges of `segment_totals_of`; the area is the label segment's, the prediction segment's for an
    FP).  The IoU sum is the sum of floor(IoU * 2^24) / 2^24: 'sq' lies below the exact mean IoU by less than 2^-24, 'pq' below sq * rq's exact value by
    less than 2^-24 as well."""
    c = _panoptic(counts)
    s0 = _area_bucket(min_area, "min_area", 0)
    s1 = SIZE_BUCKETS if max_area is None else _area_bucket(max_area, "max_area", 1)
    if s1 <= s0:
        raise ValueError(f"mmsa.evaluate: max_area = {max_area} must be above min_area = {min_area}")
    t = c[..., s0:s1, :].sum(-2)
    tp, fp, fn = t[..., 0], t[..., 1], t[..., 2]
    iou = t[..., 3].astype(np.float64) / IOU_ONE
    den = tp + 0.5 * fp + 0.5 * fn
    with np.errstate(divide="ignore", invalid="ignore"):
        return OrderedDict(pq=iou / den, sq=iou / tp.astype(np.float64), rq=tp / den, tp=tp, fp=fp, fn=fn)


def panoptic_summary_of(counts, things=None):
    """PQ / SQ / RQ of int64 [C, 24, 4] counts: the nanmean over the classes present (PQ, RQ: with a segment on either side; SQ: with a TP), rounded to two
    places of a percent, and the totals 'tp', 'fp', 'fn'.  `things=` (class indices) restricts them: PQ_th / SQ_th / RQ_th over those classes and PQ_st /
    SQ_st / RQ_st over the others are added."""
    q = panoptic_quality_of(counts)
    C = q["pq"].shape[-1]
    if q["pq"].ndim != 1:
        raise ValueError(f"mmsa.evaluate: a summary is formed from the counts of one slot [C, {SIZE_BUCKETS}, 4], got {np.asarray(counts).shape}")

    def mean(v, keep):
        with warnings.catch_warnings():
            warnings.simplefilter("ignore", RuntimeWarning)
            return _round_percent(np.nanmean(v[keep])) if keep.any() else float("nan")

    every = np.ones(C, dtype=bool)
    s = OrderedDict((k.upper(), mean(q[k], every)) for k in ("pq", "sq", "rq"))
    if things is not None:
        th = [things] if _is_int(things, 0, C - 1) else list(things)
        if not th or any(not _is_int(t, 0, C - 1) for t in th) or len(set(int(t) for t in th)) != len(th):
            raise ValueError(f"mmsa.evaluate: things = {things!r}; a list of distinct class indices in 0..{C - 1} is expected")
        keep = np.zeros(C, dtype=bool)
        keep[[int(t) for t in th]] = True
        for tag, k in (("th", keep), ("st", ~keep)):
            for name in ("pq", "sq", "rq"):
                s[f"{name.upper()}_{tag}"] = mean(q[name], k)
    s["tp"], s["fp"], s["fn"] = int(q["tp"].sum()), int(q["fp"].sum()), int(q["fn"].sum())
    return s


class PanopticEvaluator(_SlotOwner):
    """Owns the panoptic counts of an evaluation run, as SegmentEvaluator owns the segment counts: int64 [n_slots, C, 24, 4] on the device (`.counts`: TP, FP, FN
    and the fixed-point IoU sum by class and size bucket).  Slots and cases as Evaluator's.  add() makes, into buffers cached per shape and stream, the two
    component calls, `segment_counts` (bins=1, into a private buffer: its scratch planes are the areas), `segment_pairs` and `panoptic_counts`: no host sync,
    and no allocation once the buffers of a shape exist.  `capacity` (a power of two) sizes the pair table; None: the next power of two >= B * H * W / 2 of
    every shape.  A table that was too small drops hit pixels into the device word that `overflow()` reads, and every host reduction raises RuntimeError
    then: the counts are never silently short.  `things` = the class indices `summary()` reports PQ_th / PQ_st for.  Every class-map entry's `panoptic=` takes
    it.  Across ranks: mmsa.dist.allreduce_counts(pe.counts)."""
    _who, _read, _one = "PanopticEvaluator", "host_counts()", "a PanopticEvaluator"

    def __init__(self, prep, connectivity=8, capacity=None, cases=None, things=None, images=MAX_IMAGES, device=None):
        who = "mmsa.PanopticEvaluator"
        self.prep = prep
        self.connectivity = check_connectivity(connectivity, who)
        self.capacity = None if capacity is None else check_pair_capacity(capacity, who)
        _check_classes_u8(prep.num_classes, who)
        self.things = None if things is None else list(things)
        if self.things is not None:
            panoptic_summary_of(np.zeros((prep.num_classes, SIZE_BUCKETS, 4), dtype=np.int64), self.things)      # refused here, not at the first summary
        self._init_slots(cases, images)
        self._maps = {}         # (B, H, W, device, stream) -> (root_pred, root_label, scratch, match, PairTable)
        self._sides = None      # int64 [n_slots, 2, C, 24, 2]: what segment_counts adds at bins=1 (the segments of both sides by class and size)
        self._overflow = None   # int32 [1]: the overflow word of every table of this evaluator
        self._init_buffer(device)

    def _trailing(self):
        return (self.prep.num_classes, SIZE_BUCKETS, 4)

    def _buffer(self, device):
        buf = super()._buffer(device)              # refuses to allocate during a capture
        if self._sides is None:                    # made with the counts: whoever has the one has the others
            self._sides = torch.zeros(self.n_slots, 2, self.prep.num_classes, SIZE_BUCKETS, 2, dtype=torch.int64, device=device)
            self._overflow = torch.zeros(1, dtype=torch.int32, device=device)
        return buf

    def _maps_for(self, B, H, W, device):
        key = (B, H, W, device, ops._stream())
        m = self._maps.get(key)
        if m is None:
            if _capturing(device):
                raise RuntimeError(f"mmsa.{self._who}: the root maps of a {B} x {H} x {W} batch cannot be allocated during a graph capture: run one add() of "
                                   "this shape before capturing")
            capacity = default_pair_capacity(B * H * W) if self.capacity is None else self.capacity
            table = PairTable(torch.empty(capacity, dtype=torch.int64, device=device), torch.empty(capacity, dtype=torch.int32, device=device), self._overflow,
                              (B, H, W))
            m = self._maps[key] = (torch.empty(B, H, W, dtype=torch.int32, device=device), torch.empty(B, H, W, dtype=torch.int32, device=device),
                                   torch.empty(4, B, H, W, dtype=torch.int32, device=device), torch.empty(2, B, H, W, dtype=torch.int32, device=device), table)
        return m

    def add(self, pred, labels, case=None, slots=None):
        """Count a batch of stored class maps: the components of both sides, their areas, the pair table, the matches and the counts; no host sync, no
        allocation once the buffers for the shape exist."""
        pred = _check_pred(pred)
        B, H, W = (int(v) for v in pred.shape)
        with torch.cuda.device(pred.device):
            self.prep.launch_args(labels, B, H, W, pred.device)      # the label side checked before the first launch
            return self._add(pred, B, case, slots, self._launches, pred, labels, guard=False)      # this guard serves

    def _launches(self, pred, labels, buf, use):
        B, H, W = (int(v) for v in pred.shape)
        root_pred, root_label, scratch, match, table = self._maps_for(B, H, W, pred.device)
        components(pred, num_classes=self.prep.num_classes, connectivity=self.connectivity, out=root_pred)
        components(labels, labels_prep=self.prep, size=(H, W), connectivity=self.connectivity, out=root_label)
        segment_counts(pred, labels, self.prep, root_pred, root_label, 1, self._sides, scratch, use)
        segment_pairs(pred, labels, self.prep, root_pred, root_label, table=table)
        panoptic_counts(pred, labels, self.prep, root_pred, root_label, scratch, table, buf, match, use)

    def reset(self):
        super().reset()
        if self._sides is not None:
            self._sides.zero_()
            self._overflow.zero_()

    def overflow(self):
        """The hit pixels that found no slot in a pair table since the last reset() (one word from the device); 0: every count is complete."""
        return 0 if self._overflow is None else int(self._overflow.item())

    def host_counts(self):
        """The counts on the host: int64 numpy [n, C, 24, 4], n = images added so far / cases.  RuntimeError where a pair table overflowed."""
        lost = self.overflow()
        if lost:
            raise RuntimeError(f"mmsa.{self._who}: a pair table overflowed ({lost} hit pixels found no slot), so intersections are short and matches may be "
                               f"missing: make the {self._who} with a larger capacity= (a power of two; "
                               f"{'the default, half the pixels of a batch,' if self.capacity is None else self.capacity} was too small) and count again")
        return self._host()

    def _of(self, slot):
        return self._pick(self.host_counts(), slot)

    def quality(self, min_area=1, max_area=None, slot=None):
        """`panoptic_quality_of` of one slot (index or case name) or of the sum over every slot."""
        return panoptic_quality_of(self._of(slot), min_area, max_area)

    def pq(self, min_area=1, max_area=None, slot=None):
        """Panoptic quality per class: float64 [C], NaN for a class without segments."""
        return self.quality(min_area, max_area, slot)["pq"]

    def sq(self, min_area=1, max_area=None, slot=None):
        """Segmentation quality per class, the mean IoU of the matched pairs: float64 [C], NaN without a TP."""
        return self.quality(min_area, max_area, slot)["sq"]

    def rq(self, min_area=1, max_area=None, slot=None):
        """Recognition quality per class, the F1 of the matching: float64 [C]."""
        return self.quality(min_area, max_area, slot)["rq"]

    def by_size(self, slot=None):
        """The counts and qualities per power-of-two size bucket -> OrderedDict: 'min_area' int64 [24], 'tp' / 'fp' / 'fn' int64 [24, C], 'pq' / 'sq' / 'rq'
        float64 [24, C] (NaN where a class has no segment of that size)."""
        c = np.moveaxis(self._of(slot), -2, -3)                              # [24, C, 4]
        den = c[..., 0] + 0.5 * c[..., 1] + 0.5 * c[..., 2]
        iou = c[..., 3].astype(np.float64) / IOU_ONE
        with np.errstate(divide="ignore", invalid="ignore"):
            return OrderedDict(min_area=1 << np.arange(SIZE_BUCKETS, dtype=np.int64), tp=c[..., 0], fp=c[..., 1], fn=c[..., 2], pq=iou / den,
                               sq=iou / c[..., 0].astype(np.float64), rq=c[..., 0] / den)

    def summary(self, slot=None):
        """PQ / SQ / RQ (`panoptic_summary_of`, with this evaluator's `things`), the totals, and the connectivity."""
        s = panoptic_summary_of(self._of(slot), self.things)
        s["connectivity"] = self.connectivity
        return s


# ---- the segment table: the segments of a code map handed out (csrc/segtable.hip) ----
# Code map, connectivity and roots are `components`'.  A component of image b is LISTED iff its area >= min_area and its code is a class (< C); void=True also
# lists the components of the other codes (C, and 255 on the label side).  The listed segments of an image are numbered 0 .. n_b - 1 in ascending order of
# their root index -- the raster order of their first pixel -- so the numbering is canonical.  count[b] = n_b; ids[b, y, x] = the number of the pixel's segment
# (-1: not listed); records[b, k] = ROOT, CLASS, AREA, X0, Y0, X1, Y1, SUM_X, SUM_Y, SUM_Q for k < min(n_b, capacity), zero rows behind them.
SEGTAB_BLOCK = 2048                # csrc/segtable.hip SEGTAB_BLOCK: the pixels per block of the compaction (one scratch word each)
SCAN_LANES = 256                   # csrc/compact.h COMPACT_SCAN_LANES: the lanes of the compaction's scan workgroup (segment table and run tables alike)
SCAN_TRIP = 1024                   # csrc/compact.h COMPACT_SCAN_TRIP: the block counts one trip of the scan takes
SEGMENT_FIELDS = ("ROOT", "CLASS", "AREA", "X0", "Y0", "X1", "Y1", "SUM_X", "SUM_Y", "SUM_Q")
ROOT, CLASS, AREA, X0, Y0, X1, Y1, SUM_X, SUM_Y, SUM_Q = range(10)
SCORE_ONE = CONF_ONE               # the fixed-point unit of a record's score sum: SUM_Q = sum of floor(clamp(value) * 2^24)
MIN_SEGMENT_CAPACITY = 1024
SEGMENT_DTYPE = np.dtype([("image", np.int64), ("id", np.int64), ("root", np.int64), ("category", np.int64), ("area", np.int64), ("bbox", np.int64, (4,)),
                          ("centroid", np.float64, (2,)), ("score", np.float64)])


_library_checked = set()


def _check_library(kind, **getters):
    """Once per process and table kind: the named constants of this module are the loaded library's (a variant build, MMSA_LIB, would get a wrong scratch)."""
    if kind not in _library_checked:
        for name, get in getters.items():
            if get() != globals()[name]:
                raise RuntimeError(f"mmsa.evaluate: the library's {kind} constant {name} is {get()}, mmsa.evaluate.{name} is {globals()[name]}")
        _library_checked.add(kind)


def _check_rows(who, B, capacity, rows):
    if B * capacity >= 1 << 31:
        raise RuntimeError(f"{who}: {B} images of {capacity} {rows}; a row is indexed in 32 bits (B * capacity < 2^31)")


def _overflow_error(who, image, n, rows, things, lost, remedy):
    return RuntimeError(f"{who}: image {image} has {n} {things} and the table {rows} rows: {lost} {n - rows} were dropped; {remedy} with a larger capacity= "
                        f"(capacity=H * W can never overflow)")


def default_segment_capacity(H, W):
    """The default rows per image of a segment table: max(1024, H * W // 64)."""
    return max(MIN_SEGMENT_CAPACITY, int(H) * int(W) // 64)


def check_segment_capacity(capacity, who="mmsa.evaluate"):
    if not _is_int(capacity, 1, (1 << 31) - 1):
        raise ValueError(f"{who}: capacity = {capacity!r}; a positive number of rows per image is expected (None: max({MIN_SEGMENT_CAPACITY}, H * W // 64))")
    return int(capacity)


def score_threshold_q(t):
    """floor(t * 2^24) of a score threshold t in [0, 1], exactly: the integer `keep(min_score=t)` tests SUM_Q >= q * AREA with."""
    if isinstance(t, bool) or not isinstance(t, (int, float, np.integer, np.floating, Fraction)) or not 0 <= t <= 1:
        raise ValueError(f"mmsa.evaluate: min_score = {t!r}; a score in [0, 1] is expected")
    return int(Fraction(t) * SCORE_ONE // 1)


def segment_records_of(records, count, scored=True, image=0):
    """The host reading of raw records: integer [rows, 10] (one image's rows of `records`) and its `count` -> a numpy structured array of `count` segments with
    'image', 'id', 'root', 'category' (the code), 'area', 'bbox' (COCO: x, y, width, height), 'centroid' (x, y) = (SUM_X / AREA, SUM_Y / AREA) and 'score' =
    SUM_Q / (AREA * 2^24), float64 from those integers; 0 / 0 is NaN, and the score is NaN with scored=False (a table filled without `values`).  Raises
    RuntimeError naming capacity= where count exceeds the rows: the list would be short."""
    r = np.asarray(records)
    if r.ndim != 2 or r.shape[1] != len(SEGMENT_FIELDS) or r.dtype.kind not in "iu":
        raise ValueError(f"mmsa.evaluate: segment records are an integer [rows, {len(SEGMENT_FIELDS)}] array ({', '.join(SEGMENT_FIELDS)}), got {r.dtype} {r.shape}")
    n = int(count)
    if n < 0:
        raise ValueError(f"mmsa.evaluate: count = {n}")
    if n > r.shape[0]:
        raise _overflow_error("mmsa.evaluate", image, n, r.shape[0], "listed segments", "the records of the last", "fill a table")
    r = r[:n].astype(np.int64, copy=False)
    out = np.zeros(n, dtype=SEGMENT_DTYPE)
    out["image"], out["id"], out["root"], out["category"], out["area"] = image, np.arange(n), r[:, ROOT], r[:, CLASS], r[:, AREA]
    out["bbox"] = np.stack([r[:, X0], r[:, Y0], r[:, X1] - r[:, X0] + 1, r[:, Y1] - r[:, Y0] + 1], 1)
    area = r[:, AREA].astype(np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        out["centroid"] = np.stack([r[:, SUM_X] / area, r[:, SUM_Y] / area], 1)
        out["score"] = r[:, SUM_Q] / (area * SCORE_ONE) if scored else np.nan
    return out


class SegmentTable:
    """Owns the segment table of a batch of code maps on the device: `count` int32 [B], `records` int64 [B, capacity, 10], `ids` int32 [B, H, W], and the
    scratch of the launches (the root map, the area plane where min_area > 1, the block counts of the prefix sum).  One of the keywords says how a map is read,
    as `components` reads one: num_classes=C (a stored uint8 class map, codes min(map, C)) or labels_prep=prep (raw labels through the LUT and the
    nearest-neighbour tables).  A component is listed iff its area >= min_area and its code is a class; void=True also lists the other codes.  `capacity` = the
    rows per image (None: max(1024, H * W // 64) of every shape); the records of the segments beyond it are dropped, `count` keeps the true number and
    `overflow()` / `host()` say so.  update() makes the launches into buffers cached per shape and stream: no host sync, and no allocation once the buffers of a
    shape exist.  Every class-map entry's `segment_table=` takes one made with num_classes=.  runs="column" or "row": update() also fills `self.runs`, the
    RunTable of `ids` in that order (the launches of `run_lengths` into buffers of the same cache, `run_capacity` rows per image; None: max(4096,
    H * W // 8)), and with "column" `segments_info(b, masks=True)` carries every segment's COCO RLE.  runs=None: the launches are the ones above alone."""

    def __init__(self, num_classes=None, labels_prep=None, connectivity=8, min_area=1, void=False, capacity=None, runs=None, run_capacity=None):
        who = "mmsa.SegmentTable"
        self.run_order = None if runs is None else check_run_order(runs, who)
        self._run_capacity = None if run_capacity is None else check_run_capacity(run_capacity, who)
        self.runs = None         # the RunTable of `ids` of the last update (runs= given)
        _code_keywords(f"{who}:", num_classes, labels_prep, "stored class maps")
        if labels_prep is None:
            code_lut(num_classes)
        self.num_classes = int(num_classes) if labels_prep is None else int(labels_prep.num_classes)
        self.labels_prep = labels_prep
        self.connectivity = check_connectivity(connectivity, who)
        if not _is_int(min_area, 1, (1 << 31) - 1):
            raise ValueError(f"{who}: min_area = {min_area!r}; an integer pixel count >= 1 is expected (1: every component)")
        self.min_area = int(min_area)
        if not isinstance(void, (bool, np.bool_)):
            raise ValueError(f"{who}: void = {void!r}; True (list the components of every code) or False (of the classes only) is expected")
        self.void = bool(void)
        self._capacity = None if capacity is None else check_segment_capacity(capacity, who)
        self._maps = {}          # (B, H, W, device, stream) -> dict(count, records, ids, scratch, root, area)
        self.count = self.records = self.ids = self.root = None
        self.shape = None        # (B, H, W) of the last update
        self.scored = False      # the last update had `values`

    @property
    def capacity(self):
        """The rows per image: the constructor's, or the default of the last update's shape (None before the first)."""
        return self._capacity if self._capacity is not None or self.shape is None else default_segment_capacity(self.shape[1], self.shape[2])

    def _maps_for(self, B, H, W, device):
        key = (B, H, W, device, ops._stream())
        m = self._maps.get(key)
        if m is None:
            if _capturing(device):
                raise RuntimeError(f"mmsa.SegmentTable: the buffers of a {B} x {H} x {W} batch cannot be allocated during a graph capture: run one update() of this "
                                   "shape before capturing")
            capacity = default_segment_capacity(H, W) if self._capacity is None else self._capacity
            _check_library("segment table", SEGTAB_BLOCK=lib.raw.mmsa_segment_table_block)
            _check_rows("mmsa.SegmentTable", B, capacity, "rows")
            blocks = -(-H * W // SEGTAB_BLOCK)
            m = self._maps[key] = dict(count=torch.zeros(B, dtype=torch.int32, device=device),
                                       records=torch.zeros(B, capacity, len(SEGMENT_FIELDS), dtype=torch.int64, device=device),
                                       ids=torch.empty(B, H, W, dtype=torch.int32, device=device), scratch=torch.empty(B * blocks, dtype=torch.int32, device=device),
                                       root=torch.empty(B, H, W, dtype=torch.int32, device=device),
                                       area=torch.empty(B, H, W, dtype=torch.int32, device=device) if self.min_area > 1 else None,
                                       runs=None if self.run_order is None else RunTable.empty(
                                           B, H, W, self.run_order, default_run_capacity(H, W) if self._run_capacity is None else self._run_capacity, device))
        return m

    @torch.no_grad()
    def update(self, map, values=None, root=None):
        """Fill the table from a batch of maps (the component launches unless `root=` brings the root map `components` made of this map at this connectivity,
        the area launch where min_area > 1, one memset and four launches of mmsa_segment_table) -> self.  `values` (float32 [B, H, W] on the grid of the code
        map: a confidence, margin or entropy map, or a probs[r] plane) fills SUM_Q; without it SUM_Q is 0 and every score NaN."""
        num_classes = None if self.labels_prep is not None else self.num_classes
        src, grid = _code_map_grid(map, self.labels_prep, index32="a segment table")
        B, H, W = grid[0], grid[3], grid[4]
        if root is not None:
            _check_int_plane(root, "root", (B, H, W), None, "the root map of mmsa.components")
        if values is not None:
            if not isinstance(values, torch.Tensor) or values.dtype != torch.float32 or tuple(values.shape) != (B, H, W) or not values.is_contiguous():
                raise RuntimeError(f"mmsa.evaluate: values must be a contiguous float32 {(B, H, W)} tensor (a confidence, margin or entropy map, or a probs plane)")
        _check_map(src, "map", torch.uint8, "a uint8 class map or raw uint8 labels")
        for name, t in (("root", root), ("values", values)):
            if t is not None and t.device != src.device:
                raise RuntimeError(f"mmsa.evaluate: {name} is on {t.device}, the map on {src.device}")
        with torch.cuda.device(src.device):
            m = self._maps_for(B, H, W, src.device)
            if root is None:
                root = components(src, num_classes=num_classes, labels_prep=self.labels_prep, size=(H, W), connectivity=self.connectivity, out=m["root"])
            if self.min_area > 1:
                component_areas(root, out=m["area"])
            capacity = m["records"].shape[1]
            lib.call("mmsa_segment_table", *_code_map_args(src, grid, num_classes, self.labels_prep), root.data_ptr(),
                     None if m["area"] is None else m["area"].data_ptr(), None if values is None else values.data_ptr(), self.min_area,
                     256 if self.void else self.num_classes, capacity, m["count"].data_ptr(), m["ids"].data_ptr(), m["records"].data_ptr(),
                     m["scratch"].data_ptr(), ops._stream())
            if m["runs"] is not None:
                run_lengths(m["ids"], table=m["runs"])
        self.count, self.records, self.ids, self.root, self.runs = m["count"], m["records"], m["ids"], root, m["runs"]
        self.shape, self.scored = (B, H, W), values is not None
        return self

    def _filled(self):
        if self.shape is None:
            raise RuntimeError("mmsa.SegmentTable: nothing was filled yet: call update()")

    def overflow(self):
        """Whether an image of the last update has more listed segments than rows (the device words of `count`): its last records were dropped."""
        self._filled()
        return bool((self.count > self.records.shape[1]).any().item())

    def host(self, b=None):
        """The segments on the host (`segment_records_of`: two device-to-host copies) -> a numpy structured array with 'image', 'id', 'root', 'category',
        'area', 'bbox', 'centroid' and 'score'; of image `b`, or of every image in turn.  RuntimeError naming capacity= where an image has more segments than
        rows."""
        self._filled()
        B = self.shape[0]
        if b is not None and not _is_int(b, 0, B - 1):
            raise ValueError(f"mmsa.SegmentTable: b = {b!r}; an image index 0..{B - 1} (or None: every image) is expected")
        count = self.count.cpu().numpy()
        cap = int(self.records.shape[1])
        for i in range(B):
            if count[i] > cap:
                raise _overflow_error("mmsa.SegmentTable", i, int(count[i]), cap, "listed segments", "the records of the last", "make the SegmentTable")
        records = self.records.cpu().numpy()
        images = range(B) if b is None else [int(b)]
        parts = [segment_records_of(records[i], count[i], self.scored, i) for i in images]
        return parts[0] if len(parts) == 1 else np.concatenate(parts)

    def segments_info(self, b, masks=False):
        """The `segments_info` list of the COCO panoptic format for image b: dicts with 'id' (the dense id + 1: the format's PNG is `ids + 1`, 0 = VOID),
        'category_id', 'area', 'bbox' [x, y, width, height] and 'iscrowd' 0, and next to them 'centroid' [x, y] and 'score' (None without `values`).
        masks=True adds 'segmentation', the segment's uncompressed COCO RLE (`coco_rle_of` on the runs of `ids`): a table made with runs="column" has them,
        any other raises ValueError."""
        if masks and self.run_order != "column":
            raise ValueError(f"mmsa.SegmentTable: segments_info(masks=True) reads the column-major runs of ids: make the SegmentTable with runs='column' "
                             f"(this one has runs={self.run_order!r})")
        info = [dict(id=int(s["id"]) + 1, category_id=int(s["category"]), area=int(s["area"]), bbox=[int(v) for v in s["bbox"]], iscrowd=0,
                     centroid=[float(v) for v in s["centroid"]], score=float(s["score"]) if self.scored else None) for s in self.host(int(b))]
        if masks and info:
            H, W = self.shape[1:]
            starts, lengths, values = self.runs.host(int(b))
            by = np.argsort(values, kind="stable")                             # the runs grouped by id, ascending starts within one
            lo, hi = (np.searchsorted(values[by], np.arange(len(info)), side) for side in ("left", "right"))
            for k, d in enumerate(info):
                at = by[lo[k]:hi[k]]
                d["segmentation"] = {"size": [H, W], "counts": _rle_counts(starts[at], lengths[at], H * W)}
        return info

    @torch.no_grad()
    def keep(self, min_area=None, max_area=None, min_score=None, classes=None):
        """Which rows pass -> uint8 [B, capacity] on the device (1: keep), for `select_segments`: min_area <= AREA < max_area, mean score >= min_score -- tested
        in integers, SUM_Q >= floor(min_score * 2^24) * AREA -- and CLASS among `classes`.  Torch operations on `records`: no host sync.  Empty rows are 0."""
        self._filled()
        r = self.records
        area = r[..., AREA]
        ok = area > 0
        for name, v in (("min_area", min_area), ("max_area", max_area)):
            if v is not None and not _is_int(v, 1, 1 << 62):
                raise ValueError(f"mmsa.SegmentTable: {name} = {v!r}; a pixel count >= 1 is expected")
        if min_area is not None:
            ok = ok & (area >= int(min_area))
        if max_area is not None:
            ok = ok & (area < int(max_area))
        if min_score is not None:
            q = score_threshold_q(min_score)
            if not self.scored:
                raise RuntimeError("mmsa.SegmentTable: min_score= on a table filled without values=: there is no score to test")
            ok = ok & (r[..., SUM_Q] >= area * q)
        if classes is not None:
            cs = [classes] if _is_int(classes, 0, 255) else list(classes)
            if not cs or any(not _is_int(c, 0, 255) for c in cs):
                raise ValueError(f"mmsa.SegmentTable: classes = {classes!r}; a list of codes 0..255 is expected")
            among = torch.zeros_like(ok)
            for c in sorted(set(int(c) for c in cs)):
                among = among | (r[..., CLASS] == c)
            ok = ok & among
        return ok.to(torch.uint8)


@torch.no_grad()
def segment_table(map, *, num_classes=None, labels_prep=None, values=None, root=None, connectivity=8, min_area=1, void=False, capacity=None, table=None):
    """The launches of SegmentTable.update alone -> the table: a new SegmentTable of these options, or `table=` (a SegmentTable, whose own options hold: an
    option spelled out here must agree with it), filled from `map`."""
    if table is None:
        table = SegmentTable(num_classes=num_classes, labels_prep=labels_prep, connectivity=connectivity, min_area=min_area, void=void, capacity=capacity)
    else:
        if not isinstance(table, SegmentTable):
            raise RuntimeError(f"mmsa.evaluate: table= takes an mmsa.evaluate.SegmentTable, got {type(table).__name__}")
        for name, v, default, own in (("num_classes", num_classes, None, None if table.labels_prep is not None else table.num_classes),
                                      ("labels_prep", labels_prep, None, table.labels_prep), ("connectivity", connectivity, 8, table.connectivity),
                                      ("min_area", min_area, 1, table.min_area), ("void", void, False, table.void), ("capacity", capacity, None, table._capacity)):
            if v is not default and v != default and v != own and v is not own:
                raise RuntimeError(f"mmsa.evaluate: {name}={v!r} with a table made with {name}={own!r}")
    return table.update(map, values=values, root=root)


@torch.no_grad()
def select_segments(pred, table, keep, fill=255, out=None, nearest=None):
    """The class map with the segments that `keep` drops painted over (one pointwise launch, mmsa_select_segments_u8) -> uint8 [B, H, W]: `fill` where the
    pixel's id is a row of the table and keep[b, id] == 0, `pred` elsewhere -- a pixel whose segment is not listed (id -1) or has no row (id >= capacity) is
    unchanged.  `table` = a filled SegmentTable of this shape, `keep` = uint8 [B, capacity] on the device (`table.keep(...)`, or any mask made from
    `table.records`); `out=` may be `pred` itself.  The instance-level sibling of `abstain`.
    `nearest=cap` (None: the launch above alone): the painted pixels then take the class of the nearest kept pixel within `cap` pixels,
    `fill_nearest(out, hole=fill, cap=nearest, out=out)` -- two more launches.  EVERY pixel that holds `fill` is filled, also one that held it before the call:
    a caller who wants 255 kept as void paints with another byte (fill=254).  `fill` must be no class of the table (ValueError)."""
    if not isinstance(table, SegmentTable):
        raise RuntimeError(f"mmsa.evaluate: table takes an mmsa.evaluate.SegmentTable, got {type(table).__name__}")
    if not _is_int(fill, 0, 255):
        raise ValueError(f"mmsa.evaluate: fill = {fill!r}; a byte 0..255 is expected")
    nearest = _check_nearest(nearest, fill, table.num_classes, "mmsa.evaluate: select_segments")
    table._filled()
    pred = _check_map(pred, "pred", torch.uint8, "a uint8 class map", like=table.ids)
    B, H, W = (int(v) for v in pred.shape)
    capacity = int(table.records.shape[1])
    if (not isinstance(keep, torch.Tensor) or keep.dtype != torch.uint8 or tuple(keep.shape) != (B, capacity) or not keep.is_contiguous()
            or keep.device != pred.device):
        raise RuntimeError(f"mmsa.evaluate: keep must be a contiguous uint8 {(B, capacity)} tensor on {pred.device} (one byte per row of the table)")
    with torch.cuda.device(pred.device):
        if out is None:
            out = torch.empty_like(pred)
        else:
            _check_map(out, "out", torch.uint8, "a uint8 class map", like=pred)
        lib.call("mmsa_select_segments_u8", pred.data_ptr(), table.ids.data_ptr(), keep.data_ptr(), B, H, W, capacity, int(fill), out.data_ptr(), ops._stream())
        if nearest is not None:
            fill_nearest(out, hole=int(fill), cap=nearest, out=out)
    return out


# ---- segments tracked across frames: persistent ids by IoU match (csrc/track.hip) ----
TRACK_FIELDS = ("TRACK", "AGE", "PREV", "INTER")
TRACK, AGE, PREV, INTER = range(4)
TRACK_STATS = ("continued", "born", "ended")
TRACK_TRIP = 1024                  # csrc/track.hip TRACK_TRIP: the rows one trip of the assign scan takes
TRACK_DTYPE = np.dtype(SEGMENT_DTYPE.descr + [("track", np.int64), ("age", np.int64), ("prev", np.int64), ("iou", np.float64)])


def _check_ids(t, name, like=None):
    if not isinstance(t, torch.Tensor) or t.dtype != torch.int32 or t.dim() != 3 or not t.is_contiguous() or t.numel() == 0:
        raise RuntimeError(f"mmsa.evaluate: {name} must be a contiguous int32 [B, H, W] tensor (the ids of a SegmentTable)")
    if like is not None and (t.shape != like.shape or t.device != like.device):
        raise RuntimeError(f"mmsa.evaluate: {name} is {tuple(t.shape)} on {t.device}, ids_cur {tuple(like.shape)} on {like.device}")
    return t


@torch.no_grad()
def track_pairs(ids_cur, ids_prev, rows, capacity=None, table=None):
    """The intersections of the (current segment, previous segment) pairs of two ids maps, int32 [B, H, W] each (two launches: the table emptied, then a lane
    per pixel; mmsa_track_pairs) -> PairTable on the device.  Every pixel whose two ids lie in [0, rows) adds 1 to the pair of its image: key = ((b * rows + id_cur)
    << 31) | id_prev.  `capacity` / `table=` as in `segment_pairs`: a new table of the default capacity (the next power of two >= B * H * W / 2) whose
    overflow word starts at 0, or the caller's, emptied and filled, its overflow word ADDED to.  The table's shape is (B, 1, rows): `host()` then gives
    (image, current id, previous id, inter), sorted."""
    if capacity is not None:
        capacity = check_pair_capacity(capacity)
    ids_cur = _check_ids(ids_cur, "ids_cur")
    ids_prev = _check_ids(ids_prev, "ids_prev", ids_cur)
    B, H, W = (int(v) for v in ids_cur.shape)
    if not _is_int(rows, 1, (1 << 31) - 1):
        raise ValueError(f"mmsa.evaluate: rows = {rows!r}; the rows per image of the segment table (>= 1) are expected")
    _check_rows("mmsa.evaluate", B, int(rows), "rows")
    with torch.cuda.device(ids_cur.device):
        if table is None:
            table = PairTable.empty(default_pair_capacity(B * H * W) if capacity is None else capacity, ids_cur.device)
        else:
            if not isinstance(table, PairTable):
                raise RuntimeError(f"mmsa.evaluate: table= takes an mmsa.evaluate.PairTable, got {type(table).__name__}")
            table._check(ids_cur.device)
            if capacity is not None and capacity != table.capacity:
                raise RuntimeError(f"mmsa.evaluate: capacity={capacity} with a table of {table.capacity} slots")
        table.shape = (B, 1, int(rows))
        lib.call("mmsa_track_pairs", ids_cur.data_ptr(), ids_prev.data_ptr(), B, H, W, int(rows), table.keys.data_ptr(), table.counts.data_ptr(), table.capacity,
                 table.overflow.data_ptr(), ops._stream())
    return table


def _track_state(state, rows=None):
    s = np.asarray(state)
    if s.ndim < 2 or s.shape[-1] != len(TRACK_FIELDS) or s.dtype.kind not in "iu" or (rows is not None and s.shape[-2] != rows):
        raise ValueError(f"mmsa.evaluate: a tracker's state is an integer [..., rows, {len(TRACK_FIELDS)}] array ({', '.join(TRACK_FIELDS)}), got {s.dtype} {s.shape}")
    return s.astype(np.int64, copy=False)


def track_records_of(records, count, state, prev_area, scored=True, image=0):
    """The host reading of one image's rows: `segment_records_of(records, count)` with 'track', 'age', 'prev' (the predecessor's id in the previous frame, -1
    at birth) and 'iou' = INTER / (AREA + the predecessor's AREA - INTER) in float64 from those integers, NaN at birth.  state integer [rows, 4], prev_area
    integer [rows] as the tracker holds them for this image."""
    out_seg = segment_records_of(records, count, scored, image)
    s = _track_state(state, np.asarray(records).shape[0])
    pa = np.asarray(prev_area)
    if pa.shape != s.shape[:1] or pa.dtype.kind not in "iu":
        raise ValueError(f"mmsa.evaluate: prev_area is an integer [{s.shape[0]}] array (one previous area per row), got {pa.dtype} {pa.shape}")
    n = len(out_seg)
    s, pa = s[:n], pa[:n].astype(np.int64)
    out = np.zeros(n, dtype=TRACK_DTYPE)
    for name in SEGMENT_DTYPE.names:
        out[name] = out_seg[name]
    out["track"], out["age"], out["prev"] = s[:, TRACK], s[:, AGE], s[:, PREV]
    union = (out["area"] + pa - s[:, INTER]).astype(np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        out["iou"] = np.where(s[:, PREV] >= 0, s[:, INTER] / union, np.nan)
    return out


def track_summary_of(state, totals):
    """state integer [B, rows, 4] and totals integer [B, 3] -> dict(alive = the rows with a track, born / continued / ended = the totals over the images,
    mean_age = the mean AGE of the rows alive in float64, NaN without one)."""
    s = _track_state(state)
    t = np.asarray(totals)
    if t.shape[-1:] != (len(TRACK_STATS),) or t.dtype.kind not in "iu":
        raise ValueError(f"mmsa.evaluate: a tracker's totals are an integer [..., 3] array ({', '.join(TRACK_STATS)}), got {t.dtype} {t.shape}")
    t = t.astype(np.int64).reshape(-1, len(TRACK_STATS)).sum(0)
    live = s[..., TRACK] >= 0
    alive = int(live.sum())
    return dict(alive=alive, continued=int(t[0]), born=int(t[1]), ended=int(t[2]), mean_age=float(s[..., AGE][live].sum()) / alive if alive else float("nan"))


class SegmentTracker:
    """Follows the segments of one SegmentTable along a stream: image b of one `table.update()` follows image b of the one before.  `update()`, called after
    `table.update(...)`, matches the table's segments with those of the previous frame -- k continues j iff 3 * inter > AREA_k + AREA_j (IoU > 1/2, strict)
    and, with same_class=True, their classes agree; at most one partner on either side -- and fills `state` int32 [B, capacity, 4] = TRACK, AGE, PREV, INTER
    per row: the predecessor's track id and AGE + 1, or a NEW id `next_track[b]` + (the non-continuing rows before it) with AGE 1, PREV -1, INTER 0; the rows
    from min(count, capacity) on are (-1, 0, -1, 0).  `stats` int32 [B, 3] = continued, born, ended of the frame, ADDED to `totals` int64 [B, 3]
    (`mmsa.dist.allreduce_counts(tracker.totals)` sums them over ranks); `next_track` int32 [B]; tracks=True: `tracks` int32 [B, H, W], the track id of
    every pixel's segment, -1 elsewhere (an int32 map as `ids`: `run_lengths` takes it).  A segment whose id is beyond the table's rows takes part nowhere.
    The buffers are sized by the table's shape and capacity at the first update() and kept: a later update() allocates nothing and syncs nothing, and the
    previous frame lives at fixed addresses, so a captured table.update + tracker.update advances one frame per replay.  `pair_capacity` = the slots of the
    pair table (a power of two; None: `default_pair_capacity(B * H * W)`); the pixels of pairs that found no slot are ADDED to its overflow word, which
    `reset()` zeroes -- a tracker that overflowed once has lost matches, and `host` / `segments_info` / `summary` refuse to report from it.
    The device tensors speak of the table as the last tracker.update() saw it: read them before the table is filled again."""

    def __init__(self, table, same_class=True, pair_capacity=None, tracks=False):
        who = "mmsa.SegmentTracker"
        if not isinstance(table, SegmentTable):
            raise RuntimeError(f"{who}: table takes an mmsa.evaluate.SegmentTable, got {type(table).__name__}")
        for name, v in (("same_class", same_class), ("tracks", tracks)):
            if not isinstance(v, (bool, np.bool_)):
                raise ValueError(f"{who}: {name} = {v!r}; True or False is expected")
        self.table, self.same_class, self.with_tracks = table, bool(same_class), bool(tracks)
        self.pair_capacity = None if pair_capacity is None else check_pair_capacity(pair_capacity, who)
        self.shape = self.rows = None        # (B, H, W) and the rows per image the buffers were made for
        self.pairs = self.state = self.stats = self.totals = self.next_track = self.tracks = None
        self.prev_ids = self.prev_rows = self.prev_count = self.succ = self.prev_area = None

    def _make(self):
        t = self.table
        B, H, W = t.shape
        rows, device = int(t.records.shape[1]), t.ids.device
        if _capturing(device):
            raise RuntimeError("mmsa.SegmentTracker: the buffers cannot be allocated during a graph capture: run one update() before capturing")
        _check_library("segment tracker", TRACK_TRIP=lib.raw.mmsa_track_trip)
        i32 = dict(dtype=torch.int32, device=device)
        self.pairs = PairTable.empty(default_pair_capacity(B * H * W) if self.pair_capacity is None else self.pair_capacity, device)
        self.pairs.shape = (B, 1, rows)
        self.state = torch.tensor([-1, 0, -1, 0], **i32).repeat(B, rows, 1)
        self.stats, self.totals = torch.zeros(B, 3, **i32), torch.zeros(B, 3, dtype=torch.int64, device=device)
        self.next_track, self.prev_count = torch.zeros(B, **i32), torch.zeros(B, **i32)
        self.prev_ids, self.prev_rows = torch.full((B, H, W), -1, **i32), torch.zeros(B, rows, 4, **i32)
        self.succ, self.prev_area = torch.full((B, rows), -1, **i32), torch.zeros(B, rows, **i32)
        self.tracks = torch.full((B, H, W), -1, **i32) if self.with_tracks else None
        self.shape, self.rows = (B, H, W), rows

    @torch.no_grad()
    def update(self):
        """Associate the table's current frame with the previous one (six launches: mmsa_track_pairs, mmsa_track_update) -> self."""
        t = self.table
        t._filled()
        with torch.cuda.device(t.ids.device):
            if self.shape is None:
                self._make()
            if t.shape != self.shape or int(t.records.shape[1]) != self.rows or t.ids.device != self.state.device:
                raise RuntimeError(f"mmsa.SegmentTracker: the table holds a {t.shape} batch of {int(t.records.shape[1])} rows on {t.ids.device}, the tracker follows "
                                   f"{self.shape} of {self.rows} rows on {self.state.device}: a stream keeps its shape (make another tracker for another one)")
            B, H, W = self.shape
            p = self.pairs
            lib.call("mmsa_track_pairs", t.ids.data_ptr(), self.prev_ids.data_ptr(), B, H, W, self.rows, p.keys.data_ptr(), p.counts.data_ptr(), p.capacity,
                     p.overflow.data_ptr(), ops._stream())
            lib.call("mmsa_track_update", p.keys.data_ptr(), p.counts.data_ptr(), p.capacity, t.ids.data_ptr(), t.count.data_ptr(), t.records.data_ptr(), B, H, W,
                     self.rows, int(self.same_class), self.prev_ids.data_ptr(), self.prev_rows.data_ptr(), self.prev_count.data_ptr(), self.succ.data_ptr(),
                     self.prev_area.data_ptr(), self.state.data_ptr(), self.stats.data_ptr(), self.totals.data_ptr(), self.next_track.data_ptr(),
                     None if self.tracks is None else self.tracks.data_ptr(), ops._stream())
        return self

    @torch.no_grad()
    def reset(self, b=None):
        """Forget the previous frame of image b, or of every image (None): its next frame is a first frame -- everything is born, nothing ends -- and its
        track ids start at 0 again.  `totals` stay.  reset() of every image also zeroes the pair table's overflow word.  No host sync."""
        if self.shape is None:
            return self
        B = self.shape[0]
        if b is not None and not _is_int(b, 0, B - 1):
            raise ValueError(f"mmsa.SegmentTracker: b = {b!r}; an image index 0..{B - 1} (or None: every image) is expected")
        at = slice(None) if b is None else slice(int(b), int(b) + 1)
        self.prev_ids[at].fill_(-1)
        self.prev_count[at].zero_()
        self.next_track[at].zero_()
        if b is None:
            self.pairs.overflow.zero_()
        return self

    def _ready(self):
        if self.shape is None:
            raise RuntimeError("mmsa.SegmentTracker: nothing was tracked yet: call update()")

    def overflow(self):
        """The pixels of (current, previous) pairs that found no slot of the pair table since the last reset() (one device word; a host sync): 0, or the
        matches of some frame are incomplete."""
        self._ready()
        return int(self.pairs.overflow.item())

    def _complete(self):
        """-> count [B] on the host, after both overflow checks."""
        lost = self.overflow()
        if lost:
            raise RuntimeError(f"mmsa.SegmentTracker: the pair table of {self.pairs.capacity} slots overflowed ({lost} pixels of (current, previous) pairs were "
                               "dropped, so matches are missing): make the SegmentTracker with a larger pair_capacity= and reset()")
        count = self.table.count.cpu().numpy()
        for i in range(self.shape[0]):
            if count[i] > self.rows:
                raise _overflow_error("mmsa.SegmentTracker", i, int(count[i]), self.rows, "listed segments", "the records of the last", "make the SegmentTable")
        return count

    def host(self, b=None):
        """The tracked segments on the host (`track_records_of`) -> a numpy structured array with the fields of `SegmentTable.host` and 'track', 'age',
        'prev', 'iou'; of image `b`, or of every image in turn.  RuntimeError naming pair_capacity= where the pair table overflowed, naming the table's
        capacity= where an image has more segments than rows."""
        self._ready()
        B = self.shape[0]
        if b is not None and not _is_int(b, 0, B - 1):
            raise ValueError(f"mmsa.SegmentTracker: b = {b!r}; an image index 0..{B - 1} (or None: every image) is expected")
        count = self._complete()
        records, state, prev_area = self.table.records.cpu().numpy(), self.state.cpu().numpy(), self.prev_area.cpu().numpy()
        parts = [track_records_of(records[i], count[i], state[i], prev_area[i], self.table.scored, i) for i in (range(B) if b is None else [int(b)])]
        return parts[0] if len(parts) == 1 else np.concatenate(parts)

    def segments_info(self, b, masks=False):
        """`SegmentTable.segments_info(b, masks)` with 'track_id' and 'age' added to every dict."""
        rows = self.host(int(b))
        info = self.table.segments_info(int(b), masks=masks)
        for d, s in zip(info, rows):
            d["track_id"], d["age"] = int(s["track"]), int(s["age"])
        return info

    @torch.no_grad()
    def keep(self, min_age=None, max_age=None, tracks=None):
        """Which rows pass -> uint8 [B, capacity] on the device (1: keep), the format of `SegmentTable.keep`: min_age <= AGE < max_age and TRACK among
        `tracks` (a list of track ids).  Torch operations on `state`: no host sync.  Rows without a track are 0.  `table.keep(...) & tracker.keep(min_age=3)`
        through `select_segments` drops what has not persisted for three frames."""
        self._ready()
        age, track = self.state[..., AGE], self.state[..., TRACK]
        ok = track >= 0
        for name, v in (("min_age", min_age), ("max_age", max_age)):
            if v is not None and not _is_int(v, 1, (1 << 31) - 1):
                raise ValueError(f"mmsa.SegmentTracker: {name} = {v!r}; a number of frames >= 1 is expected")
        if min_age is not None:
            ok = ok & (age >= int(min_age))
        if max_age is not None:
            ok = ok & (age < int(max_age))
        if tracks is not None:
            ts = [tracks] if _is_int(tracks, 0, (1 << 31) - 1) else list(tracks)
            if not ts or any(not _is_int(v, 0, (1 << 31) - 1) for v in ts):
                raise ValueError(f"mmsa.SegmentTracker: tracks = {tracks!r}; a list of track ids >= 0 is expected")
            among = torch.zeros_like(ok)
            for v in sorted(set(int(v) for v in ts)):
                among = among | (track == v)
            ok = ok & among
        return ok.to(torch.uint8)

    def summary(self):
        """`track_summary_of` of the device tensors: tracks alive in the last frame, born / continued / ended over all frames and images, mean age."""
        self._ready()
        self._complete()
        return track_summary_of(self.state.cpu().numpy(), self.totals.cpu().numpy())


# ---- nearest-label fill: the holes of a map take the value of the nearest kept pixel (csrc/fill.hip) ----
FILL_SOURCE, FILL_HOLE, FILL_INERT = 0, 1, 2      # the roles of csrc/fill.hip's table
FILL_FAR = 65535                   # csrc/fill.hip FILL_FAR: the d2 of a hole that stays
_FILL_ROLES = {}                   # (roles, device) -> the device role table of a fill launch


def _fill_bytes(v, name):
    """A byte or a list of bytes -> the sorted tuple of them."""
    vs = (v,) if _is_int(v, 0, 255) else v
    if isinstance(vs, (str, bytes)) or not hasattr(vs, "__iter__"):
        raise ValueError(f"mmsa.evaluate: {name} = {v!r}; a byte 0..255 or a list of bytes is expected")
    vs = tuple(vs)
    if not all(_is_int(b, 0, 255) for b in vs):
        raise ValueError(f"mmsa.evaluate: {name} = {v!r}; a byte 0..255 or a list of bytes is expected")
    return tuple(sorted(set(int(b) for b in vs)))


def fill_roles(hole=255, inert=()):
    """The 256-byte role table of a fill launch, uint8 numpy [256]: 1 at the bytes of `hole` (to be filled), 2 at the bytes of `inert` (kept, offering nothing),
    0 at every other byte (a source: kept, and offered to the holes).  `hole` and `inert` are a byte or a list of bytes, disjoint, `hole` not empty."""
    holes, inerts = _fill_bytes(hole, "hole"), _fill_bytes(inert, "inert")
    if not holes:
        raise ValueError("mmsa.evaluate: hole is empty; at least one byte to fill is expected")
    both = sorted(set(holes) & set(inerts))
    if both:
        raise ValueError(f"mmsa.evaluate: hole and inert share the bytes {both}; a byte is filled or kept")
    roles = np.zeros(256, dtype=np.uint8)
    roles[list(holes)] = FILL_HOLE
    roles[list(inerts)] = FILL_INERT
    return roles


@torch.no_grad()
def fill_nearest(map, hole=255, inert=(), cap=32, out=None, d2=None, scratch=None):
    """The map with its holes filled from the nearest kept pixel (two launches, mmsa_fill_nearest_u8) -> uint8 [B, H, W] on the device.  A pixel whose byte is
    in `hole` takes the value of the nearest SOURCE pixel of its image within `cap` pixels (Euclidean, 1 <= cap <= 255), of equally near ones the topmost, then
    the leftmost; a hole with no source that near stays.  Every byte in neither list is a source; the bytes of `inert` (e.g. the 255 of an ignored region when
    the holes were painted with another byte) are kept and offer nothing -- they do not block either: the fill is Euclidean, not geodesic.  `hole` and `inert`
    are a byte or a list of bytes, disjoint.  Integers only: the same bytes on every run.
    `out=` (uint8, the map's shape) may be `map` itself (in place); `d2=` (uint16, the map's shape) receives 0 at every pixel that is no hole, the squared
    distance taken (1..cap^2) at a filled hole and FILL_FAR (65535) at a hole that stays; `scratch=` (a uint16 tensor of at least B * H * W elements, the row
    pass's plane, not `d2`) makes the call allocation-free -- without it the buffer of `boundary_distance`, cached per device and stream, is used."""
    roles = fill_roles(hole, inert)
    cap = check_distance_cap(cap)
    src = _check_map(map, "map", torch.uint8, "a uint8 class map", shape_only=True)
    B, H, W = (int(v) for v in src.shape)
    if B * H * W == 0:
        raise RuntimeError(f"mmsa.evaluate: an empty map {tuple(src.shape)}")
    if out is not None:
        _check_map(out, "out", torch.uint8, "a uint8 class map", like=src, shape_only=True)
    if d2 is not None:
        _check_map(d2, "d2", torch.uint16, "a uint16 distance map", like=src, shape_only=True)
    if scratch is not None:
        _check_scratch(scratch, torch.uint16, B * H * W)
        if scratch is d2:
            raise RuntimeError("mmsa.evaluate: scratch and d2 are two planes")
    _check_map(src, "map", torch.uint8, "a uint8 class map")
    with torch.cuda.device(src.device):
        if out is None:
            out = torch.empty_like(src)
        else:
            _check_map(out, "out", torch.uint8, "a uint8 class map", like=src)
        if d2 is not None:
            _check_map(d2, "d2", torch.uint16, "a uint16 distance map", like=src)
        if scratch is None:
            scratch = _row_plane(B * H * W, src.device)
        elif scratch.device != src.device:
            raise RuntimeError(f"mmsa.evaluate: scratch is on {scratch.device}, the map on {src.device}")
        if d2 is not None and scratch.data_ptr() == d2.data_ptr():
            raise RuntimeError("mmsa.evaluate: scratch and d2 are two planes")
        role = _table_on(_FILL_ROLES, roles, src.device, "the role table of the fill launch")
        lib.call("mmsa_fill_nearest_u8", src.data_ptr(), B, H, W, role.data_ptr(), int(np.flatnonzero(roles == FILL_HOLE)[0]), cap, scratch.data_ptr(),
                 out.data_ptr(), None if d2 is None else d2.data_ptr(), ops._stream())
    return out


def _check_nearest(nearest, fill, num_classes, who):
    """The nearest= keyword of the calls that paint `fill`: None, or the cap of the fill that follows; the painted byte must be no class."""
    if nearest is None:
        return None
    nearest = check_distance_cap(nearest, who)
    if num_classes is not None and int(fill) < int(num_classes):
        raise ValueError(f"{who}: fill = {fill} with nearest=: the byte is one of the {num_classes} classes, and a class byte would be a hole and a source at once; "
                         f"paint with a byte from {num_classes} on")
    return nearest


# ---- majority filter: every target pixel takes the most frequent class of its window (csrc/majority.hip) ----
MAJORITY_VOTER, MAJORITY_HOLE, MAJORITY_INERT = 0, 1, 2      # the roles of csrc/majority.hip's table
MAX_MAJORITY_RADIUS = 32           # csrc/majority.hip MAJ_MAX_RADIUS: a staged row of 64 + 2 r columns is two 64-bit masks
MAJORITY_WHERE = ("holes", "all")  # the library's all = 0, 1
_MAJORITY_ROLES = {}               # (roles, device) -> the device role table of a majority launch


def check_majority_radius(radius, who="mmsa.evaluate"):
    if not _is_int(radius, 1, MAX_MAJORITY_RADIUS):
        raise ValueError(f"{who}: radius = {radius!r}; an int in 1..{MAX_MAJORITY_RADIUS} is expected (the window is (2 r + 1) x (2 r + 1) pixels)")
    return int(radius)


def majority_roles(num_classes=None, hole=(), inert=None):
    """The 256-byte role table of a majority launch, uint8 numpy [256]: 1 at the bytes of `hole` (vote nothing, are rewritten), 2 at the bytes of `inert` (vote
    nothing, are kept), 0 at the voters.  With `num_classes=C` the voters are the bytes < C, and every byte >= C that is no hole is inert (the 255 of an
    uncovered or ignored pixel stays and votes nothing); without it every byte in neither list votes.  `hole` and `inert` are a byte or a list of bytes,
    disjoint, and no hole byte is a class."""
    holes, inerts = _fill_bytes(hole, "hole"), _fill_bytes(() if inert is None else inert, "inert")
    both = sorted(set(holes) & set(inerts))
    if both:
        raise ValueError(f"mmsa.evaluate: hole and inert share the bytes {both}; a byte is rewritten or kept")
    roles = np.zeros(256, dtype=np.uint8)
    if num_classes is not None:
        if not _is_int(num_classes, 1, 256):
            raise ValueError(f"mmsa.evaluate: num_classes = {num_classes!r}; a uint8 class map has 1..256 classes")
        low = [b for b in holes if b < int(num_classes)]
        if low:
            raise ValueError(f"mmsa.evaluate: hole holds the bytes {low}, which are among the {int(num_classes)} classes; a class byte votes, a hole byte "
                             f"does not: paint holes with a byte from {int(num_classes)} on")
        roles[int(num_classes):] = MAJORITY_INERT
    roles[list(holes)] = MAJORITY_HOLE
    roles[list(inerts)] = MAJORITY_INERT
    return roles


@torch.no_grad()
def majority_filter(map, radius=1, *, num_classes=None, hole=(), inert=None, where="all", half=False, out=None, support=None):
    """The majority (mode) filter of a class map (one launch, mmsa_majority_filter_u8) -> uint8 [B, H, W] on the device.  Every TARGET pixel takes the most
    frequent VOTER value of its (2 radius + 1)^2 window, 1 <= radius <= 32; the window is clipped at the image border (no padding), and images of a batch never
    see each other.  A tie never changes a pixel whose own value is among the tied; otherwise the smallest of the tied values wins.  Integers only: the same
    bytes on every run.
    Roles: with `num_classes=C` the bytes < C vote, and every byte >= C that is not in `hole` is inert -- it votes nothing and is never rewritten, so the 255
    of an uncovered or ignored pixel stays; without `num_classes` every byte in neither list votes, as in `fill_nearest`.  The bytes of `hole` vote nothing and
    are rewritten (a hole whose window holds no voter stays); `inert=` adds bytes that are kept.  `where="all"` rewrites voters and holes, `where="holes"` the
    holes alone (the other natural fill: by the vote of everything near, where `fill_nearest` takes the single nearest pixel).  `half=True`: a pixel changes only
    where one value holds MORE than half of the votes of its window.
        smooth = mmsa.majority_filter(pred, 2, num_classes=C)                                   # 5 x 5 mode filter; 255 stays void
        stable = mmsa.majority_filter(pred, 1, num_classes=C, half=True)                        # only where one class holds more than half of the votes
        closed = mmsa.majority_filter(mmsa.suppress_small(pred, 64, num_classes=C, fill=254), 3,
                                      num_classes=C, hole=254, where="holes")                   # specks take the vote of what surrounds them
    `out=` (uint8, the map's shape, NOT the map: a stencil cannot run in place); `support=` (uint16, the map's shape) receives the winning count n_best at
    every target pixel, whether or not `half` let it change, and 0 elsewhere.  The role table is uploaded once per (roles, device); with `out=` (and
    `support=`) a later call allocates nothing and can be captured in a graph."""
    radius = check_majority_radius(radius)
    roles = majority_roles(num_classes, hole, inert)
    if where not in MAJORITY_WHERE:
        raise ValueError(f"mmsa.evaluate: where = {where!r}; \"all\" (voters and holes are rewritten) or \"holes\" is expected")
    if where == "holes" and not (roles == MAJORITY_HOLE).any():
        raise ValueError("mmsa.evaluate: where = \"holes\" and hole is empty; at least one byte to rewrite is expected")
    if not isinstance(half, (bool, np.bool_)):
        raise ValueError(f"mmsa.evaluate: half = {half!r}; True or False is expected")
    src = _check_map(map, "map", torch.uint8, "a uint8 class map", shape_only=True)
    B, H, W = (int(v) for v in src.shape)
    if B * H * W == 0:
        raise RuntimeError(f"mmsa.evaluate: an empty map {tuple(src.shape)}")
    if out is not None:
        _check_map(out, "out", torch.uint8, "a uint8 class map", like=src, shape_only=True)
        if out is map:
            raise RuntimeError("mmsa.evaluate: out is the map; a stencil cannot run in place")
    if support is not None:
        _check_map(support, "support", torch.uint16, "a uint16 count map", like=src, shape_only=True)
    _check_map(src, "map", torch.uint8, "a uint8 class map")
    with torch.cuda.device(src.device):
        if out is None:
            out = torch.empty_like(src)
        else:
            _check_map(out, "out", torch.uint8, "a uint8 class map", like=src)
            if out.data_ptr() == src.data_ptr():
                raise RuntimeError("mmsa.evaluate: out is the map; a stencil cannot run in place")
        if support is not None:
            _check_map(support, "support", torch.uint16, "a uint16 count map", like=src)
            if support.data_ptr() in (src.data_ptr(), out.data_ptr()):
                raise RuntimeError("mmsa.evaluate: support aliases a map; it is a plane of its own")
        role = _table_on(_MAJORITY_ROLES, roles, src.device, "the role table of the majority launch")
        lib.call("mmsa_majority_filter_u8", src.data_ptr(), B, H, W, role.data_ptr(), radius, MAJORITY_WHERE.index(where), int(bool(half)), out.data_ptr(),
                 None if support is None else support.data_ptr(), ops._stream())
    return out


# ---- guided vote filter: the majority filter with every vote weighted by the guide frame and by the voter's confidence (csrc/vote.hip) ----
MAX_VOTE_RADIUS = 16               # csrc/vote.hip VOTE_MAX_RADIUS: a lane walks every tap of the window
MAX_RANGE_WEIGHT = 4096            # the largest entry of a range table: 4096 * 255 per tap, 33^2 taps, stays below 2^31
_VOTE_TABLES = {}                  # (bytes, device) -> the device role table or range table of a vote launch


def vote_range_table(sigma, channels=3):
    """The Gaussian range table of `vote_filter`, uint16 numpy [255 * channels + 1]: entry d = floor(256 * exp(-d^2 / (2 sigma^2)) + 0.5), formed in float64
    on the host; d is the L1 distance of two guide pixels.  Entry 0 is 256, and the table never rises."""
    if isinstance(sigma, bool) or not isinstance(sigma, (int, float, np.integer, np.floating)) or not (float(sigma) > 0 and math.isfinite(float(sigma))):
        raise ValueError(f"mmsa.evaluate: sigma = {sigma!r}; a finite float > 0 is expected (in units of the guide's L1 difference)")
    if not _is_int(channels, 1, 3) or int(channels) == 2:
        raise ValueError(f"mmsa.evaluate: channels = {channels!r}; a guide has 1 or 3 channels")
    d = np.arange(255 * int(channels) + 1, dtype=np.float64)
    return np.floor(256.0 * np.exp(-(d * d) / (2.0 * float(sigma) * float(sigma))) + 0.5).astype(np.uint16)


def _check_range_weights(table, channels):
    """range_weights= -> uint16 numpy [255 * channels + 1] with every entry in 0 .. 4096."""
    try:
        t = np.asarray(table.cpu() if isinstance(table, torch.Tensor) else table)
    except Exception:
        t = None
    n = 255 * channels + 1
    if t is None or t.dtype == object or t.dtype.kind not in "iuf" or t.ndim != 1:
        raise ValueError(f"mmsa.evaluate: range_weights must be a one-dimensional array of {n} integers in 0..{MAX_RANGE_WEIGHT}")
    if t.shape[0] != n:
        raise ValueError(f"mmsa.evaluate: range_weights has {t.shape[0]} entries; a guide of {channels} channel{'s' if channels > 1 else ''} has L1 differences "
                         f"0..{n - 1}, so {n} are expected")
    if t.dtype.kind == "f" and not (np.isfinite(t).all() and (t == np.floor(t)).all()):
        raise ValueError("mmsa.evaluate: range_weights holds values that are not integers")
    if (t < 0).any() or (t > MAX_RANGE_WEIGHT).any():
        raise ValueError(f"mmsa.evaluate: range_weights holds values outside 0..{MAX_RANGE_WEIGHT} (a tap's vote must stay below 2^20)")
    return np.ascontiguousarray(t.astype(np.uint16))


@torch.no_grad()
def vote_filter(map, radius=2, *, guide=None, sigma=None, range_weights=None, weights=None, num_classes=None, hole=(), inert=None, where="all", half=False,
                out=None, support=None):
    """The guided vote filter of a class map (one launch, mmsa_vote_filter_u8) -> uint8 [B, H, W] on the device: the joint-bilateral weighted mode filter.
    Roles (`num_classes`, `hole`, `inert`), the clipped (2 radius + 1)^2 window, `where`, `half` and the tie rule are `majority_filter`'s, 1 <= radius <= 16;
    every voter q of the window of p votes for its value with lut[d(p, q)] * wq(q), and the value with the largest SUM wins.
    `guide`: the raw uint8 frame, [B, Hg, Wg, 3], [B, Hg, Wg, 1] or [B, Hg, Wg], Hg >= H, Wg >= W (the top-left H x W is used: a padded frame needs no copy);
    d is the L1 difference of two guide pixels, and lut comes from `sigma=` (`vote_range_table`: 256 exp(-d^2 / (2 sigma^2)), rounded) or from
    `range_weights=` (255 G + 1 integers in 0..4096) -- exactly one of them with a guide, neither without.  `weights`: float32 [B, H, W], a confidence, margin
    or probability map; wq = min(255, int(clamp(w, 0, 1) * 256)), so NaN, negatives and anything below 1 / 256 vote nothing.  Integers only: the same bytes on
    every run.  With neither `guide` nor `weights` the result is `majority_filter`'s.
        snapped = mmsa.vote_filter(pred, 8, guide=rgb, sigma=8, num_classes=C)                               # contours move to the RGB frame's edges
        crossed = mmsa.vote_filter(pred, 4, guide=aux, sigma=6, weights=conf, num_classes=C)                 # guided by the aux frame, confident pixels count more
        closed = mmsa.vote_filter(mmsa.suppress_small(pred, 64, num_classes=C, fill=254), 3, guide=rgb, sigma=8,
                                  num_classes=C, hole=254, where="holes")                                    # specks take the weighted vote around them
    `out=` (uint8, the map's shape, NOT the map); `support=` (uint32, the map's shape) receives the winning sum S_best at every target pixel and 0 elsewhere.
    A pixel whose window holds no vote (zero weights, zeros in the table) stays.  The role and range tables are uploaded once per (content, device); with
    `out=` (and `support=`) a later call allocates nothing and can be captured in a graph."""
    if not _is_int(radius, 1, MAX_VOTE_RADIUS):
        raise ValueError(f"mmsa.evaluate: radius = {radius!r}; an int in 1..{MAX_VOTE_RADIUS} is expected (the window is (2 r + 1) x (2 r + 1) pixels)")
    radius = int(radius)
    roles = majority_roles(num_classes, hole, inert)
    if where not in MAJORITY_WHERE:
        raise ValueError(f"mmsa.evaluate: where = {where!r}; \"all\" (voters and holes are rewritten) or \"holes\" is expected")
    if where == "holes" and not (roles == MAJORITY_HOLE).any():
        raise ValueError("mmsa.evaluate: where = \"holes\" and hole is empty; at least one byte to rewrite is expected")
    if not isinstance(half, (bool, np.bool_)):
        raise ValueError(f"mmsa.evaluate: half = {half!r}; True or False is expected")
    src = _check_map(map, "map", torch.uint8, "a uint8 class map", shape_only=True)
    B, H, W = (int(v) for v in src.shape)
    if B * H * W == 0:
        raise RuntimeError(f"mmsa.evaluate: an empty map {tuple(src.shape)}")
    G, Hg, Wg, table = 0, 0, 0, None
    if guide is None:
        if sigma is not None or range_weights is not None:
            raise ValueError("mmsa.evaluate: sigma= and range_weights= weigh the differences of a guide; without guide= neither is taken")
    else:
        if (sigma is None) == (range_weights is None):
            raise ValueError("mmsa.evaluate: a guide takes sigma= (the Gaussian table) or range_weights= (a table of your own), exactly one of them")
        if not isinstance(guide, torch.Tensor):
            raise RuntimeError(f"mmsa.evaluate: guide must be a tensor, got {type(guide).__name__}")
        if guide.dtype != torch.uint8:
            raise RuntimeError(f"mmsa.evaluate: guide is {guide.dtype}; the raw uint8 frame is expected")
        if guide.dim() not in (3, 4) or not guide.is_contiguous() or (guide.dim() == 4 and int(guide.shape[3]) not in (1, 3)):
            raise RuntimeError(f"mmsa.evaluate: guide must be a contiguous [B, Hg, Wg, 3], [B, Hg, Wg, 1] or [B, Hg, Wg] tensor, got {tuple(guide.shape)}")
        G, Hg, Wg = (int(guide.shape[3]) if guide.dim() == 4 else 1), int(guide.shape[1]), int(guide.shape[2])
        if int(guide.shape[0]) != B or Hg < H or Wg < W:
            raise RuntimeError(f"mmsa.evaluate: guide has shape {tuple(guide.shape)}, the map is [B, H, W] = {tuple(src.shape)}; as many frames of at least that "
                               "size are expected (the map is the frame's top-left corner)")
        table = vote_range_table(sigma, G) if sigma is not None else _check_range_weights(range_weights, G)
    if weights is not None:
        _check_map(weights, "weights", torch.float32, "a float32 confidence map", like=src, shape_only=True)
    if out is not None:
        _check_map(out, "out", torch.uint8, "a uint8 class map", like=src, shape_only=True)
        if out is map:
            raise RuntimeError("mmsa.evaluate: out is the map; a stencil cannot run in place")
    if support is not None:
        _check_map(support, "support", torch.uint32, "a uint32 sum map", like=src, shape_only=True)
    _check_map(src, "map", torch.uint8, "a uint8 class map")
    with torch.cuda.device(src.device):
        if guide is not None:
            if not guide.is_cuda or guide.device != src.device:
                raise RuntimeError(f"mmsa.evaluate: guide is on {guide.device}, the map on {src.device}")
        if weights is not None:
            _check_map(weights, "weights", torch.float32, "a float32 confidence map", like=src)
        if out is None:
            out = torch.empty_like(src)
        else:
            _check_map(out, "out", torch.uint8, "a uint8 class map", like=src)
            if out.data_ptr() == src.data_ptr():
                raise RuntimeError("mmsa.evaluate: out is the map; a stencil cannot run in place")
        if support is not None:
            _check_map(support, "support", torch.uint32, "a uint32 sum map", like=src)
            if support.data_ptr() in (src.data_ptr(), out.data_ptr()):
                raise RuntimeError("mmsa.evaluate: support aliases a map; it is a plane of its own")
        inputs = [t.data_ptr() for t in (guide, weights) if t is not None]
        if out.data_ptr() in inputs or (support is not None and support.data_ptr() in inputs):
            raise RuntimeError("mmsa.evaluate: out or support aliases the guide or the weights; they are planes of their own")
        role = _table_on(_VOTE_TABLES, roles, src.device, "the role table of the vote launch")
        lut = None if table is None else _table_on(_VOTE_TABLES, table, src.device, "the range table of the vote launch")
        lib.call("mmsa_vote_filter_u8", src.data_ptr(), B, H, W, role.data_ptr(), radius, MAJORITY_WHERE.index(where), int(bool(half)),
                 None if guide is None else guide.data_ptr(), Hg, Wg, G, None if lut is None else lut.data_ptr(),
                 None if weights is None else weights.data_ptr(), out.data_ptr(), None if support is None else support.data_ptr(), ops._stream())
    return out


# ---- run-length tables: the runs of a class map or an ids map, and the COCO RLE of one id (csrc/runs.hip) ----
# Of image b of a map m [B, H, W], flat_b = m[b].ravel() (order "row") or m[b].T.ravel() (order "column": the order of COCO's mask RLE).  A HEAD is index 0 and
# every i > 0 with flat_b[i] != flat_b[i - 1]: runs continue across line ends, and a map of one value is ONE run.  count[b] = the heads, also beyond capacity;
# starts[b, j] / values[b, j] = the flat index of the j-th head in ascending order and flat_b there, for j < min(count[b], capacity); the rows behind them are
# not written.  length[j] = (starts[j + 1] or H * W) - starts[j].
RUNS_BLOCK = 2048                  # csrc/runs.hip RUNS_BLOCK: the flat indices per scan unit (one scratch word each)
RUNS_TILE = 64                     # csrc/runs.hip RUNS_TILE: the tile edge of the transpose the column order starts with
RUN_ORDERS = ("row", "column")     # the library's order 0, 1
MIN_RUN_CAPACITY = 4096


def default_run_capacity(H, W):
    """The default runs per image of a run table: max(4096, H * W // 8)."""
    return max(MIN_RUN_CAPACITY, int(H) * int(W) // 8)


def check_run_capacity(capacity, who="mmsa.evaluate"):
    if not _is_int(capacity, 1, (1 << 31) - 1):
        raise ValueError(f"{who}: capacity = {capacity!r}; a positive number of runs per image is expected (None: max({MIN_RUN_CAPACITY}, H * W // 8))")
    return int(capacity)


def check_run_order(order, who="mmsa.evaluate"):
    if order not in RUN_ORDERS:
        raise ValueError(f"{who}: order = {order!r}; 'row' (row-major runs) or 'column' (column-major runs: COCO's mask order) is expected")
    return order


def run_units(H, W):
    """The scan units of one image, a scratch word each: ceil(H * W / RUNS_BLOCK)."""
    return -(-int(H) * int(W) // RUNS_BLOCK)


def run_scratch_words(B, H, W, order, itemsize=4):
    """The int32 words of a launch's scratch: the unit counts of every image, and for "column" the transposed map (of `itemsize` bytes per pixel) behind them."""
    if "run-length" not in _library_checked:      # every run_lengths() call comes through here
        block = lib.raw.mmsa_run_lengths_block
        _check_library("run-length", RUNS_BLOCK=lambda: block(0), RUNS_TILE=lambda: block(1), SCAN_LANES=lambda: block(2), SCAN_TRIP=lambda: block(3))
    return B * run_units(H, W) + (-(-B * int(H) * int(W) * itemsize // 4) if check_run_order(order) == "column" else 0)


class RunTable:
    """A run table on the device: `count` int32 [B] (the runs of every image, also beyond capacity), `starts` and `values` int32 [B, capacity] (the flat index
    and the value of the first min(count, capacity) runs, in ascending order), the `order` ("row" or "column") the maps were flattened in, `shape` = (B, H, W) of
    the maps, and `scratch` (int32, `run_scratch_words`: the launch's own -- the unit counts of the prefix sum and, for "column", the transposed map)."""

    def __init__(self, count, starts, values, order, shape, capacity, scratch=None):
        self.count, self.starts, self.values, self.scratch = count, starts, values, scratch
        self.order = check_run_order(order, "mmsa.RunTable")
        self.shape = None if shape is None else tuple(int(v) for v in shape)
        self.capacity = check_run_capacity(capacity, "mmsa.RunTable")

    @classmethod
    def empty(cls, B, H, W, order, capacity, device):
        """The buffers of a batch of B maps of H x W pixels, uint8 or int32: nothing a later run_lengths(..., table=) of this shape has to allocate."""
        capacity = check_run_capacity(capacity, "mmsa.RunTable")
        _check_rows("mmsa.RunTable", B, capacity, "runs")
        return cls(torch.zeros(B, dtype=torch.int32, device=device), torch.empty(B, capacity, dtype=torch.int32, device=device),
                   torch.empty(B, capacity, dtype=torch.int32, device=device), order, (B, H, W), capacity,
                   torch.empty(run_scratch_words(B, H, W, order), dtype=torch.int32, device=device))

    def _check(self, B, device):
        ok = all(isinstance(t, torch.Tensor) and t.dtype == torch.int32 and t.is_contiguous() and t.device == device for t in (self.count, self.starts, self.values))
        if not ok or tuple(self.count.shape) != (B,) or tuple(self.starts.shape) != (B, self.capacity) or tuple(self.values.shape) != (B, self.capacity):
            raise RuntimeError(f"mmsa.evaluate: a RunTable of {B} images holds contiguous int32 count [{B}], starts and values [{B}, {self.capacity}] on {device}")
        return self

    def overflow(self):
        """Whether an image has more runs than rows (the device words of `count`): its last runs were dropped."""
        return bool((self.count > self.capacity).any().item())

    def host(self, b):
        """The runs of image b on the host -> int64 numpy (starts, lengths, values).  RuntimeError naming capacity= where the image has more runs than rows."""
        B, H, W = self.shape
        if not _is_int(b, 0, B - 1):
            raise ValueError(f"mmsa.RunTable: b = {b!r}; an image index 0..{B - 1} is expected")
        n = int(self.count[int(b)].item())
        if n > self.capacity:
            raise _overflow_error("mmsa.RunTable", int(b), n, self.capacity, "runs", "the last", "fill a table")
        starts = self.starts[int(b), :n].cpu().numpy().astype(np.int64)
        values = self.values[int(b), :n].cpu().numpy().astype(np.int64)
        return starts, np.diff(starts, append=H * W), values


def _check_run_map(map):
    if not isinstance(map, torch.Tensor) or map.dtype not in (torch.uint8, torch.int32):
        raise RuntimeError(f"mmsa.evaluate: map must be a uint8 (class map) or int32 (ids) tensor, got {map.dtype if isinstance(map, torch.Tensor) else type(map).__name__}")
    return _check_map(map, "map", map.dtype, "a uint8 or int32 map")


@torch.no_grad()
def run_lengths(map, order=None, capacity=None, table=None):
    """The runs of a uint8 class map or an int32 ids map [B, H, W] (mmsa_run_lengths_u8 / _i32: three launches, and for "column" a transpose into the table's
    scratch before them; no host sync) -> RunTable.  `order` = "column" (None: the default; COCO's mask order) or "row"; `capacity` = the rows per image (None: max(4096, H * W // 8); any positive number).  `table=` (a RunTable
    of B images: its own order and capacity hold, and one spelled out here must agree) is filled instead: nothing is allocated where its scratch holds
    `run_scratch_words` of this shape (RunTable.empty sizes it so), so the call can be captured.  Nothing is read back: look at `table.overflow()`, or call
    `table.host(b)`, which raises where runs were dropped."""
    if order is not None:
        check_run_order(order)
    if capacity is not None:
        capacity = check_run_capacity(capacity)
    if table is not None and not isinstance(table, RunTable):
        raise RuntimeError(f"mmsa.evaluate: table= takes an mmsa.evaluate.RunTable, got {type(table).__name__}")
    src = _check_run_map(map)
    B, H, W = (int(v) for v in src.shape)
    if B * H * W == 0:
        raise RuntimeError(f"mmsa.evaluate: an empty map {tuple(src.shape)}")
    if B * H * W >= 1 << 31:
        raise RuntimeError(f"mmsa.evaluate: {B} x {H} x {W} pixels; a run table indexes a batch in 32 bits (B * H * W < 2^31)")
    with torch.cuda.device(src.device):
        if table is None:
            table = RunTable.empty(B, H, W, order or "column", default_run_capacity(H, W) if capacity is None else capacity, src.device)
        else:
            table._check(B, src.device)
            for name, v, own in (("order", order, table.order), ("capacity", capacity, table.capacity)):
                if v is not None and v != own:
                    raise RuntimeError(f"mmsa.evaluate: {name}={v!r} with a table made with {name}={own!r}")
        words = run_scratch_words(B, H, W, table.order, src.element_size())
        s = table.scratch
        if not (isinstance(s, torch.Tensor) and s.dtype == torch.int32 and s.is_contiguous() and s.device == src.device and s.numel() >= words):
            if _capturing(src.device):
                raise RuntimeError(f"mmsa.evaluate: the scratch of a {B} x {H} x {W} run table cannot be allocated during a graph capture: make the table with "
                                   "RunTable.empty of this shape, or run one call of this shape before capturing")
            table.scratch = torch.empty(words, dtype=torch.int32, device=src.device)
        table.shape = (B, H, W)
        lib.call("mmsa_run_lengths_u8" if src.dtype == torch.uint8 else "mmsa_run_lengths_i32", src.data_ptr(), B, H, W, RUN_ORDERS.index(table.order),
                 table.capacity, table.count.data_ptr(), table.starts.data_ptr(), table.values.data_ptr(), table.scratch.data_ptr(), ops._stream())
    return table


@torch.no_grad()
def run_decode(table, fill=-1, out=None):
    """The map of a run table (one launch, mmsa_run_decode_i32: a lane per pixel and a binary search over the starts) -> int32 [B, H, W]: the value of the run
    the pixel lies in; `fill` where the image has no run.  Of an overflowed table the last kept run has no row behind it that ends it: its head pixel gets its
    value and every pixel past that head `fill`."""
    if not isinstance(table, RunTable):
        raise RuntimeError(f"mmsa.evaluate: table takes an mmsa.evaluate.RunTable, got {type(table).__name__}")
    if table.shape is None:
        raise RuntimeError("mmsa.evaluate: a RunTable without its maps' shape= (B, H, W) cannot be decoded")
    if not _is_int(fill, -(1 << 31), (1 << 31) - 1):
        raise ValueError(f"mmsa.evaluate: fill = {fill!r}; an int32 value is expected")
    B, H, W = table.shape
    device = table.count.device
    table._check(B, device)
    with torch.cuda.device(device):
        if out is None:
            out = torch.empty(B, H, W, dtype=torch.int32, device=device)
        else:
            _check_int_plane(out, "out", (B, H, W), device, "the decoded map")
        lib.call("mmsa_run_decode_i32", table.count.data_ptr(), table.starts.data_ptr(), table.values.data_ptr(), B, H, W, RUN_ORDERS.index(table.order),
                 table.capacity, int(fill), out.data_ptr(), ops._stream())
    return out


def _runs3(starts, lengths, values):
    s, l, v = (np.asarray(a) for a in (starts, lengths, values))
    if any(a.ndim != 1 or a.dtype.kind not in "iu" for a in (s, l, v)) or not len(s) == len(l) == len(v):
        raise ValueError("mmsa.evaluate: runs are three integer arrays of one length (starts, lengths, values): RunTable.host(b)")
    return s.astype(np.int64), l.astype(np.int64), v.astype(np.int64)


def runs_of_value(starts, lengths, values, v):
    """The runs of one id or class among the runs of `RunTable.host(b)` -> (starts, lengths) of those with value v, in ascending order."""
    s, l, vals = _runs3(starts, lengths, values)
    at = vals == int(v)
    return s[at], l[at]


def _rle_counts(s, l, n):
    """Ascending, non-adjacent runs (start, length) of the ones of a mask of n pixels -> COCO's counts: zeros first, no trailing zero-length entry."""
    ends = s + l
    counts = np.stack([s - np.concatenate([[0], ends[:-1]]), l], 1).ravel().tolist()
    last = int(ends[-1]) if len(ends) else 0
    return counts + [n - last] if last < n else counts


def coco_rle_of(starts, lengths, values, v, H, W, order="column"):
    """The uncompressed COCO RLE of the mask `map == v` from the runs of a COLUMN-order table (`RunTable.host(b)`) -> {"size": [H, W], "counts": [...]}: the
    run lengths of the column-major mask, alternating and starting with the zeros (a leading 0 where the mask holds pixel 0), without a trailing zero-length
    entry.  Two runs of v are never adjacent in a table (the second would be no head), so no count in the middle is 0.  `order` = the table's: "row" raises
    ValueError."""
    if check_run_order(order) != "column":
        raise ValueError("mmsa.evaluate: COCO's RLE is the column-major mask: it takes the runs of a table made with order='column', this one is order='row'")
    s, l, vals = _runs3(starts, lengths, values)
    n = int(H) * int(W)
    if len(s) == 0 or s[0] != 0 or s[-1] + l[-1] != n or (l <= 0).any():
        raise ValueError(f"mmsa.evaluate: the runs do not cover the {H} x {W} = {n} pixels of the map from index 0")
    at = vals == int(v)
    return {"size": [int(H), int(W)], "counts": _rle_counts(s[at], l[at], n)}


def rle_area_of(rle):
    """The pixels of an uncompressed COCO RLE (pycocotools' `area`, in integers): the sum of the one-runs."""
    return int(sum(rle["counts"][1::2]))


def rle_bbox_of(rle):
    """The box [x, y, width, height] of an uncompressed COCO RLE (pycocotools' `toBbox`, in integers); [0, 0, 0, 0] for an empty mask.  A one-run that
    crosses a column end spans every row."""
    H = int(rle["size"][0])
    c = np.asarray(rle["counts"], dtype=np.int64)
    ends = np.cumsum(c)
    a, e = (ends - c)[1::2], ends[1::2] - 1            # the first and the last pixel of every one-run
    keep = e >= a
    a, e = a[keep], e[keep]
    if len(a) == 0:
        return [0, 0, 0, 0]
    xa, xe = a // H, e // H
    wraps = bool((xa != xe).any())
    x0, x1 = int(xa.min()), int(xe.max())
    y0, y1 = (0, H - 1) if wraps else (int((a % H).min()), int((e % H).max()))
    return [x0, y0, x1 - x0 + 1, y1 - y0 + 1]
