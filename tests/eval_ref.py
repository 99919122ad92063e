"""numpy restatement of the reference's evaluation of a class map, written from segmentation/mmseg_custom/apis/evaluation/metrics_micro.py
(`intersect_and_union` 26-86, `total_area_to_metrics` 451-526), datasets/DELIVER.py (`pre_eval` 219-259, the ground-truth path 194-205, the summary of
`evaluate` 327-367) and datasets/pipelines/transform.py (`Resize_multimodal._resize_seg` 1169-1188) -- stated, not copied:

  labels   every `label_map` entry in dict order, `label[label == old] = new` on the uint8 map (a later entry sees what an earlier one wrote);
           reduce_zero_label: 0 -> 255, then minus 1 in uint8 (wraps), then 254 -> 255; mask = label != ignore_index; both maps are masked.
  areas    three torch.histc(bins=C, min=0, max=C-1) calls, on pred[pred == label], on pred and on label: integer data, so bin k counts the value k,
           and values outside [0, C - 1] are dropped -- from THAT histogram only.  area_union = area_pred_label + area_label - area_intersect.
  resize   mmcv.imrescale (keep_ratio: the largest size inside (long edge, short edge), int(x * f + 0.5)) / mmcv.imresize with interpolation='nearest'
           = cv2.resize(INTER_NEAREST): per axis src = min(floor(d * (1.0 / (double(n_dst) / n_src))), n_src - 1), as OpenCV's resize.cpp states it.
  metrics  aAcc = sum(intersect) / sum(label); IoU = intersect / union; Acc = Recall = intersect / label; Dice = 2 intersect / (pred + label);
           Precision = intersect / pred; Fscore = (1 + beta^2) P R / (beta^2 P + R); 0 / 0 = NaN, replaced by np.nan_to_num when nan_to_num is given.
           Float64 here; the reference divides float32 tensors.

The checker of tests/test_evaluate_gpu.py (bit-exact counts) and tests/test_evaluate_cpu.py, where tests/golden/eval_counts.npz pins it against the
imported reference.  OpenCV is not involved here (it is not installed where this is built): the nearest rule is pinned against this file only."""
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))


def load_golden():
    return np.load(os.path.join(HERE, "golden", "eval_counts.npz"))


def transform_bytes(ignore_index=255, label_map=None, reduce_zero_label=False):
    """(transformed byte uint8 [256], kept bool [256]) for every raw label byte."""
    out = np.empty(256, dtype=np.uint8)
    for v in range(256):
        x = v
        for old, new in (label_map or {}).items():
            if x == old:
                x = new
        if reduce_zero_label:
            if x == 0:
                x = 255
            x = (x - 1) % 256
            if x == 254:
                x = 255
        out[v] = x
    return out, out.astype(np.int64) != ignore_index


def lut(num_classes, ignore_index=255, label_map=None, reduce_zero_label=False):
    """The device LUT's contract: class, num_classes (kept, out of range) or 255 (ignored)."""
    t, keep = transform_bytes(ignore_index, label_map, reduce_zero_label)
    return np.where(keep, np.minimum(t, num_classes), 255).astype(np.uint8)


def transform_labels(label, ignore_index=255, label_map=None, reduce_zero_label=False):
    t, keep = transform_bytes(ignore_index, label_map, reduce_zero_label)
    return t[label], keep[label]


def intersect_and_union(pred, label, num_classes, ignore_index=255, label_map=None, reduce_zero_label=False):
    """One image -> (area_intersect, area_union, area_pred_label, area_label), int64 [num_classes]."""
    lab, keep = transform_labels(label, ignore_index, label_map, reduce_zero_label)
    p, l = pred[keep].astype(np.int64), lab[keep].astype(np.int64)

    def hist(v):
        return np.bincount(v[v < num_classes], minlength=num_classes).astype(np.int64)
    ai, ap, al = hist(p[p == l]), hist(p), hist(l)
    return ai, ap + al - ai, ap, al


def confusion(pred, label, num_classes, ignore_index=255, label_map=None, reduce_zero_label=False):
    """One image -> int64 [C + 1, C + 1]: [label class, predicted class], index C = outside [0, C) and not ignored."""
    C = num_classes
    lab, keep = transform_labels(label, ignore_index, label_map, reduce_zero_label)
    p, l = np.minimum(pred[keep].astype(np.int64), C), np.minimum(lab[keep].astype(np.int64), C)
    return np.bincount(l * (C + 1) + p, minlength=(C + 1) ** 2).reshape(C + 1, C + 1).astype(np.int64)


def areas_of(conf):
    """The four histograms from a confusion matrix (the layout's contract)."""
    C = conf.shape[-1] - 1
    ai = np.array([conf[..., k, k] for k in range(C)]).T if conf.ndim > 2 else np.array([conf[k, k] for k in range(C)])
    ap, al = conf.sum(-2)[..., :C], conf.sum(-1)[..., :C]
    return ai, ap + al - ai, ap, al


def nearest_index(n_src, n_dst):
    inv = np.float64(n_dst) / np.float64(n_src)
    ifx = np.float64(1.0) / inv
    return np.array([min(int(np.floor(d * ifx)), n_src - 1) for d in range(n_dst)], dtype=np.int32)


def new_size(Hl, Wl, scale, keep_ratio):
    if not keep_ratio:
        return int(scale[1]), int(scale[0])
    f = min(max(scale) / max(Hl, Wl), min(scale) / min(Hl, Wl))
    return int(Hl * float(f) + 0.5), int(Wl * float(f) + 0.5)


def resize_nearest(label, H, W):
    """[..., Hl, Wl] -> [..., H, W]."""
    ys, xs = nearest_index(label.shape[-2], H), nearest_index(label.shape[-1], W)
    return label[..., ys[:, None], xs[None, :]]


def total_area_to_metrics(ai, au, ap, al, metrics=("mIoU",), nan_to_num=None, beta=1):
    ai, au, ap, al = (np.asarray(a, dtype=np.float64) for a in (ai, au, ap, al))
    out = {}
    with np.errstate(divide="ignore", invalid="ignore"):
        out["aAcc"] = ai.sum() / al.sum()
        for m in metrics:
            if m == "mIoU":
                out["IoU"], out["Acc"] = ai / au, ai / al
            elif m == "mDice":
                out["Dice"], out["Acc"] = 2 * ai / (ap + al), ai / al
            elif m == "mFscore":
                P, R = ai / ap, ai / al
                out["Fscore"], out["Precision"], out["Recall"] = (1 + beta ** 2) * (P * R) / (beta ** 2 * P + R), P, R
    if nan_to_num is not None:
        out = {k: np.nan_to_num(v, nan=nan_to_num) for k, v in out.items()}
    return out


def make_case(seed, H, W, num_classes, B=1, special=True):
    """Seeded (pred, label) uint8 [B, H, W]: patches of classes with noise; with `special`, labels also hold 255, an out-of-range value
    (num_classes + 5) and class 0, and predictions hold 255."""
    rng = np.random.default_rng(seed)
    C = num_classes
    coarse = rng.integers(0, C, size=(B, (H + 15) // 16, (W + 15) // 16))
    label = np.repeat(np.repeat(coarse, 16, 1), 16, 2)[:, :H, :W].astype(np.uint8)
    noise = rng.random((B, H, W))
    pred = np.where(noise < 0.7, label, rng.integers(0, C, size=(B, H, W))).astype(np.uint8)
    if special:
        r = rng.random((B, H, W))
        label[r < 0.05] = 255
        label[(r >= 0.05) & (r < 0.08)] = min(C + 5, 254)
        label[(r >= 0.08) & (r < 0.12)] = 0
        pred[rng.random((B, H, W)) < 0.03] = 255
    return pred, label
