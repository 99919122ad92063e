"""Euclidean boundary evaluation without a GPU: the restatement (tests/boundary_distance_ref.py) against scipy's exact transform and against the Chebyshev
band of tests/boundary_ref.py, the host functions on hand-made histograms, every argument refusal that needs no device, the C entries' checks on the host, and
header / ctypes table / version."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest
import torch

from tests import boundary_distance_ref as DR
from tests import boundary_ref as BR
from tests import eval_ref as ER

import mmsa.evaluate as E  # noqa: E402  (what this file is about: a tree without the Euclidean passes fails every test of it here)

assert DR.FAR == E.DISTANCE_FAR == 65535 and E.MAX_DISTANCE_CAP ** 2 < DR.FAR, "the restatement's FAR is the package's, above every cap^2"

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("mmsa_boundary_distance_u8", "mmsa_eval_boundary_d2", "mmsa_eval_boundary_displacement")


def _maps():
    """Code maps of the kinds the kernel meets: noise over 2, 3 and 26 codes, block maps with blocks of 4 x 5 and 17 x 23, code 255 among the neighbours."""
    rng = np.random.default_rng(11)
    out = [rng.integers(0, n, size=(H, W)).astype(np.int64) for n, (H, W) in ((2, (9, 14)), (3, (23, 31)), (26, (20, 37)))]
    for (bh, bw), (H, W) in (((4, 5), (30, 41)), ((17, 23), (40, 60))):
        coarse = rng.integers(0, 5, size=((H + bh - 1) // bh, (W + bw - 1) // bw))
        out.append(np.repeat(np.repeat(coarse, bh, 0), bw, 1)[:H, :W].astype(np.int64))
    out[-1][5:9, 7:30] = 255
    out.append(np.full((6, 8), 4, dtype=np.int64))
    return out


# ---- 1. the restatement

def test_the_restatement_equals_the_exact_transform_per_class():
    ndi = pytest.importorskip("scipy.ndimage")
    for code in _maps():
        want = np.full(code.shape, DR.INF, dtype=np.int64)
        for c in np.unique(code):
            if (code != c).any():
                d = ndi.distance_transform_edt(code == c)                      # per pixel of class c: the distance to the nearest pixel of another code
                want[code == c] = np.rint(d[code == c] ** 2).astype(np.int64)
        assert np.array_equal(DR.d2_full(code), want)


def test_the_fixed_example_and_the_cap_rule():
    code = np.zeros((5, 7), dtype=np.int64)
    code[2, 3] = 1
    d = DR.d2_full(code)
    assert d[2, 3] == 1 and d[2, 0] == 9 and d[0, 0] == 13 and d[4, 6] == 13 and d[1, 2] == 2
    m = DR.d2_map(code, 3)
    assert m.dtype == np.uint16 and m[2, 0] == 9 and m[0, 0] == DR.FAR and m[0, 1] == 8 and (DR.d2_map(code, 4) == d).all()
    # the border rule: db = the distance to the first pixel outside the image
    b = DR.d2_full(code, border=True)
    assert b[0, 0] == 1 and b[2, 1] == 4 and b[2, 2] == 1 and b[1, 5] == 4 and b[2, 5] == 4
    flat = np.full((5, 9), 7, dtype=np.int64)
    assert (DR.d2_full(flat) == DR.INF).all() and (DR.d2_map(flat, 255) == DR.FAR).all()
    assert DR.d2_full(flat, border=True).tolist()[2] == [1, 4, 9, 9, 9, 9, 9, 4, 1]
    assert DR.k_of(np.array([1, 2, 3, 4, 5, 9, 10, 65025, DR.FAR]), 255).tolist() == [1, 2, 2, 2, 3, 3, 4, 255, 256]
    assert DR.k_of(np.array([1, 2, DR.FAR]), 1).tolist() == [1, 2, 2]


@pytest.mark.parametrize("border", [False, True])
def test_relations_to_the_chebyshev_band(border):
    for code in _maps():
        d2 = DR.d2_full(code, border)
        assert np.array_equal(d2 <= 2, BR.near(code, 1, border)), "D2 <= 2 <=> near(., 1)"
        for d in (1, 2, 3, 8):
            near = BR.near(code, d, border)
            assert not (near & ~(d2 <= 2 * d * d)).any(), "near(., d) => D2 <= 2 d^2"
            assert not ((d2 <= d * d) & ~near).any(), "D2 <= d^2 => near(., d)"


def test_the_restated_counts_and_histogram():
    C, H, W = 5, 23, 31
    pred, label = ER.make_case(5, H, W, C, B=2, special=True)
    lut = ER.lut(C)
    counts, hist, d2p, d2l = DR.evaluate(pred, label, lut, C, 6, 2)
    assert np.array_equal(counts, BR.boundary_counts(pred, label, lut, C, 1)), "t = 2 is the Chebyshev band at radius 1"
    for b in range(2):
        assert np.array_equal(counts[b].sum(0), ER.confusion(pred[b], label[b], C))
        assert np.array_equal(hist[b, 0].sum(-1), (counts[b, 2] + counts[b, 3]).sum(-1)) and np.array_equal(hist[b, 1].sum(-1), (counts[b, 1] + counts[b, 3]).sum(-2))
        assert int(hist[b, :, :, 0].sum()) == 0
    merged = DR.evaluate(pred, label, lut, C, 6, 9, slots=[1, 1], n_slots=3)
    assert int(merged[0][0].sum()) == 0 == int(merged[0][2].sum()) and np.array_equal(merged[1][1], hist.sum(0))


# ---- 2. the host functions on hand-made histograms

def _hist():
    h = np.zeros((2, 3, 6), dtype=np.int64)          # C = 2, cap = 4: bins 0 .. 5
    h[0, 0] = [0, 6, 2, 1, 0, 1]                      # label-boundary pixels of class 0 by their distance to the prediction's contour
    h[1, 0] = [0, 4, 0, 4, 0, 0]
    h[0, 1] = [0, 0, 0, 0, 0, 5]                      # class 1: every label-boundary pixel is FAR from the prediction's contour
    h[1, 2] = [0, 1, 0, 0, 0, 0]                      # a prediction-boundary pixel of the out-of-range row
    return h


def test_boundary_f_on_hand_made_histograms():
    import mmsa
    from mmsa.evaluate import boundary_f_curve_of, boundary_f_of
    h = _hist()
    f = boundary_f_of(h, 1)
    assert list(f) == ["precision", "recall", "F", "precision_all", "recall_all", "F_all"] and f["F"].shape == (2,) and f["F"].dtype == np.float64
    assert f["precision"][0] == 0.5 and f["recall"][0] == 0.6 and f["F"][0] == 2 * 0.5 * 0.6 / (0.5 + 0.6)
    assert np.isnan(f["precision"][1]) and f["recall"][1] == 0.0 and np.isnan(f["F"][1]), "0 / 0 is NaN"
    assert f["precision_all"] == 5 / 9 and f["recall_all"] == 6 / 15
    f3 = boundary_f_of(h, 3)
    assert f3["precision"][0] == 1.0 and f3["recall"][0] == 0.9 and f3["recall_all"] == 9 / 15 and f3["precision_all"] == 1.0
    curve = boundary_f_curve_of(h)
    assert curve["tolerance"].tolist() == [1, 2, 3, 4] and curve["F"].shape == (2, 4) and curve["F_all"].shape == (4,)
    for T in (1, 2, 3, 4):
        one = boundary_f_of(h, T)
        for k in one:
            assert np.array_equal(curve[k][..., T - 1], one[k], equal_nan=True), (k, T)
    assert curve["recall"][0].tolist() == [0.6, 0.8, 0.9, 0.9], "the FAR bin is never matched"
    zero = boundary_f_of(np.zeros((2, 3, 6), dtype=np.int64), 2)
    assert np.isnan(zero["F"]).all() and np.isnan(zero["F_all"]) and np.isnan(zero["precision_all"])
    batch = np.stack([h, 2 * h])
    assert boundary_f_of(batch, 1)["F"].shape == (2, 2) and np.array_equal(boundary_f_of(batch, 1)["F"][1], f["F"], equal_nan=True)
    assert boundary_f_curve_of(batch)["F_all"].shape == (2, 4)
    for bad in (0, 5, -1, 1.0, True, None):
        with pytest.raises(ValueError, match="tolerance = .*an integer in 1..4"):
            boundary_f_of(h, bad)
    for bad in (np.zeros((3, 3, 6), dtype=np.int64), np.zeros((2, 3, 6)), np.zeros((3, 6), dtype=np.int64), np.zeros((2, 3, 2), dtype=np.int64)):
        with pytest.raises(ValueError, match="a displacement histogram is an integer"):
            boundary_f_curve_of(bad)
    assert mmsa.boundary_f_of is boundary_f_of and "counted from 1" in boundary_f_of.__doc__ and "count from 1" in boundary_f_curve_of.__doc__


def test_distance_percentile_on_hand_made_histograms():
    from mmsa.evaluate import boundary_distance_percentile_of as pct
    h = _hist()                                       # side 0 over the rows: [0, 6, 2, 1, 0, 6] of 15; side 1: [0, 5, 0, 4, 0, 0] of 9
    p = pct(h, 0.5)
    assert list(p) == ["label_to_pred", "pred_to_label", "hd"] and p["label_to_pred"] == 2.0 and p["pred_to_label"] == 1.0 and p["hd"] == 2.0
    assert pct(h, 0.375)["label_to_pred"] == 1.0 and pct(h, 0.4)["label_to_pred"] == 2.0, "compared exactly: the float 0.4 is above 6 / 15"
    assert pct(h, 0.6)["label_to_pred"] == 3.0 and pct(h, 0.95)["label_to_pred"] == np.inf and pct(h, 0.95)["hd"] == np.inf, "inf where the bin is cap + 1"
    assert pct(h, 0.95)["pred_to_label"] == 3.0 and pct(h, 1.0)["pred_to_label"] == 3.0 and pct(h)["hd"] == np.inf
    none = h.copy()
    none[1] = 0
    assert np.isnan(pct(none)["pred_to_label"]) and np.isnan(pct(none)["hd"]) and pct(none, 0.5)["label_to_pred"] == 2.0
    for bad in (0, 0.0, 1.5, -0.1, True, None):
        with pytest.raises(ValueError, match="q = .*a share in"):
            pct(h, bad)
    with pytest.raises(ValueError, match="of one slot"):
        pct(np.stack([h, h]))


def test_evaluator_on_hand_made_counts():
    from mmsa.evaluate import BoundaryEvaluator, EuclideanBoundaryEvaluator, LabelPrep, boundary_f_of
    lp = LabelPrep(2)
    ev = EuclideanBoundaryEvaluator(lp, 2.5, cap=4, cases=["fog", "night"])
    assert isinstance(ev, BoundaryEvaluator) and ev.radius == 2.5 and ev.radius2 == 6 and ev.cap == 4 and ev.tolerance == 3 and ev.border is False
    assert ev.counts is None and ev.displacement is None and ev._trailing() == (4, 3, 3)
    assert ev.host_counts().shape == (2, 4, 3, 3) and ev.host_displacement().shape == (2, 2, 3, 6)
    assert EuclideanBoundaryEvaluator(lp, 3, images=4).host_displacement().shape == (0, 2, 3, 5)
    h = _hist()
    ev.host_displacement = lambda: np.stack([h, np.zeros_like(h)])
    c = BR.boundary_counts(*_example(), ER.lut(2), 2, 1)[0]
    ev.host_counts = lambda: np.stack([c, c])
    assert np.array_equal(ev.boundary_f(slot="fog")["F"], boundary_f_of(h, 3)["F"], equal_nan=True) and ev.boundary_f(1)["precision"][0] == 0.5
    assert ev.boundary_f_curve()["F_all"].shape == (4,) and ev.distance_percentile(0.5)["hd"] == 2.0 and np.isnan(ev.distance_percentile(slot="night")["hd"])
    s = ev.summary(slot="fog")
    assert list(s) == ["aAcc", "mIoU", "trimap_aAcc", "trimap_mIoU", "mBIoU", "band", "mBF", "HD95", "radius", "radius2", "metric"]
    assert s["mBF"] == np.round(boundary_f_of(h, 3)["F"][0] * 100, 2) / 100.0 and s["HD95"] == np.inf and s["radius"] == 2.5 and s["radius2"] == 6
    assert s["metric"] == "euclidean" and s["trimap_aAcc"] == 0.75 and s["mBIoU"] == 0.3333, "the parent's entries on the parent's layout"
    assert ev.boundary_iou(slot="fog").tolist() == [1 / 3, 1 / 3] and ev.trimap_metrics(slot="fog")["aAcc"] == 0.75
    plain = EuclideanBoundaryEvaluator(lp, radius2=2, displacement=False)
    assert plain.radius2 == 2 and plain.cap == 2 and plain.radius == np.sqrt(2.0) and plain.with_displacement is False
    plain.host_counts = lambda: c[None]
    assert list(plain.summary()) == ["aAcc", "mIoU", "trimap_aAcc", "trimap_mIoU", "mBIoU", "band", "radius", "radius2", "metric"]
    with pytest.raises(RuntimeError, match="made with displacement=False"):
        plain.boundary_f()


def _example():
    label = np.zeros((1, 8, 8), dtype=np.uint8)
    pred = np.zeros((1, 8, 8), dtype=np.uint8)
    label[0, 2:6, 2:6] = 1
    pred[0, 2:6, 3:7] = 1
    return pred, label


# ---- 3. refusals that need no device

def test_radius_and_cap_are_checked():
    from mmsa.evaluate import EuclideanBoundaryEvaluator, LabelPrep, euclidean_threshold
    lp = LabelPrep(5)
    assert euclidean_threshold(3) == (9, 3) and euclidean_threshold(2.5) == (6, 3) and euclidean_threshold(255) == (65025, 255)
    assert euclidean_threshold(1.0) == (1, 1) and euclidean_threshold(np.sqrt(2.0)) == (2, 2) and euclidean_threshold(radius2=2) == (2, 2)
    assert euclidean_threshold(radius2=9) == (9, 3) and euclidean_threshold(radius2=10) == (10, 4) and euclidean_threshold(radius2=65025) == (65025, 255)
    assert euclidean_threshold(3.0000000000000004)[0] == 9 and euclidean_threshold(2.9999999999999996) == (8, 3), "floor(radius^2) of the float's own value"
    for bad in (0, 0.99, 255.5, 256, -1, True, None, "3", float("nan")):
        with pytest.raises(ValueError, match="mmsa.EuclideanBoundaryEvaluator: radius"):
            EuclideanBoundaryEvaluator(lp, bad)
    for bad in (0, 65026, 2.0, True):
        with pytest.raises(ValueError, match="radius2 = .*1..65025"):
            EuclideanBoundaryEvaluator(lp, radius2=bad)
    with pytest.raises(ValueError, match="radius= or radius2=, one of them"):
        EuclideanBoundaryEvaluator(lp, 3, radius2=9)
    for bad in (0, 256, -3, 4.0, True, "8"):
        with pytest.raises(ValueError, match="mmsa.EuclideanBoundaryEvaluator: cap = .*1..255"):
            EuclideanBoundaryEvaluator(lp, 2, cap=bad)
    with pytest.raises(ValueError, match="cap = 3 is below ceil\\(radius\\) = 4"):
        EuclideanBoundaryEvaluator(lp, 3.5, cap=3)
    assert EuclideanBoundaryEvaluator(lp, 3.5, cap=4).cap == 4 and EuclideanBoundaryEvaluator(lp, 3.5).cap == 4 and EuclideanBoundaryEvaluator(lp, 40, cap=255).cap == 255


def test_class_limits_are_stated_and_refused():
    from mmsa.evaluate import MAX_DISPLACEMENT_CELLS, MAX_DISTANCE_CAP, MAX_EUCLIDEAN_CLASSES, DISTANCE_FAR, EuclideanBoundaryEvaluator, LabelPrep
    src = open(os.path.join(ROOT, "multimodal-sam-adapter_amd", "csrc", "distance.hip")).read()
    hist = open(os.path.join(ROOT, "multimodal-sam-adapter_amd", "csrc", "eval_hist.h")).read()
    assert int(re.search(r"#define DIST_MAX_CAP (\d+)", src).group(1)) == MAX_DISTANCE_CAP == 255
    assert int(re.search(r"#define DIST_FAR (\d+)", src).group(1)) == DISTANCE_FAR == 65535
    assert "#define DIST_MAX_CLASSES MMSA_EVAL_MAX_CLASSES" in src and int(re.search(r"#define MMSA_EVAL_MAX_CLASSES (\d+)", hist).group(1)) == MAX_EUCLIDEAN_CLASSES
    assert MAX_DISPLACEMENT_CELLS == (65536 - 256) // 4 and "#define DIST_MAX_SIDE_CELLS ((DIST_LDS_BYTES - 256) / 4)" in src
    # the sizes that must be served
    assert EuclideanBoundaryEvaluator(LabelPrep(25), 8, cap=255).cap == 255 and EuclideanBoundaryEvaluator(LabelPrep(82), 8, cap=64).cap == 64
    assert EuclideanBoundaryEvaluator(LabelPrep(62), 8, cap=255).cap == 255
    with pytest.raises(RuntimeError, match="mmsa.EuclideanBoundaryEvaluator: 63 classes at cap 255: .* = 16448 cells per side .* at most 16320"):
        EuclideanBoundaryEvaluator(LabelPrep(63), 8, cap=255)
    assert EuclideanBoundaryEvaluator(LabelPrep(63), 8, cap=255, displacement=False).with_displacement is False
    with pytest.raises(RuntimeError, match="127 classes; Euclidean boundary evaluation supports 2..126"):
        EuclideanBoundaryEvaluator(LabelPrep(127), 8, displacement=False)


def test_python_refusals_of_maps_and_arguments():
    import mmsa
    import mmsa.inference as inf
    from mmsa.evaluate import BoundaryEvaluator, EuclideanBoundaryEvaluator, Evaluator, LabelPrep
    lp = LabelPrep(5)
    u8 = torch.zeros(1, 8, 8, dtype=torch.uint8)
    u16 = torch.zeros(1, 8, 8, dtype=torch.uint16)
    for bad in (0, 256, 2.0, True, None):
        with pytest.raises(ValueError, match="cap = .*1..255"):
            mmsa.boundary_distance(u8, bad, num_classes=5)
    with pytest.raises(ValueError, match="num_classes= .* or labels_prep= .*one of them"):
        mmsa.boundary_distance(u8, 3)
    with pytest.raises(ValueError, match="one of them"):
        mmsa.boundary_distance(u8, 3, num_classes=5, labels_prep=lp)
    with pytest.raises(RuntimeError, match="map is torch.float32; a uint8 class map or raw uint8 labels"):
        mmsa.boundary_distance(u8.float(), 3, num_classes=5)
    with pytest.raises(RuntimeError, match="map must be a contiguous \\[B, H, W\\] tensor"):
        mmsa.boundary_distance(u8[0], 3, num_classes=5)
    with pytest.raises(RuntimeError, match="map must be a tensor"):
        mmsa.boundary_distance(np.zeros((1, 8, 8), dtype=np.uint8), 3, num_classes=5)
    with pytest.raises(RuntimeError, match="size=\\(4, 4\\) for a stored 8 x 8 class map"):
        mmsa.boundary_distance(u8, 3, num_classes=5, size=(4, 4))
    with pytest.raises(RuntimeError, match="size mismatch: the label maps are 8 x 8, .* not 4 x 4"):
        mmsa.boundary_distance(u8, 3, labels_prep=lp, size=(4, 4))
    with pytest.raises(RuntimeError, match="map must be a GPU tensor"):
        mmsa.boundary_distance(u8, 3, num_classes=5)
    for fn, last in ((mmsa.boundary_counts_d2, 2), (mmsa.boundary_displacement, 3)):
        with pytest.raises(RuntimeError, match="d2_pred is torch.uint8; a uint16 distance map"):
            fn(u8, u8, lp, u8, u16, last)
        with pytest.raises(RuntimeError, match="d2_label is torch.int16; a uint16 distance map"):
            fn(u8, u8, lp, u16, u16.to(torch.int16), last)
        with pytest.raises(RuntimeError, match="d2_label has shape \\(1, 8, 7\\), the map is \\[B, H, W\\] = \\(1, 8, 8\\)"):
            fn(u8, u8, lp, u16, u16[:, :, :7].contiguous(), last)
        with pytest.raises(RuntimeError, match="pred is torch.int64; a uint8 class map"):
            fn(u8.long(), u8, lp, u16, u16, last)
        with pytest.raises(RuntimeError, match="pred must be a GPU tensor"):
            fn(u8, u8, lp, u16, u16, last)
    for bad in (0, 65026, 2.0, True):
        with pytest.raises(ValueError, match="t = .*1..65025"):
            mmsa.boundary_counts_d2(u8, u8, lp, u16, u16, bad)
    with pytest.raises(ValueError, match="cap = 0; 1..255"):
        mmsa.boundary_displacement(u8, u8, lp, u16, u16, 0)
    with pytest.raises(RuntimeError, match="63 classes at cap 255"):
        mmsa.boundary_displacement(u8, u8, LabelPrep(63), u16, u16, 255)
    with pytest.raises(RuntimeError, match="127 classes; Euclidean boundary evaluation"):
        mmsa.boundary_counts_d2(u8, u8, LabelPrep(127), u16, u16, 4)
    ev = EuclideanBoundaryEvaluator(lp, 2)
    with pytest.raises(RuntimeError, match="pred must be a GPU tensor"):
        ev.add(u8, u8)
    # every entry's boundary= takes the subclass, and the parent keeps its own limits
    ok = inf.MapOptions.of("whole_class_map", labels=u8, boundary=ev).at((1, 8, 8), None, "whole_class_map")
    assert ok.boundary is ev
    with pytest.raises(RuntimeError, match="mmsa.whole_class_map: boundary= needs labels="):
        inf.whole_class_map(None, None, torch.zeros(1, 6, 8, 8), boundary=ev)
    with pytest.raises(ValueError, match="mmsa.BoundaryEvaluator: radius = 33; 1..32 pixels"):
        BoundaryEvaluator(lp, 33)
    with pytest.raises(ValueError, match="mmsa.BoundaryEvaluator: radius = 2.5"):
        BoundaryEvaluator(lp, 2.5)
    assert not isinstance(Evaluator(lp), BoundaryEvaluator)
    assert list(inspect.signature(mmsa.boundary_distance).parameters) == ["map", "cap", "border", "labels_prep", "num_classes", "size", "scratch", "out"]
    assert list(inspect.signature(mmsa.boundary_counts_d2).parameters) == ["pred", "labels", "prep", "d2_pred", "d2_label", "t", "counts", "slots"]
    assert list(inspect.signature(mmsa.boundary_displacement).parameters) == ["pred", "labels", "prep", "d2_pred", "d2_label", "cap", "hist", "slots"]
    assert list(inspect.signature(EuclideanBoundaryEvaluator.__init__).parameters) == ["self", "prep", "radius", "cap", "border", "displacement", "cases", "images",
                                                                                     "device", "radius2"]
    for name in ("EuclideanBoundaryEvaluator", "boundary_distance", "boundary_counts_d2", "boundary_displacement", "boundary_f_of", "boundary_f_curve_of",
                 "boundary_distance_percentile_of"):
        assert name in mmsa.__all__ and hasattr(mmsa, name)
    lut = mmsa.evaluate.code_lut(prep=LabelPrep(5, reduce_zero_label=True))
    assert set(lut.tolist()) <= set(range(6)) | {255} and mmsa.evaluate.code_lut(num_classes=5).tolist() == [min(v, 5) for v in range(256)]


# ---- 4. the C entries on the host

def test_the_entries_refuse_bad_arguments_on_the_host():
    """Before any launch, so no GPU is needed: every pointer is a fake but the slot table, which the entries read on the host."""
    import mmsa
    raw = mmsa.lib.raw
    fake = ctypes.c_void_p(256)
    other = ctypes.c_void_p(512)
    ERR_ARG = -1

    def dist(src=fake, B=1, Hs=4, Ws=4, lut=None, ymap=None, xmap=None, H=4, W=4, cap=3, border=0, scratch=fake, d2=other):
        rc = raw.mmsa_boundary_distance_u8(src, B, Hs, Ws, lut, ymap, xmap, H, W, cap, border, scratch, d2, None)
        return (rc, mmsa.lib.last_error()) if rc else (0, "")

    for cap in (0, 256, -1):
        rc, msg = dist(cap=cap)
        assert rc == ERR_ARG and f"boundary_distance_u8: cap = {cap}; 1..255 are supported" in msg, msg
    for border in (2, -1):
        rc, msg = dist(border=border)
        assert rc == ERR_ARG and f"boundary_distance_u8: border = {border}; 0 " in msg, msg
    for kw in (dict(src=None), dict(scratch=None), dict(d2=None)):
        rc, msg = dist(**kw)
        assert rc == ERR_ARG and "boundary_distance_u8: src, scratch and d2 are required" in msg, msg
    rc, msg = dist(d2=fake)
    assert rc == ERR_ARG and "scratch and d2 are two planes" in msg
    rc, msg = dist(ymap=fake)
    assert rc == ERR_ARG and "boundary_distance_u8: ymap and xmap come together" in msg
    rc, msg = dist(Hs=5)
    assert rc == ERR_ARG and "boundary_distance_u8: size mismatch: the source is 5 x 4, the grid 4 x 4" in msg
    for kw in (dict(B=0), dict(H=0), dict(W=-1), dict(H=1 << 16, W=1 << 16, Hs=1 << 16, Ws=1 << 16)):
        rc, msg = dist(**kw)
        assert rc == ERR_ARG and "boundary_distance_u8: bad map size" in msg, msg

    slots = (ctypes.c_int * 1)(0)

    def counts(entry, name, scalar, C=5, pred=fake, label=fake, lut=fake, buf=fake, tab=slots, d2p=fake, d2l=fake, Hl=4):
        rc = getattr(raw, entry)(pred, label, 1, 4, 4, Hl, 4, lut, C, None, None, tab, 1, d2p, d2l, scalar, buf, None)
        return (rc, mmsa.lib.last_error()) if rc else (0, "")

    for entry, name, good in (("mmsa_eval_boundary_d2", "eval_boundary_d2", 4), ("mmsa_eval_boundary_displacement", "eval_boundary_displacement", 3)):
        for kw in (dict(pred=None), dict(d2p=None), dict(d2l=None)):
            rc, msg = counts(entry, name, good, **kw)
            assert rc == ERR_ARG and f"{name}: pred, d2_pred and d2_label are required" in msg, msg
        for kw in (dict(label=None), dict(lut=None), dict(buf=None), dict(tab=None)):
            rc, msg = counts(entry, name, good, **kw)
            assert rc == ERR_ARG and f"{name}: label, lut, slots and counts are required" in msg, msg
        rc, msg = counts(entry, name, good, Hl=5)
        assert rc == ERR_ARG and f"{name}: size mismatch" in msg
        rc, msg = counts(entry, name, good, tab=(ctypes.c_int * 1)(3))
        assert rc == ERR_ARG and f"{name}: slots[0] = 3 outside the 1 count slots" in msg
    for t in (0, 65026, -4):
        rc, msg = counts("mmsa_eval_boundary_d2", "", t)
        assert rc == ERR_ARG and f"eval_boundary_d2: t = {t}; a squared radius in 1..65025" in msg, msg
    for C in (1, 127):
        rc, msg = counts("mmsa_eval_boundary_d2", "", 4, C=C)
        assert rc == ERR_ARG and f"eval_boundary_d2: {C} classes; 2..126 are supported" in msg and "LDS" in msg, msg
    for cap in (0, 256):
        rc, msg = counts("mmsa_eval_boundary_displacement", "", cap)
        assert rc == ERR_ARG and f"eval_boundary_displacement: cap = {cap}; 1..255 are supported" in msg, msg
    rc, msg = counts("mmsa_eval_boundary_displacement", "", 255, C=63)
    assert rc == ERR_ARG and "eval_boundary_displacement: 63 classes at cap 255: (C + 1) * (cap + 2) = 16448 cells per side; at most 16320" in msg, msg


def test_the_entries_are_declared_bound_and_versioned():
    import mmsa
    from tests.test_host_cpu import _header_prototypes
    hdr = open(os.path.join(ROOT, "include", "mmsa.h")).read()
    ver = open(os.path.join(ROOT, "include", "mmsa_version.h")).read()
    assert mmsa.lib.version() == mmsa.lib.ABI_VERSION == int(re.search(r"#define MMSA_ABI_VERSION (\d+)", ver).group(1)) == 114
    protos = _header_prototypes()
    kinds = {ctypes.c_void_p: "P", ctypes.c_int: "I"}
    for e in ENTRIES:
        assert re.search(r"\bint " + e + r"\(", hdr) and e in mmsa.lib.SIGNATURES and hasattr(mmsa.lib.raw, e) and e in ver, e
        assert protos[e] == ("I", [kinds[t] for t in mmsa.lib.SIGNATURES[e]]), e
    assert len(mmsa.lib.SIGNATURES["mmsa_eval_boundary_d2"]) == len(mmsa.lib.SIGNATURES["mmsa_eval_confusion_u8"]) + 3      # the two maps and t
    assert mmsa.lib.SIGNATURES["mmsa_eval_boundary_displacement"] == mmsa.lib.SIGNATURES["mmsa_eval_boundary_d2"]
