"""Boundary evaluation on the GPU (mmsa_eval_boundary_u8, csrc/boundary.hip): the device counts against the numpy restatement of tests/boundary_ref.py, bit for
bit (torch.equal on int64) -- radii and sizes on both sides of every tile edge, the exact reach of the radius in all eight directions, boundaries on both
sides of every tile seam, the label side (tables, LUT, ignored and out-of-range bytes), the border rule, the identities of the counts, the class limits and
zone groups, and the public entries on the tiny model."""
import functools

import numpy as np
import pytest
import torch

from tests import boundary_ref as BR
from tests import eval_ref as ER
from tests.test_topk_gpu import NUM_CLASSES, SLIDE_CFG, models  # noqa: F401  (the tiny model of the entry tests, a module-scoped fixture)

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
RADII = (1, 2, 3, 7, 16, 32)
SIZES = [(1, 1), (5, 3), (37, 53), (64, 64), (130, 67), (33, 257)]


@functools.lru_cache(maxsize=None)
def _case(H, W, C, B=3):
    pred, label = ER.make_case(1000 * H + W + C, H, W, C, B=B, special=True)
    pred.setflags(write=False)
    label.setflags(write=False)
    return pred, label


def _dev(a):
    return torch.from_numpy(np.array(a)).to(DEV)      # a copy: the cached cases are read-only


def _both(pred, label, C, d, border=False, slots=None, resize=None, **kw):
    """(device counts, restated counts as a tensor) of numpy maps; `resize` = (H, W): the labels go through the nearest-neighbour tables."""
    import mmsa
    from mmsa.evaluate import LabelPrep
    lp = LabelPrep(C, resize=None if resize is None else dict(seg_scale=(resize[1], resize[0]), keep_ratio=False), **kw)
    tabs = (None, None) if resize is None else (ER.nearest_index(label.shape[1], resize[0]), ER.nearest_index(label.shape[2], resize[1]))
    got = mmsa.boundary_counts(_dev(pred), _dev(label), lp, d, border=border, slots=slots)
    want = BR.boundary_counts(pred, label, ER.lut(C, **kw), C, d, border, *tabs, slots=slots)
    assert got.dtype == torch.int64 and tuple(got.shape) == want.shape
    return got.cpu(), torch.from_numpy(want)


# ---- 1. radii and sizes

@pytest.mark.parametrize("C", [5, 25])
@pytest.mark.parametrize("H,W", SIZES)
def test_radii_and_sizes_equal_the_restatement(H, W, C):
    pred, label = _case(H, W, C)
    for d in RADII:
        got, want = _both(pred, label, C, d)
        assert torch.equal(got, want), (H, W, C, d)
        assert int(got.sum()) == int((ER.lut(C)[label] != 255).sum())
    for d in (1, 3, 32):
        got, want = _both(pred, label, C, d, border=True)
        assert torch.equal(got, want), (H, W, C, d, "border")


# ---- 2. the reach of the radius: Chebyshev, exactly d

DIRS = [(-1, -1), (-1, 0), (-1, 1), (0, -1), (0, 1), (1, -1), (1, 0), (1, 1)]


@pytest.mark.parametrize("side", ["label", "pred"])
@pytest.mark.parametrize("d", [1, 3, 32])
def test_the_band_reaches_exactly_d_in_all_eight_directions(d, side):
    """A uniform map with one differing pixel; the OTHER map marks sixteen probe pixels with a class each, at Chebyshev distance d (classes 2..9) and d + 1
    (classes 10..17) in the eight directions, so the zone of every probe can be read from the counts."""
    C, H, W, cy, cx = 25, 75, 71, 36, 35
    one = np.zeros((1, H, W), dtype=np.uint8)
    one[0, cy, cx] = 1
    probes = np.zeros((1, H, W), dtype=np.uint8)
    for k, (dy, dx) in enumerate(DIRS):
        probes[0, cy + d * dy, cx + d * dx] = 2 + k
        probes[0, cy + (d + 1) * dy, cx + (d + 1) * dx] = 10 + k
    label, pred = (one, probes) if side == "label" else (probes, one)
    got, want = _both(pred, label, C, d)
    assert torch.equal(got, want)
    c = got[0].numpy()
    near = (c[2] + c[3]) if side == "label" else (c[1] + c[3])      # the zones near a boundary of the map that holds the single pixel
    far = (c[0] + c[1]) if side == "label" else (c[0] + c[2])
    for k in range(8):
        at_d = (near[0, 2 + k], far[0, 2 + k]) if side == "label" else (near[2 + k, 0], far[2 + k, 0])
        beyond = (near[0, 10 + k], far[0, 10 + k]) if side == "label" else (near[10 + k, 0], far[10 + k, 0])
        assert tuple(at_d) == (1, 0), f"direction {DIRS[k]}: the pixel at distance {d} is in the band"
        assert tuple(beyond) == (0, 1), f"direction {DIRS[k]}: the pixel at distance {d + 1} is not"
    assert int(near.sum()) == (2 * d + 1) ** 2, "the band of one pixel is its (2 d + 1)^2 window"


# ---- 3. seams: a boundary on both sides of every multiple of 16, whatever the tile

@pytest.mark.parametrize("side", ["label", "pred"])
@pytest.mark.parametrize("axis", ["vertical", "horizontal"])
def test_lines_on_both_sides_of_every_seam(axis, side):
    C, H, W = 5, 100, 150
    lines = np.zeros((3, H, W), dtype=np.uint8)
    for b, off in enumerate((-1, 0, 1)):                             # one image per offset: one-pixel lines at k * 16 + off
        for k in range(0, 11):
            at = k * 16 + off
            if axis == "vertical" and 0 <= at < W:
                lines[b, :, at] = 1 + k % 3
            if axis == "horizontal" and 0 <= at < H:
                lines[b, at, :] = 1 + k % 3
    other = _case(H, W, C)[0]
    label, pred = (lines, other) if side == "label" else (other, lines)
    for d in (1, 3, 7):
        got, want = _both(pred, label, C, d)
        assert torch.equal(got, want), (axis, side, d)


# ---- 4. the label side

def test_the_label_side():
    C, H, W = 5, 37, 53
    pred = _case(H, W, C)[0]
    for Hl, Wl in ((19, 23), (90, 120)):                             # up and down through the tables
        label = _case(Hl, Wl, C)[1]
        for d in (1, 3, 16):
            got, want = _both(pred, label, C, d, resize=(H, W))
            assert torch.equal(got, want), (Hl, Wl, d)
        got, want = _both(pred, label, C, 2, border=True, resize=(H, W), slots=[1, 0, 1])
        assert torch.equal(got, want)
    label = _case(H, W, C)[1]                                         # holds 255, an out-of-range byte and class 0; pred holds 255
    assert (label == 255).any() and (label == C + 5).any() and (pred == 255).any()
    for kw in (dict(reduce_zero_label=True), dict(label_map={0: 2, 10: 1, 3: 255}), dict(ignore_index=2), dict(reduce_zero_label=True, label_map={1: 0})):
        for d in (1, 7):
            got, want = _both(pred, label, C, d, **kw)
            assert torch.equal(got, want), (kw, d)
    # an ignored neighbour puts a class pixel in the band; the ignored pixel itself is counted nowhere
    lab = np.zeros((1, 20, 30), dtype=np.uint8)
    lab[0, 9, 14] = 255
    prd = np.zeros((1, 20, 30), dtype=np.uint8)
    got, want = _both(prd, lab, C, 2)
    assert torch.equal(got, want) and int(got.sum()) == 20 * 30 - 1 and int(got[0, 2, 0, 0]) == 24 and int(got[0, 0, 0, 0]) == 20 * 30 - 25
    # prediction byte 255 (and any byte >= C) is the code C: column C, and no boundary between two such bytes
    prd[0, 3:6, 3:6] = 255
    prd[0, 4, 4] = 200
    got, want = _both(prd, lab, C, 1)
    assert torch.equal(got, want) and int(got[0, :, 0, C].sum()) == 9 and int(got[0, 0, 0, C]) == 1      # the centre of the 3 x 3 block is interior


# ---- 5. the border rule

def test_the_border_rule():
    C = 5
    for H, W in ((40, 70), (9, 200), (64, 64)):
        flat = np.full((2, H, W), 3, dtype=np.uint8)
        for d in (1, 4, 32):
            got, want = _both(flat, flat, C, d)
            assert torch.equal(got, want) and int(got[:, 0, 3, 3].sum()) == 2 * H * W == int(got.sum()), "a uniform map: every count in zone 0"
            got, want = _both(flat, flat, C, d, border=True)
            assert torch.equal(got, want)
            if 2 * d >= min(H, W):
                assert int(got[:, 3, 3, 3].sum()) == 2 * H * W, "every pixel is within d of the border: zone 3"
            else:
                assert int(got[:, 0, 3, 3].sum()) == 2 * (H - 2 * d) * (W - 2 * d) and int(got[:, 1].sum()) == 0 == int(got[:, 2].sum())


# ---- 6. identities on device results

def test_identities_of_the_counts():
    import mmsa
    from mmsa.evaluate import BoundaryEvaluator, Evaluator, LabelPrep
    C, H, W = 25, 130, 67
    pred, label = _case(H, W, C)
    d_pred, d_lab = _dev(pred), _dev(label)
    lp = LabelPrep(C)
    conf = mmsa.confusion(d_pred, d_lab, lp)
    for d, border in ((1, False), (7, True), (32, False)):
        got = mmsa.boundary_counts(d_pred, d_lab, lp, d, border=border)
        assert torch.equal(got.sum(1), conf), "the sum over the zones is the confusion matrix"
        again = mmsa.boundary_counts(d_pred, d_lab, lp, d, border=border)
        assert again.cpu().numpy().tobytes() == got.cpu().numpy().tobytes(), "two runs, the same bytes"
        twice = got.clone()
        assert mmsa.boundary_counts(d_pred, d_lab, lp, d, border=border, counts=twice) is twice and torch.equal(twice, 2 * got), "ADDED to"
        merged = mmsa.boundary_counts(d_pred, d_lab, lp, d, border=border, slots=[1, 0, 1])
        assert tuple(merged.shape) == (2, 4, C + 1, C + 1) and torch.equal(merged[1], got[0] + got[2]) and torch.equal(merged[0], got[1])
    got = mmsa.boundary_counts(d_pred, d_lab, lp, 3)
    be, ev = BoundaryEvaluator(lp, 3, cases=["fog", "night"], device=DEV), Evaluator(lp, cases=["fog", "night"], device=DEV)
    be.add(d_pred[:2], d_lab[:2], case="night").add(d_pred[2:], d_lab[2:], case="fog")
    ev.add(d_pred[:2], d_lab[:2], case="night").add(d_pred[2:], d_lab[2:], case="fog")
    assert torch.equal(be.counts[1], got[0] + got[1]) and torch.equal(be.counts[0], got[2])
    assert np.array_equal(be.evaluator_counts(), ev.host_counts())
    s, whole = be.summary(), ev.summary()
    assert s["aAcc"] == whole["aAcc"] and s["mIoU"] == whole["mIoU"] and 0 < s["band"] <= 1 and be.boundary_iou().shape == (C,)
    want = BR.boundary_counts(pred, label, ER.lut(C), C, 3).sum(0)
    assert np.array_equal(be.boundary_iou(), BR.boundary_iou(want), equal_nan=True)
    per = BoundaryEvaluator(lp, 3, border=True, images=4)
    per.add(d_pred[:1], d_lab[:1]).add(d_pred[1:], d_lab[1:])
    assert per.used == 3 and torch.equal(per.counts[:3], mmsa.boundary_counts(d_pred, d_lab, lp, 3, border=True)) and per.host_counts().shape[0] == 3
    with pytest.raises(RuntimeError, match="per-image slots"):
        per.add(d_pred[:2], d_lab[:2])
    with pytest.raises(ValueError, match="radius = 33; 1..32"):
        mmsa.boundary_counts(d_pred, d_lab, lp, 33)
    with pytest.raises(RuntimeError, match="counts must be a contiguous int64"):
        mmsa.boundary_counts(d_pred, d_lab, lp, 3, counts=torch.zeros(3, C + 1, C + 1, dtype=torch.int64, device=DEV))


# ---- 7. classes: the limits and the zone groups

def _thresholds(r):
    """(the largest C that runs as one zone group, the largest with two) at radius r, from the launch shape the Python layer states."""
    from mmsa.evaluate import MAX_BOUNDARY_CLASSES, boundary_launch_shape
    groups = [boundary_launch_shape(C, r)[0] for C in range(2, MAX_BOUNDARY_CLASSES + 1)]
    return 2 + groups.count(1) - 1, 2 + groups.count(1) + groups.count(2) - 1


@pytest.mark.parametrize("r", [3, 32])
def test_class_limits_and_zone_groups(r):
    import mmsa
    from mmsa.evaluate import MAX_BOUNDARY_CLASSES, LabelPrep, boundary_launch_shape
    one, two = _thresholds(r)
    assert 25 <= one < two <= MAX_BOUNDARY_CLASSES
    classes = sorted({2, one, one + 1, two, min(two + 1, MAX_BOUNDARY_CLASSES), MAX_BOUNDARY_CLASSES})
    assert [boundary_launch_shape(C, r)[0] for C in (one, one + 1, two)] == [1, 2, 2] and boundary_launch_shape(MAX_BOUNDARY_CLASSES, 32)[0] == 4
    H, W = 40, 131                                                    # two tiles across; two tiles down at the 32-row tile of the large radii
    for C in classes:
        pred, label = _case(H, W, C, B=2)
        for border in ((False, True) if C in (one + 1, MAX_BOUNDARY_CLASSES) else (False,)):
            got, want = _both(pred, label, C, r, border=border)
            assert torch.equal(got, want), (C, r, border, boundary_launch_shape(C, r))
    with pytest.raises(RuntimeError, match=f"{MAX_BOUNDARY_CLASSES + 1} classes; boundary evaluation supports 2..{MAX_BOUNDARY_CLASSES}"):
        mmsa.boundary_counts(_dev(pred), _dev(label), LabelPrep(MAX_BOUNDARY_CLASSES + 1), r)


# ---- 8. the entries on the tiny model

def test_entries_count_the_returned_map(models):  # noqa: F811
    import mmsa
    import mmsa.inference as inf
    from mmsa.evaluate import BoundaryEvaluator, Evaluator, LabelPrep
    cfg, m, h, frame, x = models
    lp = LabelPrep(NUM_CLASSES)
    g = torch.Generator().manual_seed(12)

    def labels(shape):
        coarse = torch.randint(0, NUM_CLASSES, (shape[0], (shape[1] + 15) // 16, (shape[2] + 15) // 16), generator=g, dtype=torch.uint8)
        lab = coarse.repeat_interleave(16, 1).repeat_interleave(16, 2)[:, :shape[1], :shape[2]].contiguous()
        lab[torch.rand(shape, generator=g) < 0.03] = 255
        return lab.to(DEV)

    def fresh(**kw):
        return BoundaryEvaluator(lp, 3, images=4, device=DEV, **kw), Evaluator(lp, images=4, device=DEV)

    # slide_class_map, at the frame's size (with and without the fused evaluation launch) and rescaled
    for kw in (dict(), dict(fused=True), dict(ori_shape=(300, 380, 3)), dict(topk=2)):
        plain = inf.slide_class_map(m, h, frame, (256, 256), (170, 170), max_batch=2, **{k: v for k, v in kw.items() if k != "fused"})[0]
        lab = labels(plain.shape)
        be, ev = fresh()
        cm = inf.slide_class_map(m, h, frame, (256, 256), (170, 170), max_batch=2, labels=lab, evaluator=ev, boundary=be, **kw)[0]
        assert torch.equal(cm, plain) and torch.equal(be.counts[:1], mmsa.boundary_counts(cm, lab, lp, 3)), f"slide {kw}"
        assert np.array_equal(be.evaluator_counts(), ev.host_counts()) and int(be.counts.sum()) == int((lab != 255).sum())
    # whole_class_map with ori_shape=, without an evaluator next to it
    plain = inf.whole_class_map(m, h, x, ori_shape=(200, 310))
    lab = labels(plain.shape)
    be, _ = fresh(border=True)
    cm = inf.whole_class_map(m, h, x, ori_shape=(200, 310), labels=lab, boundary=be)
    assert torch.equal(cm, plain) and torch.equal(be.counts[:2], mmsa.boundary_counts(cm, lab, lp, 3, border=True)) and be.used == 2
    # class_map by mode
    be, ev = fresh()
    cm = inf.class_map(m, h, x, dict(mode="whole_dim", dim=(192, 240)), labels=(lab2 := labels((2, 192, 240))), evaluator=ev, boundary=be)
    assert torch.equal(be.counts[:2], mmsa.boundary_counts(cm, lab2, lp, 3)) and np.array_equal(be.evaluator_counts(), ev.host_counts())
    # aug_class_map
    imgs, flips, ori = [frame, frame.flip(3)], [None, "horizontal"], (300, 380, 3)
    plain = inf.aug_class_map(m, h, imgs, SLIDE_CFG, ori_shape=ori, flips=flips, max_batch=4)[0]
    lab = labels(plain.shape)
    be, ev = fresh()
    cm = inf.aug_class_map(m, h, imgs, SLIDE_CFG, ori_shape=ori, flips=flips, max_batch=4, labels=lab, evaluator=ev, boundary=be)[0]
    assert torch.equal(cm, plain) and torch.equal(be.counts[:1], mmsa.boundary_counts(cm, lab, lp, 3))
    assert np.array_equal(be.evaluator_counts(), ev.host_counts())
    with pytest.raises(RuntimeError, match="slide_class_map: boundary= with return_map=False"):
        inf.slide_class_map(m, h, frame, (256, 256), (170, 170), labels=lab, evaluator=ev, boundary=be, return_map=False)


def test_runner_counts_the_boundaries_of_every_frame(models):  # noqa: F811
    import mmsa
    import mmsa.inference as inf
    from mmsa.evaluate import BoundaryEvaluator, Evaluator, LabelPrep
    cfg, m, h, frame, x = models
    lp = LabelPrep(NUM_CLASSES)
    cm = inf.slide_class_map(m, h, frame, (256, 256), (170, 170), max_batch=2)[0]
    lab = torch.randint(0, NUM_CLASSES, tuple(cm.shape), generator=torch.Generator().manual_seed(6), dtype=torch.uint8).to(DEV)
    sr = inf.SlideRunner(m, h, frame, (256, 256), (170, 170), chains=2)
    be, ev = BoundaryEvaluator(lp, 2, cases=["day", "all"], device=DEV), Evaluator(lp, cases=["day", "all"], device=DEV)
    for _ in range(2):                                                # two frames
        res = sr.run(labels=lab, evaluator=ev, boundary=be, case="all")
        torch.cuda.synchronize()
        assert torch.equal(res.outputs()[0], cm)
    one = mmsa.boundary_counts(cm, lab, lp, 2, slots=[1], counts=torch.zeros_like(be.counts))
    assert torch.equal(be.counts, 2 * one) and int(be.counts[0].sum()) == 0
    assert np.array_equal(be.evaluator_counts(), ev.host_counts())
    be.reset()
    sr.run(labels=lab, boundary=be, case="day")                      # without an evaluator next to it
    torch.cuda.synchronize()
    assert torch.equal(be.counts[0], one[1]) and int(be.counts[1].sum()) == 0
    with pytest.raises(RuntimeError, match="SlideRunner.run: boundary= needs labels="):
        sr.run(boundary=be)
    with pytest.raises(RuntimeError, match="SlideRunner.run: boundary= with return_map=False"):
        sr.run(labels=lab, evaluator=ev, boundary=be, return_map=False)
