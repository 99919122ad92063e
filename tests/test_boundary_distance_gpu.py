"""Euclidean boundary evaluation on the GPU (csrc/distance.hip): the distance maps, the zone counts and the displacement histogram against the numpy restatement
of tests/boundary_distance_ref.py, bit for bit -- every alignment class of a 64-wide wave, caps beyond the image and at the saturation of the row runs, uniform
maps, batch seams, noise and block maps, the label side (LUT, tables, slots), the identities that tie the counts to the Chebyshev pass and to the confusion
matrix, the evaluator on the entries of the tiny model, and the limits."""
import functools

import numpy as np
import pytest
import torch

from tests import boundary_distance_ref as DR
from tests import boundary_ref as BR
from tests import eval_ref as ER
from tests.test_topk_gpu import NUM_CLASSES, SLIDE_CFG, models  # noqa: F401  (the tiny model of the entry tests, a module-scoped fixture)

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SIZES = [(1, 1), (1, 70), (67, 1), (2, 3), (9, 63), (9, 64), (9, 65), (67, 130)]


def _dev(a):
    return torch.from_numpy(np.array(a)).to(DEV)      # a copy: the cached cases are read-only


def _host(t):
    return t.cpu().numpy()


@functools.lru_cache(maxsize=None)
def _codes(H, W, B=2):
    """uint8 [B, H, W]: image 0 noise over 3 codes, image 1 blocks of 4 x 5 over 5 codes with a patch of code 255 -- read-only, shared."""
    rng = np.random.default_rng(1000 * H + W)
    out = np.zeros((B, H, W), dtype=np.uint8)
    out[0] = rng.integers(0, 3, size=(H, W))
    coarse = rng.integers(0, 5, size=((H + 3) // 4, (W + 4) // 5))
    out[1] = np.repeat(np.repeat(coarse, 4, 0), 5, 1)[:H, :W]
    out[1, H // 3:H // 3 + 2, W // 2:W // 2 + 9] = 255
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def _full_of(data, shape):
    """The restated distances of one image (no border, no cap), computed once per map."""
    d = DR.d2_full(np.frombuffer(data, dtype=np.uint8).reshape(shape))
    d.setflags(write=False)
    return d


def _want(code, cap, border):
    """uint16 [B, H, W] for uint8 codes [B, H, W]: the restatement with the border and cap rules applied to the shared distances."""
    out = []
    for one in code:
        d = _full_of(one.tobytes(), one.shape)
        out.append(DR.capped(np.minimum(d, DR.border_d2(*one.shape)) if border else d, cap))
    return np.stack(out)


def _check(code, cap, what=""):
    import mmsa
    for border in (False, True):
        got = mmsa.boundary_distance(_dev(code), cap, border, num_classes=254)
        assert got.dtype == torch.uint16 and tuple(got.shape) == code.shape
        want = _want(code, cap, border)
        bad = np.argwhere(_host(got) != want)
        assert bad.size == 0, (what, code.shape, cap, border, bad[:5].tolist(), _host(got)[tuple(bad[0])], want[tuple(bad[0])])


# ---- 1. the distance kernel

@pytest.mark.parametrize("H,W", SIZES)
def test_every_alignment_class_equals_the_restatement(H, W):
    code = _codes(H, W)
    for cap in (1, 2, 5, 64, 255):
        _check(code, cap)


@pytest.mark.parametrize("H,W", [(3, 255), (3, 256), (3, 257), (2, 600)])
def test_rows_on_both_sides_of_one_pixel_per_lane(H, W):
    """The row pass gives each of a workgroup's 256 lanes ceil(W / 256) pixels: one up to 256 columns, two from 257 on, three at 600 with idle lanes at the end."""
    for cap in (2, 40, 255):
        _check(_codes(H, W), cap)


@pytest.mark.parametrize("W,x", [(256, 255), (512, 1), (512, 511)])
def test_a_row_with_one_change_at_an_end_of_the_scan(W, x):
    """The scan over the lanes of a row (csrc/row_scan.h) with ONE marked index in the whole row, every other row without any: the change in the last piece of
    the last wave (one pixel per lane at 256 columns, two at 512) and in the first piece of the first wave (a change is at x >= 1: two pixels per lane)."""
    code = np.zeros((2, 5, W), dtype=np.uint8)
    code[0, 2, x:] = 9                                                # the only change of image 0: at x of row 2
    code[1, 4, :x] = 9                                                # and of image 1: at x of row 4
    for cap in (3, 255):
        _check(code, cap, (W, x))


def test_a_cap_larger_than_the_image():
    _check(_codes(9, 70), 255)
    _check(_codes(9, 70), 100)


@pytest.mark.parametrize("cap", [255, 7])
def test_saturation_at_the_cap(cap):
    """One differing pixel at the end of a 5 x 300 map: along its row the distances run from 1 to 299; those above the cap are FAR, the cap itself is not."""
    import mmsa
    code = np.zeros((1, 5, 300), dtype=np.uint8)
    code[0, 4, 299] = 9
    _check(code, cap)
    got = _host(mmsa.boundary_distance(_dev(code), cap, num_classes=254))[0]
    d = 299 - np.arange(300)                                          # the distance along row 4
    assert (got[4, :299][d[:299] > cap] == DR.FAR).all() and got[4, 299 - cap] == cap * cap and got[4, 298 - cap] == DR.FAR
    assert got[4, 299] == 1 and got[0, 299] == (16 if cap >= 4 else DR.FAR)
    rows = np.zeros((1, 300, 5), dtype=np.uint8)                     # the same down a column
    rows[0, 299, 4] = 9
    _check(rows, cap)


def test_a_uniform_map():
    import mmsa
    flat = np.full((2, 40, 70), 3, dtype=np.uint8)
    for cap in (1, 9, 255):
        got = _host(mmsa.boundary_distance(_dev(flat), cap, num_classes=25))
        assert (got == DR.FAR).all(), "one code: nothing is near, at any cap"
        got = _host(mmsa.boundary_distance(_dev(flat), cap, True, num_classes=25))
        assert np.array_equal(got[0], DR.capped(DR.border_d2(40, 70), cap)) and np.array_equal(got[0], got[1]), "the db^2 pattern"


def test_no_distance_leaks_across_a_batch_seam():
    import mmsa
    for H, W in ((6, 64), (5, 70), (4, 3)):
        code = np.zeros((3, H, W), dtype=np.uint8)
        code[1], code[2] = 7, 200
        got = _host(mmsa.boundary_distance(_dev(code), 255, num_classes=254))
        assert (got == DR.FAR).all(), "neighbouring images are uniform with different codes: every image is FAR everywhere"
        code[1, H - 1, W - 1] = 0                                     # one pixel next to the seam changes its own image only
        got = _host(mmsa.boundary_distance(_dev(code), 255, num_classes=254))
        assert (got[0] == DR.FAR).all() and (got[2] == DR.FAR).all() and np.array_equal(got, _want(code, 255, False))


@pytest.mark.parametrize("kind", ["noise2", "noise3", "noise26", "blocks4x5", "blocks17x23"])
def test_map_contents(kind):
    rng = np.random.default_rng(len(kind))
    H, W = 45, 150
    if kind.startswith("noise"):
        code = rng.integers(0, int(kind[5:]), size=(1, H, W)).astype(np.uint8)
    else:
        bh, bw = (4, 5) if kind == "blocks4x5" else (17, 23)
        coarse = rng.integers(0, 6, size=(1, (H + bh - 1) // bh, (W + bw - 1) // bw))
        code = np.repeat(np.repeat(coarse, bh, 1), bw, 2)[:, :H, :W].astype(np.uint8)
    code[0, 10:13, 40:90] = 255                                        # code 255 as a neighbour
    for cap in (3, 32, 255):
        _check(code, cap, kind)
    # num_classes makes the codes: every byte from C on is ONE code
    import mmsa
    got = mmsa.boundary_distance(_dev(code), 32, num_classes=2)
    assert np.array_equal(_host(got), _want(np.minimum(code, 2), 32, False))


# ---- 2. the label side, slots and cases: everything an add() leaves behind

@functools.lru_cache(maxsize=None)
def _case(H, W, C, B=3):
    pred, label = ER.make_case(1000 * H + W + C, H, W, C, B=B, special=True)
    pred.setflags(write=False)
    label.setflags(write=False)
    return pred, label


def _both(pred, label, C, radius2, cap, border=False, slots=None, resize=None, **kw):
    """(device counts, histogram, d2_pred, d2_label) and the restated four, of numpy maps; `resize` = (H, W): the labels go through the tables."""
    import mmsa
    from mmsa.evaluate import LabelPrep
    lp = LabelPrep(C, resize=None if resize is None else dict(seg_scale=(resize[1], resize[0]), keep_ratio=False), **kw)
    tabs = (None, None) if resize is None else (ER.nearest_index(label.shape[1], resize[0]), ER.nearest_index(label.shape[2], resize[1]))
    dp, dl = _dev(pred), _dev(label)
    d2p = mmsa.boundary_distance(dp, cap, border, num_classes=C)
    d2l = mmsa.boundary_distance(dl, cap, border, labels_prep=lp)
    counts = mmsa.boundary_counts_d2(dp, dl, lp, d2p, d2l, radius2, slots=slots)
    hist = mmsa.boundary_displacement(dp, dl, lp, d2p, d2l, cap, slots=slots)
    want = DR.evaluate(pred, label, ER.lut(C, **kw), C, cap, radius2, border, *tabs, slots=slots)
    assert counts.dtype == torch.int64 and tuple(counts.shape) == want[0].shape and hist.dtype == torch.int64 and tuple(hist.shape) == want[1].shape
    return (_host(counts), _host(hist), _host(d2p), _host(d2l)), want


def _same(got, want, what):
    for g, w, name in zip(got, want, ("counts", "hist", "d2_pred", "d2_label")):
        assert np.array_equal(g, w), (what, name)


def test_the_label_side():
    C, H, W = 5, 37, 53
    pred = _case(H, W, C)[0]
    for Hl, Wl in ((19, 23), (90, 120)):                             # up and down through the tables
        label = _case(Hl, Wl, C)[1]
        _same(*_both(pred, label, C, 9, 4, resize=(H, W)), (Hl, Wl))
        _same(*_both(pred, label, C, 2, 6, border=True, resize=(H, W), slots=[1, 0, 1]), (Hl, Wl, "border, slots"))
    label = _case(H, W, C)[1]                                         # holds 255, an out-of-range byte and class 0; pred holds 255
    assert (label == 255).any() and (label == C + 5).any() and (pred == 255).any()
    for kw in (dict(reduce_zero_label=True), dict(label_map={0: 2, 10: 1, 3: 255}), dict(ignore_index=2), dict(reduce_zero_label=True, label_map={1: 0})):
        _same(*_both(pred, label, C, 5, 3, **kw), kw)
    # an ignored neighbour puts a class pixel next to a label boundary; the ignored pixel itself is counted nowhere
    lab = np.zeros((1, 20, 30), dtype=np.uint8)
    lab[0, 9, 14] = 255
    prd = np.zeros((1, 20, 30), dtype=np.uint8)
    got, want = _both(prd, lab, C, 4, 2)
    _same(got, want, "ignored neighbour")
    assert int(got[0].sum()) == 20 * 30 - 1 and int(got[0][0, 2, 0, 0]) == 12 and int(got[1][0, 0, 0].sum()) == 8 and int(got[1][0, 0, 0, 3]) == 8
    assert (got[2] == DR.FAR).all() and got[3][0, 9, 14] == 1 and got[3][0, 9, 12] == 4 and got[3][0, 9, 11] == DR.FAR


# ---- 3. identities on device results

def test_identities_of_the_counts():
    import mmsa
    from mmsa.evaluate import EuclideanBoundaryEvaluator, LabelPrep
    C, H, W = 25, 67, 130
    pred, label = _case(H, W, C)
    dp, dl = _dev(pred), _dev(label)
    lp = LabelPrep(C)
    conf = mmsa.confusion(dp, dl, lp)
    for border in (False, True):
        ev = EuclideanBoundaryEvaluator(lp, radius2=2, border=border, images=3, device=DEV).add(dp, dl)
        assert ev.cap == 2 and torch.equal(ev.counts, mmsa.boundary_counts(dp, dl, lp, 1, border=border)), "radius2 = 2 is the Chebyshev band at radius 1, bit for bit"
        side0, side1 = ev.displacement[:, 0].sum(-1), ev.displacement[:, 1].sum(-1)
        assert torch.equal(side0, (ev.counts[:, 2] + ev.counts[:, 3]).sum(-1)), "side 0 by class: the label band at t = 2, row by row"
        assert torch.equal(side1, (ev.counts[:, 1] + ev.counts[:, 3]).sum(-2)), "side 1 by class: the prediction band at t = 2, column by column"
        assert int(ev.displacement[..., 0].sum()) == 0, "bin 0 stays 0"
        d2p = mmsa.boundary_distance(dp, 12, border, num_classes=C)
        d2l = mmsa.boundary_distance(dl, 12, border, labels_prep=lp)
        hp, hl = _host(d2p).astype(np.int64), _host(d2l).astype(np.int64)
        codes = [BR.codes(pred[b], label[b], ER.lut(C), C) for b in range(3)]
        near = {}
        for t in (1, 2, 9, 18, 64, 128, 144):                        # several radii from ONE pair of maps; thresholding the maps on the host gives the same counts
            got = mmsa.boundary_counts_d2(dp, dl, lp, d2p, d2l, t)
            assert torch.equal(got.sum(1), conf), "the zone sum is the confusion matrix"
            want = np.stack([BR.counts_of(2 * (hl[b] <= t) + (hp[b] <= t), *codes[b], C) for b in range(3)])
            assert np.array_equal(_host(got), want), (t, border)
            near[t] = _host(got)
        for d in (1, 3, 8):                                           # the near sets are nested: t = d^2 inside Chebyshev d inside t = 2 d^2
            cheb = _host(mmsa.boundary_counts(dp, dl, lp, d, border=border))
            inner, outer = near[d * d], near[2 * d * d]
            for lo, hi in ((inner, cheb), (cheb, outer)):
                assert (lo[:, 3] <= hi[:, 3]).all() and (lo[:, 0] >= hi[:, 0]).all(), d
                assert ((lo[:, 2] + lo[:, 3]) <= (hi[:, 2] + hi[:, 3])).all() and ((lo[:, 1] + lo[:, 3]) <= (hi[:, 1] + hi[:, 3])).all(), d
    twice = near[144].copy()
    buf = _dev(twice)
    assert mmsa.boundary_counts_d2(dp, dl, lp, d2p, d2l, 144, counts=buf) is buf and np.array_equal(_host(buf), 2 * twice), "ADDED to"
    merged = mmsa.boundary_displacement(dp, dl, lp, d2p, d2l, 12, slots=[1, 0, 1])
    per = mmsa.boundary_displacement(dp, dl, lp, d2p, d2l, 12)
    assert tuple(merged.shape) == (2, 2, C + 1, 14) and torch.equal(merged[1], per[0] + per[2]) and torch.equal(merged[0], per[1])
    with pytest.raises(RuntimeError, match="out must be a contiguous uint16"):
        mmsa.boundary_distance(dp, 12, num_classes=C, out=torch.empty(3, H, W, dtype=torch.int16, device=DEV))
    with pytest.raises(RuntimeError, match="scratch must be a contiguous uint16 tensor of at least"):
        mmsa.boundary_distance(dp, 12, num_classes=C, scratch=torch.empty(10, dtype=torch.uint16, device=DEV))
    with pytest.raises(RuntimeError, match="hist must be a contiguous int64"):
        mmsa.boundary_displacement(dp, dl, lp, d2p, d2l, 12, hist=torch.zeros(3, 2, C + 1, 13, dtype=torch.int64, device=DEV))


# ---- 4. the evaluator and the entries

def test_the_evaluator_adds_what_the_restatement_adds():
    from mmsa.evaluate import BoundaryEvaluator, EuclideanBoundaryEvaluator, LabelPrep
    C, H, W = 5, 37, 53
    pred, label = _case(H, W, C)
    dp, dl = _dev(pred), _dev(label)
    lp = LabelPrep(C)
    ev = EuclideanBoundaryEvaluator(lp, 2.5, cap=6, cases=["fog", "night"], device=DEV)
    assert ev.counts is not None and ev.displacement is not None and tuple(ev.displacement.shape) == (2, 2, C + 1, 8)
    ev.add(dp[:2], dl[:2], case="night").add(dp[2:], dl[2:], case="fog")
    torch.cuda.synchronize()
    want = DR.evaluate(pred, label, ER.lut(C), C, 6, 6, slots=[1, 1, 0])
    assert np.array_equal(_host(ev.counts), want[0]) and np.array_equal(_host(ev.displacement), want[1])
    first = (_host(ev.counts).tobytes(), _host(ev.displacement).tobytes())
    ev.reset()
    before = torch.cuda.memory_allocated()
    ev.add(dp[:2], dl[:2], case="night").add(dp[2:], dl[2:], case="fog")
    torch.cuda.synchronize()
    assert torch.cuda.memory_allocated() == before, "a second add of the same shapes allocates nothing"
    assert (_host(ev.counts).tobytes(), _host(ev.displacement).tobytes()) == first, "a repeated run, the same bytes"
    assert np.array_equal(ev.evaluator_counts(), want[0].sum(1)) and ev.boundary_iou().shape == (C,)
    s = ev.summary()
    assert list(s)[-5:] == ["mBF", "HD95", "radius", "radius2", "metric"] and 0 <= s["mBF"] <= 1 and s["HD95"] >= 1 and s["radius2"] == 6
    import mmsa
    assert np.array_equal(ev.boundary_f(2, slot="fog")["F"], mmsa.boundary_f_of(want[1][0], 2)["F"], equal_nan=True)
    assert ev.distance_percentile()["hd"] == mmsa.boundary_distance_percentile_of(want[1].sum(0))["hd"]
    per = EuclideanBoundaryEvaluator(lp, 3, border=True, displacement=False, images=4)
    per.add(dp[:1], dl[:1]).add(dp[1:], dl[1:])
    assert per.used == 3 and per.displacement is None and np.array_equal(_host(per.counts[:3]), DR.evaluate(pred, label, ER.lut(C), C, 3, 9, True)[0])
    with pytest.raises(RuntimeError, match="per-image slots"):
        per.add(dp[:2], dl[:2])
    with pytest.raises(RuntimeError, match="size mismatch"):
        per.add(dp[:1], dl[:1, :30].contiguous())
    with pytest.raises(ValueError, match="mmsa.BoundaryEvaluator: radius = 33; 1..32 pixels"):
        BoundaryEvaluator(lp, 33)


def test_entries_count_the_returned_map(models):  # noqa: F811
    import mmsa.inference as inf
    from mmsa.evaluate import EuclideanBoundaryEvaluator, Evaluator, LabelPrep
    cfg, m, h, frame, x = models
    lp = LabelPrep(NUM_CLASSES)
    g = torch.Generator().manual_seed(12)

    def labels(shape):
        coarse = torch.randint(0, NUM_CLASSES, (shape[0], (shape[1] + 15) // 16, (shape[2] + 15) // 16), generator=g, dtype=torch.uint8)
        lab = coarse.repeat_interleave(16, 1).repeat_interleave(16, 2)[:, :shape[1], :shape[2]].contiguous()
        lab[torch.rand(shape, generator=g) < 0.03] = 255
        return lab.to(DEV)

    def fresh(**kw):
        return EuclideanBoundaryEvaluator(lp, 3.5, cap=8, images=4, device=DEV, **kw)

    plain = inf.whole_class_map(m, h, x, ori_shape=(200, 310))
    lab = labels(plain.shape)
    be, ev, alone = fresh(border=True), Evaluator(lp, images=4, device=DEV), fresh(border=True)
    cm = inf.whole_class_map(m, h, x, ori_shape=(200, 310), labels=lab, evaluator=ev, boundary=be)
    alone.add(cm, lab)
    assert torch.equal(cm, plain) and be.used == 2 and torch.equal(be.counts, alone.counts) and torch.equal(be.displacement, alone.displacement)
    assert int(be.counts.sum()) == int((lab != 255).sum()) and np.array_equal(be.evaluator_counts(), ev.host_counts())
    plain = inf.slide_class_map(m, h, frame, (256, 256), (170, 170), max_batch=2)[0]
    lab = labels(plain.shape)
    be, alone = fresh(), fresh()
    cm = inf.slide_class_map(m, h, frame, (256, 256), (170, 170), max_batch=2, labels=lab, boundary=be)[0]
    alone.add(cm, lab)
    assert torch.equal(cm, plain) and torch.equal(be.counts, alone.counts) and torch.equal(be.displacement, alone.displacement) and int(be.displacement.sum()) > 0


# ---- 5. the limits

@pytest.mark.parametrize("C,cap", [(25, 255), (82, 64), (62, 255), (126, 100)])
def test_the_sizes_that_must_be_served(C, cap):
    pred, label = _case(40, 131, C, B=2)
    _same(*_both(pred, label, C, min(cap * cap, 50), cap), (C, cap))


def test_a_combination_beyond_the_limit_is_refused_before_any_launch():
    import mmsa
    from mmsa.evaluate import EuclideanBoundaryEvaluator, LabelPrep
    pred, label = _case(40, 131, 5, B=2)
    dp, dl = _dev(pred), _dev(label)
    d2 = mmsa.boundary_distance(dp, 255, num_classes=63)
    with pytest.raises(RuntimeError, match="63 classes at cap 255: .* = 16448 cells per side .* at most 16320"):
        mmsa.boundary_displacement(dp, dl, LabelPrep(63), d2, d2, 255)
    with pytest.raises(RuntimeError, match="63 classes at cap 255"):
        EuclideanBoundaryEvaluator(LabelPrep(63), 10, cap=255, device=DEV)
    with pytest.raises(RuntimeError, match="127 classes; Euclidean boundary evaluation supports 2..126"):
        mmsa.boundary_counts_d2(dp, dl, LabelPrep(127), d2, d2, 4)
    ok = EuclideanBoundaryEvaluator(LabelPrep(63), 10, cap=255, displacement=False, images=2, device=DEV).add(dp, dl)      # the zone counts alone have no such limit
    assert int(ok.counts.sum()) == int((ER.lut(63)[label] != 255).sum())
