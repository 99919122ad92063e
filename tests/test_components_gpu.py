"""Segment-level evaluation on the GPU (csrc/components.hip): the root maps, the areas, the suppressed maps and the segment counts against the numpy
restatement of tests/components_ref.py, byte for byte.  Everything is integers: every comparison is equality.  The shapes are the smallest at which each
mechanism can fail: one pixel, one row, one column, a map inside one 64 x 32 tile, maps of several tiles that are ragged on both axes, two different images
in a batch; the long parent chains (serpentine, spiral), the late merge (comb), the corner-only contact (staircase), the codes 255 and C, the label side
through LUT and tables; then the identities that tie the counts to the confusion matrix, the evaluator and the entries on the tiny model."""
import functools

import numpy as np
import pytest
import torch

from tests import boundary_ref as BR
from tests import components_ref as CR
from tests import eval_ref as ER
from tests.test_topk_gpu import NUM_CLASSES, SLIDE_CFG, models  # noqa: F401  (the tiny model of the entry tests, a module-scoped fixture)

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
C = 25
SHAPES = [(1, 1), (1, 257), (257, 1), (31, 63), (67, 131), (130, 200)]


def _dev(a):
    return torch.from_numpy(np.array(a)).to(DEV)      # a copy: the cached cases are read-only


def _host(t):
    return t.cpu().numpy()


@functools.lru_cache(maxsize=None)
def _map(kind, H, W):
    """uint8 [H, W], read-only and shared: the maps of the issue's list."""
    rng = np.random.default_rng(1000 * H + W + len(kind))
    if kind == "noise":
        m = rng.integers(0, C, size=(H, W)).astype(np.uint8)
    elif kind == "blocky":
        m = CR.blocky(rng, H, W, C)
    elif kind == "special":      # regions of the bytes C, C + 3 and 255 (ONE code of a class map, min(v, C)) next to classes
        m = CR.blocky(rng, H, W, 4, 5, 11)
        m[H // 5:H // 2, W // 4:W // 2] = C
        m[H // 3:2 * H // 3, W // 2:3 * W // 4] = 255
        m[H // 2:H // 2 + 3, :] = C + 3
    else:
        m = getattr(CR, kind)(H, W)
    m.setflags(write=False)
    return m


@functools.lru_cache(maxsize=None)
def _want_roots(kind, H, W, connectivity, num_classes=C):
    r = CR.roots(np.minimum(_map(kind, H, W), num_classes), connectivity)
    r.setflags(write=False)
    return r


def _roots(maps, connectivity, num_classes=C):
    import mmsa
    got = mmsa.components(_dev(np.stack(maps)), num_classes=num_classes, connectivity=connectivity)
    assert got.dtype == torch.int32 and tuple(got.shape) == (len(maps),) + maps[0].shape
    return _host(got)


# ---- 1. the roots

@pytest.mark.parametrize("connectivity", [4, 8])
@pytest.mark.parametrize("H,W", SHAPES)
def test_roots_of_noise_and_blocky_maps(H, W, connectivity):
    for kind in ("noise", "blocky", "special"):
        got = _roots([_map(kind, H, W)], connectivity)
        assert np.array_equal(got[0], _want_roots(kind, H, W, connectivity)), kind


@pytest.mark.parametrize("connectivity", [4, 8])
def test_roots_of_the_long_chains_and_the_late_merges(connectivity):
    for kind, H, W in (("serpentine", 67, 131), ("spiral", 67, 131), ("comb", 67, 131), ("staircase", 67, 131), ("serpentine", 130, 200), ("spiral", 130, 200),
                       ("comb", 130, 200), ("staircase", 130, 200), ("serpentine", 31, 63), ("spiral", 31, 63)):
        got = _roots([_map(kind, H, W)], connectivity)
        assert np.array_equal(got[0], _want_roots(kind, H, W, connectivity)), (kind, H, W)
    # what the shapes are there for: the path is ONE component rooted at the corner; the teeth are one component at either connectivity; the diagonal is one
    # component at 8 and H components at 4
    assert (_want_roots("spiral", 130, 200, connectivity)[_map("spiral", 130, 200) == 1] == 0).all()
    assert (_want_roots("comb", 67, 131, connectivity)[_map("comb", 67, 131) == 1] == 0).all()
    assert len(np.unique(_want_roots("staircase", 67, 131, connectivity)[_map("staircase", 67, 131) == 1])) == (1 if connectivity == 8 else 67)


@pytest.mark.parametrize("connectivity", [4, 8])
def test_two_different_images_in_a_batch(connectivity):
    H, W = 96, 160
    maps = [_map("blocky", H, W), np.full((H, W), 7, dtype=np.uint8)]
    got = _roots(maps, connectivity)
    assert np.array_equal(got[0], _want_roots("blocky", H, W, connectivity)) and not got[1].any()      # one code: every pixel hangs under pixel 0 of ITS image
    got = _roots(maps[::-1] + [_map("noise", H, W)], connectivity)
    assert not got[0].any() and np.array_equal(got[1], _want_roots("blocky", H, W, connectivity)) and np.array_equal(got[2], _want_roots("noise", H, W, connectivity))


def test_the_special_codes_of_a_class_map():
    m = _map("special", 67, 131)
    r = _want_roots("special", 67, 131, 4)
    assert len({int(r[y, x]) for y, x in ((67 // 5, 131 // 4), (67 // 2, 131 // 2 + 3), (67 // 2 + 1, 0))}) == 1      # the bytes C, 255 and C + 3 are ONE code, and touch
    assert len(np.unique(m[r == r[67 // 2 + 1, 0]])) == 3
    # with another class count the byte C is a class of its own
    got = _roots([m], 8, num_classes=C + 2)
    assert np.array_equal(got[0], _want_roots("special", 67, 131, 8, C + 2)) and not np.array_equal(got[0], _want_roots("special", 67, 131, 8))


@pytest.mark.parametrize("connectivity", [4, 8])
def test_the_label_side(connectivity):
    import mmsa
    from mmsa.evaluate import LabelPrep
    rng = np.random.default_rng(77)
    label = np.stack([CR.blocky(rng, 50, 90, 8, 3, 9), rng.integers(0, 8, size=(50, 90)).astype(np.uint8)])
    label[0, 10:20, 30:60] = 255
    label[1, 30:35, :] = 255
    label[0, 40:, :20] = 40                                                # beyond the classes: the code C
    H, W = 67, 131
    for kw in (dict(reduce_zero_label=True, label_map={3: 1, 5: 255}), dict()):
        lp = LabelPrep(6, resize=dict(seg_scale=(W, H), keep_ratio=False), **kw)
        got = mmsa.components(_dev(label), labels_prep=lp, connectivity=connectivity)
        assert tuple(got.shape) == (2, H, W)
        ymap, xmap = ER.nearest_index(50, H), ER.nearest_index(90, W)
        for b in range(2):
            L = BR.codes(np.zeros((H, W), dtype=np.uint8), label[b], ER.lut(6, **kw), 6, ymap, xmap)[0]
            assert (L == 255).any() and (L == 6).any()
            assert np.array_equal(_host(got[b]), CR.roots(L, connectivity)), (kw, b)
    same = mmsa.components(_dev(label), labels_prep=LabelPrep(6), size=(50, 90), connectivity=connectivity)      # no tables
    L = BR.codes(np.zeros((50, 90), dtype=np.uint8), label[1], ER.lut(6), 6)[0]
    assert np.array_equal(_host(same[1]), CR.roots(L, connectivity))


def test_determinism_and_out():
    import mmsa
    for kind in ("spiral", "noise"):
        d = _dev(_map(kind, 130, 200)[None])
        a = mmsa.components(d, num_classes=C)
        out = torch.full((1, 130, 200), -7, dtype=torch.int32, device=DEV)
        b = mmsa.components(d, num_classes=C, out=out)
        torch.cuda.synchronize()
        assert b is out and _host(a).tobytes() == _host(b).tobytes() == _want_roots(kind, 130, 200, 8).tobytes()
    with pytest.raises(RuntimeError, match=r"out must be a contiguous int32 \(1, 130, 200\) tensor"):
        mmsa.components(d, num_classes=C, out=out[:, :100])


# ---- 2. areas and suppression

@pytest.mark.parametrize("H,W", [(1, 257), (31, 63), (67, 131), (130, 200)])
def test_areas(H, W):
    import mmsa
    for kind in ("noise", "blocky", "serpentine"):      # 64 distinct roots in a wave; a few; one root for half the map
        want_r = np.stack([_want_roots(kind, H, W, 8), _want_roots(kind, H, W, 4)])
        root = mmsa.components(_dev(np.stack([_map(kind, H, W)] * 2)), num_classes=C)
        root[1].copy_(_dev(want_r[1]))                 # two different root maps in the batch
        area = mmsa.component_areas(root)
        assert area.dtype == torch.int32 and np.array_equal(_host(area), CR.areas(want_r)), kind
        assert area.sum((1, 2)).tolist() == [H * W, H * W]
        assert torch.equal(area != 0, root == torch.arange(H * W, device=DEV, dtype=torch.int32).view(1, H, W))      # non-zero exactly at the roots
        again = torch.full_like(area, 9)
        assert mmsa.component_areas(root, out=again) is again and torch.equal(again, area)      # the plane is zeroed by the entry


@pytest.mark.parametrize("connectivity", [4, 8])
def test_suppress_small(connectivity):
    import mmsa
    H, W = 67, 131
    pred = np.stack([_map("noise", H, W) % 3, _map("special", H, W)])
    d = _dev(pred)
    for min_area in (1, 2, 17, H * W + 1):
        want = CR.suppress(pred, C, min_area, connectivity)
        got = mmsa.suppress_small(d, min_area, num_classes=C, connectivity=connectivity)
        assert got.dtype == torch.uint8 and got.data_ptr() != d.data_ptr() and np.array_equal(_host(got), want), min_area
        if min_area == 1:
            assert np.array_equal(want, pred)          # the identity
        if min_area == H * W + 1:
            assert (want == 255).all()
        out, root, area = torch.empty_like(d), torch.empty(2, H, W, dtype=torch.int32, device=DEV), torch.empty(2, H, W, dtype=torch.int32, device=DEV)
        assert mmsa.suppress_small(d, min_area, num_classes=C, connectivity=connectivity, fill=200, out=out, root=root, area=area) is out
        assert np.array_equal(_host(out), CR.suppress(pred, C, min_area, connectivity, fill=200))
        assert np.array_equal(_host(root), CR.roots_batch(np.minimum(pred, C), connectivity)) and np.array_equal(_host(area), CR.areas(_host(root)))
        inplace = d.clone()
        assert mmsa.suppress_small(inplace, min_area, num_classes=C, connectivity=connectivity, out=inplace) is inplace and np.array_equal(_host(inplace), want)
    assert (want != pred).any() and 0 < (CR.suppress(pred, C, 17, connectivity) == 255).sum() < pred.size


# ---- 3. the segment counts

def _seg_case(kind, H=67, W=131, Cn=6):
    """(pred, label) uint8 [2, H, W]."""
    rng = np.random.default_rng(len(kind) + H)
    label = np.stack([CR.blocky(rng, H, W, Cn, 4, 15), CR.blocky(rng, H, W, Cn, 9, 30)])
    label[0, 5:20, 40:60] = 255                            # ignored regions
    label[1, 30:33, :] = 255
    label[1, 50:, 100:] = Cn + 4                           # kept, out of range: the code C
    if kind == "same":
        pred = np.where(label == 255, 2, label).astype(np.uint8)
    elif kind == "shifted":
        pred = np.minimum(np.roll(label, (3, 5), (1, 2)), Cn + 1).astype(np.uint8)
    else:
        pred = rng.integers(0, Cn + 1, size=label.shape).astype(np.uint8)
        pred[0, :20] = label[0, :20]
    return pred, label


def _segments(pred, label, Cn, bins, connectivity=8, slots=None, counts=None, **kw):
    import mmsa
    from mmsa.evaluate import LabelPrep
    lp = LabelPrep(Cn, **kw)
    dp, dl = _dev(pred), _dev(label)
    rp = mmsa.components(dp, num_classes=Cn, connectivity=connectivity)
    rl = mmsa.components(dl, labels_prep=lp, connectivity=connectivity)
    scratch = torch.full((4,) + pred.shape, 5, dtype=torch.int32, device=DEV)
    got = mmsa.segment_counts(dp, dl, lp, rp, rl, bins, counts=counts, scratch=scratch, slots=slots)
    return got, scratch, lp, dp, dl


@pytest.mark.parametrize("bins", [1, 10, 64])
@pytest.mark.parametrize("kind", ["same", "shifted", "noise"])
def test_segment_counts(kind, bins):
    import mmsa
    Cn = 6
    pred, label = _seg_case(kind)
    got, scratch, lp, dp, dl = _segments(pred, label, Cn, bins)
    want, planes, _, _ = CR.segment_counts(pred, label, ER.lut(Cn), Cn, bins)
    assert got.dtype == torch.int64 and tuple(got.shape) == (2, 2, Cn, 24, bins + 1)
    assert np.array_equal(_host(got), want) and np.array_equal(_host(scratch), planes)
    conf = _host(mmsa.confusion(dp, dl, lp))
    s = _host(scratch).reshape(4, -1).sum(1)
    assert s[0] == s[2] == conf.sum() and s[1] == s[3] == sum(np.trace(c[:Cn, :Cn]) for c in conf)
    codes = [BR.codes(pred[b], label[b], ER.lut(Cn), Cn)[0] for b in range(2)]
    n_label = [sum(len(np.unique(CR.roots(L, 8)[L == c])) for L in codes) for c in range(Cn)]      # the label components of every class, by the restatement
    assert _host(got)[:, 0].sum((0, -1, -2)).tolist() == n_label and min(n_label) > 0
    if kind == "same":
        assert not _host(got)[:, 0, :, :, :bins].any() and not _host(got)[:, 1, :, :, :bins].any()      # every segment lands in the last bin
    else:
        assert _host(got)[..., :bins].any()
    twice = mmsa.segment_counts(dp, dl, lp, mmsa.components(dp, num_classes=Cn), mmsa.components(dl, labels_prep=lp), bins, counts=got.clone())
    assert torch.equal(twice, 2 * got)                     # the call ADDS


@pytest.mark.parametrize("connectivity", [4, 8])
def test_segment_counts_label_side_slots_and_connectivity(connectivity):
    Cn = 6
    pred, label = _seg_case("shifted")
    kw = dict(reduce_zero_label=True, label_map={4: 255})
    got, scratch, _, _, _ = _segments(pred, label, Cn, 10, connectivity, slots=[2, 2], **kw)
    want, planes, _, _ = CR.segment_counts(pred, label, ER.lut(Cn, **kw), Cn, 10, connectivity, slots=[2, 2])
    assert tuple(got.shape) == (3, 2, Cn, 24, 11) and np.array_equal(_host(got), want) and np.array_equal(_host(scratch), planes) and not _host(got)[:2].any()
    # the labels through the tables: 40 x 70 labels against a 67 x 131 prediction
    import mmsa
    from mmsa.evaluate import LabelPrep
    small = _seg_case("noise", 40, 70)[1]
    lp = LabelPrep(Cn, resize=dict(seg_scale=(131, 67), keep_ratio=False))
    dp, dl = _dev(pred), _dev(small)
    rp, rl = mmsa.components(dp, num_classes=Cn, connectivity=connectivity), mmsa.components(dl, labels_prep=lp, connectivity=connectivity)
    got = mmsa.segment_counts(dp, dl, lp, rp, rl, 10, slots=[1, 0])
    want = CR.segment_counts(pred, small, ER.lut(Cn), Cn, 10, connectivity, ER.nearest_index(40, 67), ER.nearest_index(70, 131), slots=[1, 0])[0]
    assert np.array_equal(_host(got), want)


def test_segment_evaluator_adds_what_segment_counts_counts_and_allocates_once():
    import mmsa
    from mmsa.dist import allreduce_counts
    from mmsa.evaluate import LabelPrep, SegmentEvaluator
    Cn = 6
    pred, label = _seg_case("noise")
    lp = LabelPrep(Cn)
    dp, dl = _dev(pred), _dev(label)
    for connectivity, bins in ((8, 10), (4, 7)):
        want = CR.segment_counts(pred, label, ER.lut(Cn), Cn, bins, connectivity)[0]
        se = SegmentEvaluator(lp, bins=bins, connectivity=connectivity, images=6, device=DEV)
        assert se.counts is not None and se.add(dp, dl) is se and se.used == 2 and np.array_equal(se.host_counts(), want)
        rp, rl = mmsa.components(dp, num_classes=Cn, connectivity=connectivity), mmsa.components(dl, labels_prep=lp, connectivity=connectivity)
        assert torch.equal(se.counts[:2], mmsa.segment_counts(dp, dl, lp, rp, rl, bins))
        del rp, rl
        torch.cuda.synchronize()
        before = torch.cuda.memory_allocated()
        se.add(dp, dl)
        torch.cuda.synchronize()
        assert torch.cuda.memory_allocated() == before and se.used == 4      # the second add of a shape allocates nothing
        assert np.array_equal(se.host_counts()[2:], want) and allreduce_counts(se.counts) is se.counts
        assert np.array_equal(se.recall(1.0), mmsa.segment_rate_of(want.sum(0), 0, 1.0), equal_nan=True) and se.summary()["label_segments"] == 2 * want[:, 0].sum()
    cases = SegmentEvaluator(lp, cases=["fog", "night"], device=DEV)
    cases.add(dp, dl, case="night").add(dp[:1], dl[:1], case="fog")
    want = CR.segment_counts(pred, label, ER.lut(Cn), Cn, 10)[0]
    assert np.array_equal(cases.host_counts(), np.stack([want[0], want.sum(0)]))
    same = SegmentEvaluator(lp, images=2, device=DEV).add(dl.where(dl != 255, dl.new_tensor(1)).clamp(max=Cn), dl)      # the prediction is the labels
    assert (same.recall(1.0)[~np.isnan(same.recall(1.0))] == 1.0).all() and same.summary()["mSR"] == 1.0 and same.summary()["mSP"] == 1.0


# ---- 4. the entries on the tiny model

def test_entries_count_the_returned_map(models):  # noqa: F811
    import mmsa.inference as inf
    from mmsa.evaluate import Evaluator, LabelPrep, SegmentEvaluator
    cfg, m, h, frame, x = models
    lp = LabelPrep(NUM_CLASSES)
    g = torch.Generator().manual_seed(12)

    def labels(shape):
        coarse = torch.randint(0, NUM_CLASSES, (shape[0], (shape[1] + 15) // 16, (shape[2] + 15) // 16), generator=g, dtype=torch.uint8)
        lab = coarse.repeat_interleave(16, 1).repeat_interleave(16, 2)[:, :shape[1], :shape[2]].contiguous()
        lab[torch.rand(shape, generator=g) < 0.03] = 255
        return lab.to(DEV)

    def fresh():
        return SegmentEvaluator(lp, images=4, device=DEV)

    def direct(cm, lab):
        import mmsa
        return mmsa.segment_counts(cm, lab, lp, mmsa.components(cm, num_classes=NUM_CLASSES), mmsa.components(lab, labels_prep=lp))

    plain = inf.whole_class_map(m, h, x, ori_shape=(200, 310))
    lab = labels(plain.shape)
    se, ev = fresh(), Evaluator(lp, images=4, device=DEV)
    cm = inf.whole_class_map(m, h, x, ori_shape=(200, 310), labels=lab, evaluator=ev, segments=se)
    assert torch.equal(cm, plain) and se.used == 2 and torch.equal(se.counts[:2], direct(cm, lab)) and int(se.counts.sum()) > 0
    assert torch.equal(inf.whole_class_map(m, h, x, ori_shape=(200, 310), segments=None), plain)
    plain = inf.slide_class_map(m, h, frame, (256, 256), (170, 170), max_batch=2)[0]
    lab = labels(plain.shape)
    se = fresh()
    cm = inf.slide_class_map(m, h, frame, (256, 256), (170, 170), max_batch=2, labels=lab, segments=se)[0]
    assert torch.equal(cm, plain) and se.used == 1 and torch.equal(se.counts[:1], direct(cm, lab)) and int(se.counts.sum()) > 0
    assert torch.equal(inf.slide_class_map(m, h, frame, (256, 256), (170, 170), max_batch=2, segments=None)[0], plain)
    # the refusals, under the entry's name
    with pytest.raises(RuntimeError, match="mmsa.whole_class_map: segments= needs labels="):
        inf.whole_class_map(m, h, x, segments=se)
    with pytest.raises(RuntimeError, match="mmsa.slide_class_map: segments= with return_map=False"):
        inf.slide_class_map(m, h, frame, (256, 256), (170, 170), labels=lab, evaluator=ev, segments=se, return_map=False)
    with pytest.raises(RuntimeError, match="mmsa.slide_class_map: segments= takes an mmsa.evaluate.SegmentEvaluator, got Evaluator"):
        inf.slide_class_map(m, h, frame, (256, 256), (170, 170), labels=lab, segments=ev)
    assert se.used == 1                                    # a refused call has taken no slot
