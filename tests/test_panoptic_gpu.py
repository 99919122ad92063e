"""Panoptic quality on the GPU (csrc/pairs.hip): the pair table as a sorted multiset, the match planes and the counts against the numpy restatement of
tests/panoptic_ref.py, byte for byte.  Everything is integers: every comparison is equality.  The inputs are panoptic_ref.gpu_cases() -- one pixel, a few
pixels, exactly one 64 x 32 tile, ragged tiles, several tiles; one and three images; both connectivities -- whose tables tests/test_panoptic_cpu.py has
predicted: none of them can drop a key, except the one that must.  Then the identities that tie the table to the area planes and the counts to
SegmentEvaluator's, the evaluator, and the entries on the tiny model."""
import functools
from fractions import Fraction

import numpy as np
import pytest
import torch

from tests import components_ref as CR
from tests import panoptic_ref as PR
from tests.test_topk_gpu import NUM_CLASSES, SLIDE_CFG, models  # noqa: F401  (the tiny model of the entry tests, a module-scoped fixture)

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CASES = PR.gpu_cases()


def _dev(a):
    return torch.from_numpy(np.array(a)).to(DEV)      # a copy: the cached cases are read-only


def _host(t):
    return t.cpu().numpy()


def _prep(C, kw, label, H, W):
    from mmsa.evaluate import LabelPrep
    if label.shape[1:] != (H, W):
        kw = dict(kw, resize=dict(seg_scale=(W, H), keep_ratio=False))
    return LabelPrep(C, **kw)


@functools.lru_cache(maxsize=None)
def _want(name, H, W, connectivity):
    """The restatement of one case, computed once and shared."""
    pred, label, C, kw, _ = PR.case(name, H, W)
    ymap, xmap = PR.tables_of(label, H, W)
    return PR.panoptic(pred, label, PR.lut_of(C, kw), C, connectivity, ymap, xmap)


def _run(name, H, W, connectivity, capacity=None):
    """The functional path on the device -> (table, planes, match, counts, root_pred, root_label, the case)."""
    import mmsa
    pred, label, C, kw, _ = PR.case(name, H, W)
    lp = _prep(C, kw, label, H, W)
    dp, dl = _dev(pred), _dev(label)
    rp = mmsa.components(dp, num_classes=C, connectivity=connectivity)
    rl = mmsa.components(dl, labels_prep=lp, size=(H, W), connectivity=connectivity)
    planes = torch.full((4,) + pred.shape, 5, dtype=torch.int32, device=DEV)
    mmsa.segment_counts(dp, dl, lp, rp, rl, 1, scratch=planes)
    table = mmsa.segment_pairs(dp, dl, lp, rp, rl, capacity=capacity)
    match = torch.full((2,) + pred.shape, 7, dtype=torch.int32, device=DEV)
    counts = mmsa.panoptic_counts(dp, dl, lp, rp, rl, planes, table, match=match)
    return table, planes, match, counts, rp, rl, (dp, dl, lp, C)


def _id(c):
    return f"{c[0]}-{c[1]}x{c[2]}-c{c[3]}" + (f"-cap{c[4]}" if c[4] else "")


# ---- 1. table, match and counts against the restatement

@pytest.mark.parametrize("case", [c for c in CASES if not c[-1]], ids=_id)
def test_table_match_and_counts_equal_the_restatement(case):
    name, H, W, connectivity, capacity, _ = case
    want = _want(name, H, W, connectivity)
    table, planes, match, counts, rp, rl, (dp, dl, lp, C) = _run(name, H, W, connectivity, capacity)
    B = dp.shape[0]
    assert table.capacity == (capacity or PR.default_capacity(B * H * W)) and int(table.overflow.item()) == 0
    assert np.array_equal(_host(rp), want["root_pred"]) and np.array_equal(_host(rl), want["root_label"]) and np.array_equal(_host(planes), want["planes"])
    # the table as a sorted multiset: every key once, with its intersection
    keys, inter = _host(table.keys), _host(table.counts)
    used = keys != -1
    assert not inter[~used].any()
    order = np.argsort(keys[used])
    assert keys[used][order].tobytes() == want["keys"].tobytes() and inter[used][order].astype(np.int64).tobytes() == want["inter"].tobytes()
    # the occupied slots are the ones an unbounded linear-probing table of these keys occupies, whatever the order of arrival
    assert np.array_equal(np.nonzero(used)[0], PR.table_prediction(want["keys"], table.capacity)["occupied"])
    img, g, p, n = table.host()
    assert np.array_equal((img * H * W + g) << 31 | p, want["keys"]) and np.array_equal(n, want["inter"]) and (img < B).all()
    assert match.dtype == torch.int32 and _host(match).tobytes() == want["match"].tobytes()
    assert counts.dtype == torch.int64 and tuple(counts.shape) == (B, C, 24, 4) and _host(counts).tobytes() == want["counts"].tobytes()
    # identities on the device results: the table grouped by label root IS plane hit0, grouped by prediction root plane hit1
    pl = _host(planes).reshape(4, -1)
    hit0, hit1 = np.zeros_like(pl[1]), np.zeros_like(pl[3])
    np.add.at(hit0, img * H * W + g, n)
    np.add.at(hit1, img * H * W + p, n)
    assert np.array_equal(hit0, pl[1]) and np.array_equal(hit1, pl[3])
    m = _host(match).reshape(2, B, -1)
    for b in range(B):                                       # match[0] and match[1] are inverse to each other
        at = np.nonzero(m[0, b] >= 0)[0]
        assert np.array_equal(m[1, b][m[0, b][at]], at) and (m[1, b] >= 0).sum() == len(at)
    assert _host(counts)[..., 0].sum() == (m[0] >= 0).sum()


def test_what_the_maps_are_there_for():
    """The cases do what the list says they do -- read from the device results of the larger shapes."""
    import mmsa
    H, W = 70, 45
    _, _, _, counts, _, _, (_, _, _, C) = _run("same", H, W, 8)
    c = _host(counts).sum((0, 2))
    assert c[:, 0].sum() > 10 and not c[:, 1:3].any() and c[:, 3].tolist() == (c[:, 0] << 24).tolist()      # all TP, every q = 2^24
    q = mmsa.panoptic_quality_of(_host(counts).sum(0))
    assert (q["pq"][c[:, 0] > 0] == 1.0).all() and mmsa.panoptic_summary_of(_host(counts).sum(0))["PQ"] == 1.0
    for conn in (4, 8):
        c = _host(_run("blobs", H, W, conn)[3])[0].sum(1)
        assert c[1].tolist() == [0, 1, 1, 0] and c[2].tolist() == [1, 0, 0, (2 << 24) // 3] and c[3].tolist() == [0, 1, 2, 0] and c[4].tolist() == [0, 2, 1, 0]
    # whole waves share one pair: far fewer keys than waves
    table = _run("patchy", 130, 97, 8)[0]
    assert 0 < int((table.keys != -1).sum()) < 3 * 130 * 97 // 64 // 4
    # every pixel its own pair
    table = _run("checker", H, W, 4, 2 * PR.default_capacity(4 * H * W))[0]
    assert int((table.keys != -1).sum()) == H * W and int(table.counts.max()) == 1
    # a blob wholly inside an ignored region has area_p == 0 and counts nowhere; area_p excludes ignored pixels elsewhere
    table, planes, match, counts, rp, rl, (dp, dl, lp, C) = _run("ignored", H, W, 8)
    y, x = H // 4 + 4, W // 4 + 4
    root = int(rp[0, y, x])
    assert int(dp[0, y, x]) == 5 and int(planes[2, 0].view(-1)[root]) == 0 and int(match[1, 0].view(-1)[root]) == -1
    area_all = _host(mmsa.component_areas(rp))
    assert (_host(planes[2]) < area_all).any() and (_host(planes[2]) <= area_all).all()
    want = _want("ignored", H, W, 8)
    assert np.array_equal(_host(counts), want["counts"]) and (dl == 40).any()      # a kept label out of range is the code C: counted nowhere, matched by nothing
    # the label side through LUT and tables changes the result: the same bytes read without them differ
    assert _run("lut", H, W, 8)[6][1].shape[1:] != (H, W)


# ---- 2. overflow: the bounded loop gives up, and nothing reports from a short table

def test_a_table_that_is_too_small_overflows_and_is_refused():
    import mmsa
    name, H, W, connectivity, capacity, overflows = [c for c in CASES if c[-1]][0]
    assert capacity == 2 and overflows
    table, planes, match, counts, rp, rl, (dp, dl, lp, C) = _run(name, H, W, connectivity, capacity)
    torch.cuda.synchronize()
    lost = int(table.overflow.item())
    assert lost > 0 and lost + int(table.counts.sum()) == H * W and int((table.keys != -1).sum()) == 2      # every hit pixel is in the table or in the word
    with pytest.raises(RuntimeError, match="the pair table of 2 slots overflowed"):
        table.host()
    pe = mmsa.PanopticEvaluator(lp, connectivity=connectivity, capacity=2, device=DEV)
    pe.add(dp, dl)
    assert pe.overflow() == lost
    for read in (pe.summary, pe.host_counts, pe.pq, pe.sq, pe.rq, pe.by_size):
        with pytest.raises(RuntimeError, match=r"mmsa.PanopticEvaluator: a pair table overflowed \(\d+ hit pixels found no slot\).*capacity="):
            read()
    pe.reset()
    assert pe.overflow() == 0 and pe.host_counts().shape == (0, C, 24, 4)
    again = mmsa.segment_pairs(dp, dl, lp, rp, rl, table=table)      # table= keeps adding to the word
    assert again is table and int(table.overflow.item()) == 2 * lost
    with pytest.raises(ValueError, match="capacity = 6 is not a power of two.*4 and 8"):
        mmsa.segment_pairs(dp, dl, lp, rp, rl, capacity=6)


# ---- 3. the evaluator

@pytest.mark.parametrize("connectivity", [4, 8])
def test_evaluator_equals_the_restatement_and_segment_evaluator(connectivity):
    import mmsa
    from mmsa.dist import allreduce_counts
    H, W = 130, 97
    for name in ("shifted", "ignored", "lut"):
        pred, label, C, kw, _ = PR.case(name, H, W)
        want = _want(name, H, W, connectivity)
        lp = _prep(C, kw, label, H, W)
        dp, dl = _dev(pred), _dev(label)
        pe = mmsa.PanopticEvaluator(lp, connectivity=connectivity, images=8, device=DEV)
        assert pe.add(dp, dl) is pe and pe.used == pred.shape[0] and pe.overflow() == 0
        assert pe.host_counts().tobytes() == want["counts"].tobytes() and allreduce_counts(pe.counts) is pe.counts
        se = mmsa.SegmentEvaluator(lp, bins=1, connectivity=connectivity, images=8, device=DEV).add(dp, dl)
        sides = se.host_counts().sum(-1)                     # [n, 2, C, 24]
        c = pe.host_counts()
        assert np.array_equal(c[..., 0] + c[..., 2], sides[:, 0])                       # TP + FN per (class, bucket) IS the label side
        assert np.array_equal((c[..., 0] + c[..., 1]).sum(-1), sides[:, 1].sum(-1))     # sum over buckets of TP + FP per class IS the prediction side
        assert torch.equal(pe._sides[:pe.used], se.counts[:se.used])
        # SQ within 2^-24 of the Fraction mean, PQ = SQ * RQ within the same
        q = pe.quality()
        for cls in range(C):
            ious = [i for cc, i in want["ious"] if cc == cls]
            if ious:
                exact = sum(ious) / len(ious)
                assert -Fraction(1, 1 << 50) <= exact - Fraction(q["sq"][cls]) < Fraction(1, 1 << 24) + Fraction(1, 1 << 50)
                assert abs(q["pq"][cls] - q["sq"][cls] * q["rq"][cls]) < 1e-15
        assert np.array_equal(pe.pq(), q["pq"], equal_nan=True) and pe.summary()["tp"] == int(c[..., 0].sum())
        assert np.array_equal(pe.by_size()["tp"].sum(0), q["tp"])


def test_evaluator_is_deterministic_uses_case_slots_and_allocates_once():
    import mmsa
    H, W = 70, 45
    pred, label, C, kw, _ = PR.case("shifted", H, W)
    want = _want("shifted", H, W, 8)["counts"]
    lp = _prep(C, kw, label, H, W)
    dp, dl = _dev(pred), _dev(label)
    runs = [_run("shifted", H, W, 8) for _ in range(2)]
    assert _host(runs[0][3]).tobytes() == _host(runs[1][3]).tobytes() and _host(runs[0][2]).tobytes() == _host(runs[1][2]).tobytes()
    pe = mmsa.PanopticEvaluator(lp, images=8, device=DEV)
    pe.add(dp, dl)
    torch.cuda.synchronize()
    before = torch.cuda.memory_allocated()
    pe.add(dp, dl)
    torch.cuda.synchronize()
    assert torch.cuda.memory_allocated() == before and pe.used == 6      # the second add of a shape allocates nothing
    assert np.array_equal(pe.host_counts()[3:], want) and np.array_equal(pe.host_counts()[:3], want)
    cases = mmsa.PanopticEvaluator(lp, cases=["fog", "night"], things=[0, 1, 2], device=DEV)
    cases.add(dp, dl, case="night").add(dp[:1], dl[:1], case="fog")
    assert np.array_equal(cases.host_counts(), np.stack([want[0], want.sum(0)]))
    assert np.array_equal(cases.pq(slot="fog"), mmsa.panoptic_quality_of(want[0])["pq"], equal_nan=True)
    s = cases.summary(slot="night")
    assert s == dict(mmsa.panoptic_summary_of(want.sum(0), things=[0, 1, 2]), connectivity=8) and "PQ_th" in s
    slots = mmsa.PanopticEvaluator(lp, images=4, device=DEV)
    slots.add(dp, dl, slots=[3, 3, 1])
    assert slots.used == 0 and np.array_equal(_host(slots.counts), np.stack([0 * want[0], want[2], 0 * want[0], want[0] + want[1]]))
    # the functional call ADDS
    t = runs[0]
    twice = mmsa.panoptic_counts(t[6][0], t[6][1], lp, t[4], t[5], t[1], t[0], counts=t[3].clone())
    assert torch.equal(twice, 2 * t[3])
    with pytest.raises(RuntimeError, match=r"match must be a contiguous int32 \(2, 3, 70, 45\) tensor"):
        mmsa.panoptic_counts(t[6][0], t[6][1], lp, t[4], t[5], t[1], t[0], match=t[2][:1])
    with pytest.raises(RuntimeError, match="planes must be a contiguous int32 tensor of at least"):
        mmsa.panoptic_counts(t[6][0], t[6][1], lp, t[4], t[5], t[1][:2], t[0])


# ---- 4. the entries on the tiny model

def test_entries_count_the_returned_map(models):  # noqa: F811
    import mmsa
    import mmsa.inference as inf
    from mmsa.evaluate import LabelPrep, PanopticEvaluator, SegmentEvaluator
    cfg, m, h, frame, x = models
    lp = LabelPrep(NUM_CLASSES)
    g = torch.Generator().manual_seed(12)

    def labels(shape):
        coarse = torch.randint(0, NUM_CLASSES, (shape[0], (shape[1] + 15) // 16, (shape[2] + 15) // 16), generator=g, dtype=torch.uint8)
        lab = coarse.repeat_interleave(16, 1).repeat_interleave(16, 2)[:, :shape[1], :shape[2]].contiguous()
        lab[torch.rand(shape, generator=g) < 0.03] = 255
        return lab.to(DEV)

    def fed(cm, lab):
        return PanopticEvaluator(lp, images=4, device=DEV).add(cm, lab)

    plain = inf.whole_class_map(m, h, x, ori_shape=(200, 310))
    lab = labels(plain.shape)
    pe, se = PanopticEvaluator(lp, images=4, device=DEV), SegmentEvaluator(lp, images=4, device=DEV)
    cm = inf.whole_class_map(m, h, x, ori_shape=(200, 310), labels=lab, segments=se, panoptic=pe)
    assert torch.equal(cm, plain) and pe.used == 2 and se.used == 2 and pe.overflow() == 0
    assert torch.equal(pe.counts, fed(cm, lab).counts) and int(pe.counts[..., :3].sum()) > 0
    assert torch.equal(inf.whole_class_map(m, h, x, ori_shape=(200, 310), panoptic=None), plain)
    plain = inf.slide_class_map(m, h, frame, (256, 256), (170, 170), max_batch=2)[0]
    lab = labels(plain.shape)
    pe = PanopticEvaluator(lp, images=4, device=DEV)
    cm = inf.slide_class_map(m, h, frame, (256, 256), (170, 170), max_batch=2, labels=lab, panoptic=pe)[0]
    assert torch.equal(cm, plain) and pe.used == 1 and torch.equal(pe.counts, fed(cm, lab).counts) and int(pe.counts[..., :3].sum()) > 0
    want = PR.panoptic(_host(cm), _host(lab), PR.lut_of(NUM_CLASSES, {}), NUM_CLASSES, 8)["counts"]
    assert np.array_equal(pe.host_counts(), want)
    # the refusals, under the entry's name
    with pytest.raises(RuntimeError, match="mmsa.whole_class_map: panoptic= needs labels="):
        inf.whole_class_map(m, h, x, panoptic=pe)
    with pytest.raises(RuntimeError, match="mmsa.slide_class_map: panoptic= with return_map=False"):
        inf.slide_class_map(m, h, frame, (256, 256), (170, 170), labels=lab, evaluator=mmsa.Evaluator(lp, images=4, device=DEV), panoptic=pe, return_map=False)
    with pytest.raises(RuntimeError, match="mmsa.slide_class_map: panoptic= takes an mmsa.evaluate.PanopticEvaluator, got SegmentEvaluator"):
        inf.slide_class_map(m, h, frame, (256, 256), (170, 170), labels=lab, panoptic=se)
    assert pe.used == 1                                    # a refused call has taken no slot
