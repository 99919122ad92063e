"""Panoptic quality without a GPU: the numpy restatement (tests/panoptic_ref.py) against a brute-force statement from sets of pixels and Fractions, the
uniqueness of matches, the host functions on hand-made counts, the capacity refusals, the exports and the ctypes entries -- and, for every input of
tests/test_panoptic_gpu.py, the table the restatement predicts: no key can be dropped there (or must be, where the test wants that)."""
import functools
from fractions import Fraction

import numpy as np
import pytest

from tests import boundary_ref as BR
from tests import components_ref as CR
from tests import panoptic_ref as PR


def _codes(pred, label, C, kw, H, W, b=0):
    ymap, xmap = PR.tables_of(label, H, W)
    return BR.codes(pred[b], label[b], PR.lut_of(C, kw), C, ymap, xmap)


# ---- 1. the restatement against sets of pixels

@pytest.mark.parametrize("connectivity", [4, 8])
@pytest.mark.parametrize("name,H,W", [("blobs", 11, 9), ("same", 9, 13), ("shifted", 12, 17), ("noise", 8, 9), ("ignored", 24, 31), ("lut", 17, 23),
                                      ("checker", 5, 7)])
def test_restatement_equals_the_brute_force_statement(name, H, W, connectivity):
    pred, label, C, kw, _ = PR.case(name, H, W, C=4 if name == "noise" else 25)
    ymap, xmap = PR.tables_of(label, H, W)
    want = PR.panoptic(pred, label, PR.lut_of(C, kw), C, connectivity, ymap, xmap)
    for b in range(pred.shape[0]):
        L, P = _codes(pred, label, C, kw, H, W, b)
        tp, fp, fn, matches = PR.brute_force(L, P, C, connectivity)
        assert np.array_equal(want["counts"][b], PR.counts_of_brute_force(tp, fp, fn, matches, C)), b
        m0 = {g: p for g, p, _ in matches}
        got0 = {int(g): int(p) for g, p in enumerate(want["match"][0, b].ravel()) if p >= 0}
        assert got0 == m0 and {int(p): int(g) for p, g in enumerate(want["match"][1, b].ravel()) if g >= 0} == {p: g for g, p in m0.items()}


def test_the_hand_made_pairs():
    pred, label, C, kw, _ = PR.case("blobs", 11, 9)
    r = PR.panoptic(pred, label, PR.lut_of(C, kw), C, 8)
    c = r["counts"][0].sum(1)                                # [C, 4]
    assert c[1].tolist() == [0, 1, 1, 0]                      # IoU exactly 1/2: no match -- one FP and one FN
    assert c[2].tolist() == [1, 0, 0, (2 << 24) // 3]         # IoU 2/3: a match, q = floor(2^25 / 3)
    assert c[3].tolist() == [0, 1, 2, 0]                      # one blob over two label segments: 6 / 14 each, no match
    assert c[4].tolist() == [0, 2, 1, 0]                      # one label segment under two blobs
    assert c[0, 0] == 1 and c[0, 1] == c[0, 2] == 0           # the background matches itself
    assert sorted(i for _, i in r["ious"])[0] == Fraction(2, 3)


def test_matches_are_unique_on_random_maps():
    rng = np.random.default_rng(5)
    for trial in range(40):
        H, W, C = int(rng.integers(3, 14)), int(rng.integers(3, 14)), int(rng.integers(2, 4))
        label = CR.blocky(rng, H, W, C, 1, 4)
        pred = np.where(rng.random((H, W)) < 0.25, rng.integers(0, C + 1, size=(H, W)), label).astype(np.uint8)
        label = np.where(rng.random((H, W)) < 0.05, 255, label).astype(np.uint8)
        for conn in (4, 8):
            r = PR.panoptic(pred[None], label[None], PR.lut_of(C, {}), C, conn)      # asserts uniqueness while it matches
            m0, m1 = r["match"][0, 0].ravel(), r["match"][1, 0].ravel()
            g = np.nonzero(m0 >= 0)[0]
            assert np.array_equal(m1[m0[g]], g) and (m1 >= 0).sum() == len(g) == r["counts"][..., 0].sum()
            # every candidate of a matched segment beyond its match fails the test: inter1 + inter2 <= area
            for k, n in zip(r["keys"].tolist(), r["inter"].tolist()):
                gg, pp = k >> 31, k & ((1 << 31) - 1)
                ag, ap = int(r["planes"][0, 0].ravel()[gg]), int(r["planes"][2, 0].ravel()[pp])
                assert (3 * n > ap + ag) == (m0[gg] == pp) and n <= min(ag, ap)


# ---- 2. the host functions

def _counts(C=3):
    c = np.zeros((C, 24, 4), dtype=np.int64)
    c[0, 3] = [2, 1, 1, (1 << 24) + (1 << 23)]               # two TPs of IoU 1 and 1/2 (the sum is all that is kept), one FP, one FN, areas 8..15
    c[0, 10] = [1, 0, 0, 1 << 24]
    c[1, 5] = [0, 2, 0, 0]                                   # only FPs: PQ = RQ = 0, SQ = 0 / 0
    return c                                                 # class 2: nothing


def test_quality_from_hand_made_counts():
    import mmsa
    q = mmsa.panoptic_quality_of(_counts())
    assert q["tp"].tolist() == [3, 0, 0] and q["fp"].tolist() == [1, 2, 0] and q["fn"].tolist() == [1, 0, 0]
    assert q["sq"][0] == 2.5 / 3 and q["rq"][0] == 3 / 4 and q["pq"][0] == 2.5 / 4
    assert q["pq"][1] == 0 and q["rq"][1] == 0 and np.isnan(q["sq"][1])
    assert all(np.isnan(q[k][2]) for k in ("pq", "sq", "rq"))
    q = mmsa.panoptic_quality_of(_counts(), min_area=8, max_area=16)
    assert q["tp"].tolist() == [2, 0, 0] and q["pq"][0] == 1.5 / 3 and np.isnan(q["pq"][1])
    assert mmsa.panoptic_quality_of(np.stack([_counts(), 2 * _counts()]))["pq"].shape == (2, 3)
    with pytest.raises(ValueError, match="min_area = 12 is not the edge of a size bucket.*nearest edges are 8 and 16"):
        mmsa.panoptic_quality_of(_counts(), min_area=12)
    with pytest.raises(ValueError, match="max_area = 8 must be above min_area = 8"):
        mmsa.panoptic_quality_of(_counts(), min_area=8, max_area=8)
    with pytest.raises(ValueError, match=r"panoptic counts are an integer \[\.\.\., C, 24, 4\] array"):
        mmsa.panoptic_quality_of(np.zeros((3, 24, 3), dtype=np.int64))
    with pytest.raises(ValueError, match="panoptic counts are an integer"):
        mmsa.panoptic_quality_of(_counts().astype(np.float64))


def test_summary_and_things():
    import mmsa
    s = mmsa.panoptic_summary_of(_counts())
    assert s["PQ"] == round((2.5 / 4 + 0) / 2 * 100, 2) / 100 and s["SQ"] == round(2.5 / 3 * 100, 2) / 100 and s["RQ"] == round(0.75 / 2 * 100, 2) / 100
    assert (s["tp"], s["fp"], s["fn"]) == (3, 3, 1) and "PQ_th" not in s
    s = mmsa.panoptic_summary_of(_counts(), things=[0])
    assert s["PQ_th"] == 0.625 and s["PQ_st"] == 0.0 and s["SQ_th"] == round(2.5 / 3 * 100, 2) / 100 and np.isnan(s["SQ_st"])
    s = mmsa.panoptic_summary_of(_counts(), things=[2])
    assert np.isnan(s["PQ_th"]) and s["PQ_st"] == round(0.3125 * 100, 2) / 100
    assert np.isnan(mmsa.panoptic_summary_of(np.zeros((3, 24, 4), dtype=np.int64))["PQ"])
    for bad in ([3], [0, 0], [], [True], [-1]):
        with pytest.raises(ValueError, match="a list of distinct class indices in 0..2"):
            mmsa.panoptic_summary_of(_counts(), things=bad)
    with pytest.raises(ValueError, match="the counts of one slot"):
        mmsa.panoptic_summary_of(np.stack([_counts(), _counts()]))


def test_sq_lies_within_two_to_the_minus_24_of_the_fraction_mean():
    import mmsa
    pred, label, C, kw, _ = PR.case("shifted", 40, 50)
    r = PR.panoptic(pred, label, PR.lut_of(C, kw), C, 8)
    q = mmsa.panoptic_quality_of(r["counts"].sum(0))
    checked = 0
    for c in range(C):
        ious = [i for cc, i in r["ious"] if cc == c]
        if ious:
            exact = sum(ious) / len(ious)
            assert -Fraction(1, 1 << 50) <= exact - Fraction(q["sq"][c]) < Fraction(1, 1 << 24) + Fraction(1, 1 << 50)      # float64 of the quotient: 2^-53 relative
            checked += 1
    assert checked > 5


# ---- 3. capacity, exports, entries

def test_capacity_refusals():
    import mmsa
    from mmsa.evaluate import LabelPrep, check_pair_capacity, default_pair_capacity
    assert [check_pair_capacity(v) for v in (2, 4, 1 << 20, 1 << 30)] == [2, 4, 1 << 20, 1 << 30]
    with pytest.raises(ValueError, match="capacity = 3 is not a power of two.*neighbouring powers are 2 and 4"):
        check_pair_capacity(3)
    with pytest.raises(ValueError, match="capacity = 1000 is not a power of two.*neighbouring powers are 512 and 1024"):
        check_pair_capacity(1000)
    with pytest.raises(ValueError, match="capacity = 1 is not a power of two"):
        check_pair_capacity(1)
    with pytest.raises(ValueError, match="neighbouring powers are 1073741824 and 1073741824"):
        check_pair_capacity(1 << 31)
    for bad in (0, -4, 2.0, True, None, "8"):
        with pytest.raises(ValueError, match="a number of table slots"):
            check_pair_capacity(bad)
    with pytest.raises(ValueError, match="mmsa.PanopticEvaluator: capacity = 48 is not a power of two.*32 and 64"):
        mmsa.PanopticEvaluator(LabelPrep(25), capacity=48)
    with pytest.raises(ValueError, match="mmsa.PanopticEvaluator: connectivity = 6"):
        mmsa.PanopticEvaluator(LabelPrep(25), connectivity=6)
    with pytest.raises(ValueError, match="things = \\[25\\]"):
        mmsa.PanopticEvaluator(LabelPrep(25), things=[25])
    for n in (1, 2, 3, 4, 5, 35, 2048, 2049, 1080 * 1920, 2 * 1024 * 1024):
        c = default_pair_capacity(n)
        assert c == PR.default_capacity(n) and c >= 2 and 2 * c >= n and (c == 2 or c < n) and c & (c - 1) == 0


def test_an_evaluator_without_a_device_reads_as_empty():
    import mmsa
    from mmsa.evaluate import LabelPrep
    pe = mmsa.PanopticEvaluator(LabelPrep(5), cases=["fog", "night"], things=[1, 2])
    assert pe.counts is None and pe.overflow() == 0 and pe.host_counts().shape == (2, 5, 24, 4) and np.isnan(pe.pq()).all()
    assert np.isnan(pe.summary()["PQ"]) and pe.summary()["connectivity"] == 8 and pe.by_size()["tp"].shape == (24, 5)


def test_exports_and_entries():
    import inspect
    import mmsa
    import mmsa.inference as inf
    for name in ("PanopticEvaluator", "PairTable", "segment_pairs", "panoptic_counts", "panoptic_quality_of", "panoptic_summary_of"):
        assert getattr(mmsa, name) is getattr(mmsa.evaluate, name) and name in mmsa.__all__
    assert mmsa.evaluate.PAIR_MAX_PROBES == PR.MAX_PROBES and mmsa.evaluate.IOU_ONE == PR.IOU_ONE
    for name in ("mmsa_segment_pairs", "mmsa_eval_panoptic"):
        assert name in mmsa.lib.SIGNATURES and hasattr(mmsa.lib.raw, name)
    assert len(mmsa.lib.SIGNATURES["mmsa_segment_pairs"]) == 18 and len(mmsa.lib.SIGNATURES["mmsa_eval_panoptic"]) == 22
    for fn in (inf.slide_class_map, inf.whole_class_map, inf.class_map, inf.aug_class_map, inf.MapPlan.class_map, inf.SlideRunner.run):
        assert inspect.signature(fn).parameters["panoptic"].default is None, fn.__qualname__
    o = inf.MapOptions.of("slide_class_map")
    assert o.panoptic is None
    with pytest.raises(RuntimeError, match="mmsa.slide_class_map: panoptic= takes an mmsa.evaluate.PanopticEvaluator, got int"):
        inf.MapOptions.of("slide_class_map", panoptic=3, labels=object())
    from mmsa.evaluate import LabelPrep
    pe = mmsa.PanopticEvaluator(LabelPrep(5))
    with pytest.raises(RuntimeError, match="mmsa.whole_class_map: panoptic= needs labels="):
        inf.MapOptions.of("whole_class_map", panoptic=pe)
    with pytest.raises(RuntimeError, match="mmsa.whole_class_map: panoptic= with return_map=False"):
        inf.MapOptions.of("whole_class_map", panoptic=pe, labels=object(), return_map=False)


# ---- 4. the tables of the GPU tests, predicted

def test_the_hash_and_the_probe_rule():
    assert PR.slot_of(0, 2) == 0 and PR.slot_of(1, 2) == 1 and PR.slot_of(1, 1 << 30) == 0x9E3779B97F4A7C15 >> 34
    assert PR.slot_of((5 << 31) | 5, 16) == (((5 << 31) | 5) * 0x9E3779B97F4A7C15 % (1 << 64)) >> 60
    # the occupied set does not depend on the order of insertion
    rng = np.random.default_rng(3)
    keys = np.unique(rng.integers(0, 1 << 40, size=200))
    a = PR.table_prediction(keys, 256)
    for _ in range(5):
        b = PR.table_prediction(rng.permutation(keys), 256)
        assert np.array_equal(a["occupied"], b["occupied"]) and a["longest_walk"] == b["longest_walk"]
    assert len(a["occupied"]) == len(keys) and a["overflow_impossible"] and not a["overflow_certain"]
    # a walk is the distance to the first free slot: three keys of one home look at 1, 2, 3 slots
    same_home = [k for k in range(4000) if PR.slot_of(k, 1024) == 7][:3]
    assert PR.table_prediction(same_home, 1024)["longest_walk"] == 3 and PR.table_prediction(same_home[:1], 1024)["longest_walk"] == 1
    full = PR.table_prediction(range(300), 256)
    assert full["overflow_certain"] and not full["overflow_impossible"]
    assert PR.table_prediction(range(2), 2)["overflow_impossible"]      # a full table that dropped nothing


@functools.lru_cache(maxsize=None)
def _keys(name, H, W, connectivity):
    pred, label, C, kw, _ = PR.case(name, H, W)
    ymap, xmap = PR.tables_of(label, H, W)
    return PR.panoptic(pred, label, PR.lut_of(C, kw), C, connectivity, ymap, xmap)["keys"], pred.shape[0]


def test_every_gpu_input_has_the_overflow_its_test_expects():
    cases = PR.gpu_cases()
    assert len(cases) > 50 and sum(c[-1] for c in cases) == 1
    worst = 0
    for name, H, W, connectivity, capacity, overflows in cases:
        keys, B = _keys(name, H, W, connectivity)
        t = PR.table_prediction(keys, capacity or PR.default_capacity(B * H * W))
        assert t["overflow_certain"] if overflows else t["overflow_impossible"], (name, H, W, connectivity, capacity, t["longest_walk"], t["load"])
        if not overflows:
            assert len(t["occupied"]) == len(keys)
            worst = max(worst, t["longest_walk"])
    assert 1 < worst <= PR.MAX_PROBES
    # the checkerboard at 4: every pixel its own pair -- the default capacity could not hold them
    keys, _ = _keys("checker", 32, 64, 4)
    assert len(keys) == 32 * 64 and PR.table_prediction(keys, PR.default_capacity(32 * 64))["overflow_certain"]
