"""Host side of selective evaluation (mmsa.evaluate.selective / abstain / SelectiveEvaluator; no GPU): the numpy restatement (tests/selective_ref.py)
against a brute-force loop in Python integers, the three identities that tie it to the confusion counts (tests/eval_ref.py) and the reliability bins
(tests/calibration_ref.py), the metric functions, SelectiveEvaluator's bookkeeping and refusals, the two entries' declarations and host-side refusals,
and the `selective=` refusals of the inference entries."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from tests import calibration_ref as CR
from tests import eval_ref as ER
from tests import selective_ref as SR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VARIANTS, GPU_PAIRS = SR.VARIANTS, SR.GPU_PAIRS


def _brute(pred, conf, label, C, K, **kw):
    """Pixel by pixel, in Python integers but for the ONE float32 product the bin is defined by."""
    t, keep = ER.transform_bytes(**kw)
    out = [[[0] * (C + 1) for _ in range(C + 1)] for _ in range(K)]
    for p, c, raw in zip(pred.ravel().tolist(), conf.ravel(), label.ravel().tolist()):
        if not keep[raw]:
            continue
        c = np.float32(c)
        if np.isnan(c) or c < 0:
            c = np.float32(0)
        elif c > 1:
            c = np.float32(1)
        k = min(K - 1, int(np.float32(c) * np.float32(K)))
        out[k][min(int(t[raw]), C)][min(p, C)] += 1
    return np.array(out, dtype=np.int64)


@pytest.mark.parametrize("kw", VARIANTS, ids=("plain", "rzl", "map", "ignore0"))
def test_restatement_equals_the_brute_force_loop(kw):
    """A few hundred pixels per case; CR.make_case puts CR.SPECIALS on the first pixels and exact edges j / K on a fifth of the rest."""
    for C, K in ((2, 1), (5, 15), (25, 16), (7, 64)):
        pred, conf, label = CR.make_case(150 + C, 9, 31, C, K, B=2)
        assert np.isnan(conf[0].ravel()[0]) and np.isin(conf[0].ravel()[10:], (np.arange(K + 1) / K).astype(np.float32)).sum() >= 20
        for b in range(2):
            got = SR.counts_of(pred[b], conf[b], label[b], C, K, **kw)
            assert got.dtype == np.int64 and got.shape == (K, C + 1, C + 1)
            assert np.array_equal(got, _brute(pred[b], conf[b], label[b], C, K, **kw)), (C, K, b)
    # the specials alone: NaN, -1, 0, 1e-40, -inf, -0.0 -> bin 0; 2, 1, the float below 1, +inf -> the last bin
    n = len(CR.SPECIALS)
    cls = (np.arange(n) % 5).astype(np.uint8)
    for K in (1, 2, 15, 64):
        got = SR.counts_of(cls, CR.SPECIALS, cls, 5, K)
        want = np.zeros((K, 6, 6), dtype=np.int64)
        for i, k in enumerate((0, 0, K - 1, 0, K - 1, 0, K - 1, K - 1, 0, 0)):
            want[k, cls[i], cls[i]] += 1
        assert np.array_equal(got, want), K


@pytest.mark.parametrize("C,K", GPU_PAIRS)
def test_the_three_identities(C, K):
    """(1) the sum over the bins is the confusion matrix; (2) the rows < C of bin k sum to the calibration's total[k], the trace of its [:C, :C] block is
    correct[k]; (3) the confusion counts of the abstained map are counts[k0:].sum(0) with the row sums of counts[:k0] added into column C."""
    from mmsa.evaluate import reliability_counts_of, selective_counts_of
    H, W = (37, 255) if C < 100 else (37, 1021)
    pred, conf, label = CR.make_case(400 + C + K, H, W, C, K)
    for kw in VARIANTS:
        counts = SR.counts_of(pred[0], conf[0], label[0], C, K, **kw)
        assert np.array_equal(counts.sum(0), ER.confusion(pred[0], label[0], C, **kw))
        bins = CR.bins_of(pred[0], conf[0], label[0], C, K, **kw)
        assert np.array_equal(counts[:, :C, :].sum((1, 2)), bins[0]) and np.array_equal(np.trace(counts[:, :C, :C], axis1=1, axis2=2), bins[1])
        assert np.array_equal(reliability_counts_of(counts), bins[:2])
        for k0 in sorted({0, 1, K // 2, K - 1, K}):
            gated = SR.abstain_of(pred[0], conf[0], K, k0)
            assert np.array_equal(ER.confusion(gated, label[0], C, **kw), SR.abstained_counts(counts, k0)), (kw, k0)
            assert np.array_equal(selective_counts_of(counts, k0), counts[k0:].sum(0))
    counts = SR.counts_of(pred[0], conf[0], label[0], C, K)
    assert counts[:, C, :].any() and counts[:, :, C].any()                  # out-of-range labels and uncovered predictions are in play


@pytest.mark.parametrize("C,K", GPU_PAIRS)
def test_the_gpu_cases_fill_every_bin_with_every_kind_of_pixel(C, K):
    """What tests/test_selective_gpu.py asserts of its W > 1, plain-LUT cases: every bin of every image holds a correct, a wrong and a row-C pixel; and
    the cases cycle every label variant, pointer offset and float4 phase."""
    least, seen = [1 << 60] * 3, set()
    for B, H, W, kw, po, lo, co, seed in SR.gpu_cases(C, K):
        seen.add((tuple(sorted(kw)), po, lo, co))
        if W == 1 or kw:
            continue
        pred, conf, label = CR.make_case(seed, H, W, C, K, B=B)
        for b in range(B):
            c = SR.counts_of(pred[b], conf[b], label[b], C, K)
            good, rowc = np.trace(c[:, :C, :C], axis1=1, axis2=2), c[:, C, :].sum(1)
            wrong = c[:, :C, :].sum((1, 2)) - good
            assert (good > 0).all() and (wrong > 0).all() and (rowc > 0).all(), (C, K, B, W)
            least = [min(a, int(v.min())) for a, v in zip(least, (good, wrong, rowc))]
    print(f"C {C} K {K}: the emptiest bin holds {least[0]} correct / {least[1]} wrong / {least[2]} row-C pixels")
    assert {s[0] for s in seen} == {tuple(sorted(v)) for v in SR.VARIANTS} and {s[3] for s in seen} == {0, 4, 8, 12} and len({s[1:3] for s in seen}) >= 5


def test_selective_metrics_of():
    from mmsa.evaluate import (area_metrics, areas_of, risk_coverage_of, selective_areas_of, selective_counts_of, selective_metrics_of)
    C, K = 7, 10
    for out_of_range, kw in ((None, dict()), (3, dict()), (None, dict(reduce_zero_label=True))):
        # out_of_range=3: the "out of range" label value is a class, so no kept label lies outside [0, C) and row C is empty
        pred, conf, label = CR.make_case(77, 37, 257, C, K, out_of_range=out_of_range)
        counts = SR.counts_of(pred[0], conf[0], label[0], C, K, **kw)
        assert (counts[:, C, :].sum() == 0) == (out_of_range == 3)
        m = selective_metrics_of(counts, metric=("mIoU", "mFscore"))
        assert list(m) == ["coverage", "aAcc", "IoU", "Acc", "Fscore", "Precision", "Recall", "mIoU", "mAcc", "mFscore", "mPrecision", "mRecall"]
        assert m["coverage"].shape == m["aAcc"].shape == m["mIoU"].shape == (K,) and m["IoU"].shape == (K, C) and m["IoU"].dtype == np.float64
        whole = area_metrics(*areas_of(counts.sum(0)), metric=("mIoU", "mFscore"))
        for key, v in whole.items():                                                    # entry 0 is the plain evaluation, exactly
            assert np.array_equal(m[key][0], v, equal_nan=True), key
        assert m["mIoU"][0] == np.nanmean(whole["IoU"])
        for k in range(K):                                                              # entry k is area_metrics on the suffix sum
            one = area_metrics(*areas_of(selective_counts_of(counts, k)), metric=("mIoU", "mFscore"))
            assert all(np.array_equal(m[key][k], v, equal_nan=True) for key, v in one.items()), k
            assert all(np.array_equal(a[k], b) for a, b in zip(selective_areas_of(counts), areas_of(counts[k:].sum(0))))
        # coverage and aAcc against the calibration's curve.  aAcc_k = sum_{l < C} S_k[l, l] / sum_{l < C} sum_p S_k[l, p] (S_k = counts[k:].sum(0)):
        # `total_area_to_metrics` divides by sum(area_label), and area_label has the label rows l < C only -- row C (kept labels outside [0, C)) is in
        # neither the numerator nor the denominator, exactly as Calibration leaves those pixels out.  So the two agree with out-of-range labels as without.
        cov, acc = risk_coverage_of(CR.bins_of(pred[0], conf[0], label[0], C, K, **kw))
        assert np.array_equal(m["coverage"], cov) and np.array_equal(m["aAcc"], acc, equal_nan=True) and m["coverage"][0] == 1
        assert (np.diff(m["coverage"]) <= 0).all()
    # a threshold that keeps nothing: NaN, not an exception and not a warning
    import warnings
    e = counts.copy()
    e[K - 2:] = 0
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        m = selective_metrics_of(e)
    assert m["coverage"][K - 1] == 0 and np.isnan(m["aAcc"][K - 2:]).all() and np.isnan(m["mIoU"][K - 2:]).all() and not np.isnan(m["mIoU"][:K - 2]).any()
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        z = selective_metrics_of(np.zeros((3, 4, 4), dtype=np.int64))
    assert all(np.isnan(v).all() for v in z.values())
    assert np.array_equal(selective_metrics_of(e, nan_to_num=0)["mIoU"][K - 2:], [0, 0])
    # refusals and overflow
    assert not selective_counts_of(counts, K).any()
    for bad in (-1, K + 1, 1.5, True):
        with pytest.raises(ValueError, match="min_bin"):
            selective_counts_of(counts, bad)
    with pytest.raises(ValueError, match=r"\[K, C \+ 1, C \+ 1\]"):
        selective_counts_of(np.zeros((3, 4, 5), dtype=np.int64))
    with pytest.raises(ValueError, match=r"\[K, C \+ 1, C \+ 1\]"):
        selective_metrics_of(np.zeros((3, 4, 4)))
    big = np.zeros((3, 4, 4), dtype=np.int64)
    big[:, 1, 1] = 2 ** 62
    assert selective_counts_of(big, 2)[1, 1] == 2 ** 62 and selective_counts_of(big[:1], 0)[1, 1] == 2 ** 62
    with pytest.raises(OverflowError, match="int64"):
        selective_counts_of(big, 0)
    big[0, 1, 1] = -5
    with pytest.raises(OverflowError, match="wrapped"):
        selective_counts_of(big, 2)


def test_threshold_is_a_bin_edge_or_refused():
    from mmsa.evaluate import bin_edge, bin_of, threshold_bin
    for K in (1, 2, 10, 15, 16, 64):
        assert np.array_equal(bin_of(CR.SPECIALS, K), CR.bin_index(CR.SPECIALS, K))
        conf = CR.make_case(K, 9, 31, 5, K)[1]
        assert np.array_equal(bin_of(conf, K), CR.bin_index(conf, K))
        for j in range(K):
            e = bin_edge(j, K)
            assert e.dtype == np.float32 and CR.bin_index(e, K) == j and (j == 0 or CR.bin_index(np.nextafter(e, np.float32(0)), K) == j - 1)
            assert abs(float(e) - j / K) <= 2.0 ** -24
            assert threshold_bin(float(e), K) == j and threshold_bin(e, K) == j
    assert threshold_bin(0.5, 2) == 1 and threshold_bin(0.25, 16) == 4 and threshold_bin(0, 15) == 0 and threshold_bin(0.2, 5) == 1
    with pytest.raises(ValueError, match=r"not a bin edge of 15 bins.*0.2666666\d+ \(min_bin 4\) and 0.3333333\d+ \(min_bin 5\)"):
        threshold_bin(0.33, 15)
    with pytest.raises(ValueError, match=r"min_bin=15 \(abstain everywhere\)"):
        threshold_bin(1.0, 15)
    for bad in (-0.1, 1.5, "0.5", None, True, float("nan")):
        with pytest.raises(ValueError, match="threshold"):
            threshold_bin(bad, 15)


def test_selective_evaluator_without_a_device():
    from mmsa.evaluate import Evaluator, LabelPrep, SelectiveEvaluator, abstain, selective
    lp = LabelPrep(5)
    se = SelectiveEvaluator(lp, cases=["fog", "night"])
    assert se.n_bins == 15 and se.counts is None and se.host_counts().shape == (2, 15, 6, 6) and se.host_counts().dtype == np.int64
    assert SelectiveEvaluator(lp, bins=10).host_counts().shape == (0, 10, 6, 6)
    assert se.evaluator_counts().shape == (2, 6, 6) and se.reliability_counts().shape == (2, 2, 15) and se.reliability_counts(slot="night").shape == (2, 15)
    assert SelectiveEvaluator(lp).evaluator_counts().shape == (0, 6, 6) and [a.shape for a in SelectiveEvaluator(lp).areas()] == [(0, 5)] * 4
    # nothing added: NaN everywhere, the Evaluator's keys
    ev = Evaluator(lp, cases=["fog", "night"])
    assert list(se.metrics()) == list(ev.metrics()) and np.isnan(se.metrics(min_bin=3, slot="fog")["aAcc"])
    assert all(np.array_equal(a, b) for a, b in zip(se.areas(), ev.areas()))
    assert list(se.coverage_curve())[:2] == ["coverage", "aAcc"] and se.coverage_curve(slot=1)["mIoU"].shape == (15,)
    with pytest.raises(KeyError, match="SelectiveEvaluator"):
        se.slots_for(2, case="rain")
    assert se.slots_for(3, case="night") == [1, 1, 1] and se._slot_index("night") == 1
    per = SelectiveEvaluator(lp, images=3)
    assert per.slots_for(2) == [0, 1] == per.slots_for(2)                  # nothing is taken before a launch has gone through
    per._taken(2, None, None)
    assert per.used == 2 and per.slots_for(1) == [2]
    with pytest.raises(RuntimeError, match="SelectiveEvaluator: 2 \\+ 2 images but 3 per-image slots \\(read host_counts\\(\\)"):
        per.slots_for(2)
    assert per.used == 2                                                   # the refusal consumed no slot
    with pytest.raises(KeyError, match="a SelectiveEvaluator made with cases"):
        per.slots_for(1, case="fog")
    per.reset()
    assert per.used == 0
    for bad in (0, 65, 2.5, True, None):
        with pytest.raises(ValueError, match="1..64 confidence bins"):
            SelectiveEvaluator(lp, bins=bad)
    with pytest.raises(ValueError, match="at least one slot"):
        SelectiveEvaluator(lp, images=0)
    # the size refusal names the size; 64 slots of the largest case are allowed (528 MB), nothing is allocated without device=
    with pytest.raises(ValueError, match=r"131 slots x 64 bins x 127 x 127 int64 counts are 1081804288 bytes, above the 1073741824 \(1 GiB\)"):
        SelectiveEvaluator(LabelPrep(126), bins=64, images=131)
    assert SelectiveEvaluator(LabelPrep(126), bins=64, images=64).counts is None and SelectiveEvaluator(LabelPrep(126), bins=64, images=130).n_slots == 130
    with pytest.raises(RuntimeError, match="selective evaluation supports 2..126"):
        SelectiveEvaluator(LabelPrep(127))
    # there is no CPU path
    p, c = torch.zeros(1, 4, 4, dtype=torch.uint8), torch.zeros(1, 4, 4)
    with pytest.raises(RuntimeError, match="pred must be a GPU tensor"):
        selective(p, c, p, lp)
    with pytest.raises(RuntimeError, match="pred must be a GPU tensor"):
        abstain(p, c, 15, 3)
    with pytest.raises(RuntimeError, match="pred must be a GPU tensor"):
        per.add(p, c, p)
    assert per.used == 0 and per.counts is None


def test_the_entries_are_declared_bound_and_versioned():
    import mmsa
    hdr = open(os.path.join(ROOT, "include", "mmsa.h")).read()
    ver = int(re.search(r"#define MMSA_ABI_VERSION (\d+)", open(os.path.join(ROOT, "include", "mmsa_version.h")).read()).group(1))
    for name in ("mmsa_eval_selective", "mmsa_abstain_u8"):
        assert name in hdr and name in mmsa.lib.SIGNATURES and hasattr(mmsa.lib.raw, name)
    assert mmsa.lib.version() == mmsa.lib.ABI_VERSION == ver >= 113
    assert mmsa.SelectiveEvaluator is mmsa.evaluate.SelectiveEvaluator and mmsa.selective is mmsa.evaluate.selective and mmsa.abstain is mmsa.evaluate.abstain
    assert {"SelectiveEvaluator", "selective", "abstain"} <= set(mmsa.__all__)
    # the library refuses bad arguments on the host, before any launch (no GPU needed)
    one = (ctypes.c_int * 1)(0)
    fake = ctypes.c_void_p(256)
    call = mmsa.lib.raw.mmsa_eval_selective

    def refused(*a):
        return call(*a) != 0 and mmsa.lib.last_error()
    for C in (1, 127, 254):
        msg = refused(fake, fake, fake, 1, 4, 4, 4, 4, fake, C, None, None, one, 1, 15, fake, None)
        assert "2..126" in msg and "LDS" in msg and "histogram" in msg
    for bins in (0, 65):
        assert "1..64" in refused(fake, fake, fake, 1, 4, 4, 4, 4, fake, 25, None, None, one, 1, bins, fake, None)
    for B in (0, 65):
        assert "images per call" in refused(fake, fake, fake, B, 4, 4, 4, 4, fake, 25, None, None, one, 1, 15, fake, None)
    assert "size mismatch" in refused(fake, fake, fake, 1, 4, 4, 5, 4, fake, 25, None, None, one, 1, 15, fake, None)
    assert "come together" in refused(fake, fake, fake, 1, 4, 4, 5, 4, fake, 25, fake, None, one, 1, 15, fake, None)
    assert "come together" in refused(fake, fake, fake, 1, 4, 4, 5, 4, fake, 25, None, fake, one, 1, 15, fake, None)
    assert "4-byte aligned" in refused(fake, ctypes.c_void_p(258), fake, 1, 4, 4, 4, 4, fake, 25, None, None, one, 1, 15, fake, None)
    assert "are required" in refused(None, fake, fake, 1, 4, 4, 4, 4, fake, 25, None, None, one, 1, 15, fake, None)
    assert "are required" in refused(fake, None, fake, 1, 4, 4, 4, 4, fake, 25, None, None, one, 1, 15, fake, None)
    assert "are required" in refused(fake, fake, None, 1, 4, 4, 4, 4, fake, 25, None, None, one, 1, 15, fake, None)
    assert "are required" in refused(fake, fake, fake, 1, 4, 4, 4, 4, None, 25, None, None, one, 1, 15, fake, None)
    assert "are required" in refused(fake, fake, fake, 1, 4, 4, 4, 4, fake, 25, None, None, None, 1, 15, fake, None)
    assert "are required" in refused(fake, fake, fake, 1, 4, 4, 4, 4, fake, 25, None, None, one, 1, 15, None, None)
    one[0] = 3
    assert "outside the 2 count slots" in refused(fake, fake, fake, 1, 4, 4, 4, 4, fake, 25, None, None, one, 2, 15, fake, None)
    call = mmsa.lib.raw.mmsa_abstain_u8
    for a in ((None, fake, 16, 15, 3, fake, None), (fake, None, 16, 15, 3, fake, None), (fake, fake, 16, 15, 3, None, None)):
        assert "are required" in refused(*a)
    assert "4-byte aligned" in refused(fake, ctypes.c_void_p(258), 16, 15, 3, fake, None)
    for bins in (0, 65):
        assert "1..64" in refused(fake, fake, 16, bins, 0, fake, None)
    for mb in (-1, 16):
        assert "outside 0..15" in refused(fake, fake, 16, 15, mb, fake, None)
    for n in (0, -4, 1 << 40):
        assert "pixels" in refused(fake, fake, n, 15, 3, fake, None)


def test_inference_entries_refuse_a_selective_evaluator_without_its_inputs():
    """selective= needs labels= and the confidence map, by name, before anything is looked at (no GPU needed: the check comes first)."""
    import mmsa.inference as inf
    from mmsa.evaluate import Calibration, LabelPrep, SelectiveEvaluator
    se = SelectiveEvaluator(LabelPrep(5))
    lab = torch.zeros(1, 8, 8, dtype=torch.uint8)
    x = torch.zeros(1, 6, 8, 8)
    with pytest.raises(RuntimeError, match="whole_class_map: selective= needs labels="):
        inf.whole_class_map(None, None, x, confidence=True, selective=se)
    with pytest.raises(RuntimeError, match="slide_class_map: selective= needs the confidence map"):
        inf.slide_class_map(None, None, x, (4, 4), (4, 4), labels=lab, selective=se)
    with pytest.raises(RuntimeError, match="class_map: selective= needs labels="):
        inf.class_map(None, None, x, dict(mode="whole"), confidence=True, selective=se)
    with pytest.raises(RuntimeError, match="aug_class_map: selective= needs the confidence map"):
        inf.aug_class_map(None, None, [x], dict(mode="whole"), labels=lab, selective=se)
    for kw in (dict(fused=True), dict(return_map=False)):
        with pytest.raises(RuntimeError, match="whole_class_map: confidence with fused=True / return_map=False"):
            inf.whole_class_map(None, None, x, labels=lab, confidence=True, selective=se, **kw)
        with pytest.raises(RuntimeError, match="slide_class_map: confidence with fused=True / return_map=False"):
            inf.slide_class_map(None, None, x, (4, 4), (4, 4), labels=lab, confidence=True, selective=se, **kw)
    for wrong in (object(), Calibration(LabelPrep(5))):
        with pytest.raises(RuntimeError, match="selective= takes an mmsa.evaluate.SelectiveEvaluator"):
            inf.whole_class_map(None, None, x, labels=lab, confidence=True, selective=wrong)
    with pytest.raises(RuntimeError, match="calibration= takes an mmsa.evaluate.Calibration, got SelectiveEvaluator"):
        inf.whole_class_map(None, None, x, labels=lab, confidence=True, calibration=se)
    plan = inf.MapPlan.whole(1, 8, 8)
    with pytest.raises(RuntimeError, match="come together"):                 # labels= with none of the three is refused as before
        plan.class_map(None, None, None, labels=lab)
    with pytest.raises(RuntimeError, match="selective= needs the confidence map"):
        plan.class_map(None, None, None, labels=lab, selective=se)
    with pytest.raises(RuntimeError, match="inference: selective= needs labels="):
        plan.class_map(None, None, None, conf=x[0], selective=se)
    assert se.used == 0 and se.counts is None
