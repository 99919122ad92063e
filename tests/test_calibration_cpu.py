"""Host side of the calibration path of mmsa.evaluate (no GPU): the numpy restatement (tests/calibration_ref.py) against a brute-force loop in Python
integers and fractions, its invariants against the confusion counts of tests/eval_ref.py, the quantisation bound of the ECE, the metric functions on
hand-made bins, Calibration's slot bookkeeping and refusals, and the ABI number."""
import ctypes
import os
import re
from fractions import Fraction

import numpy as np
import pytest
import torch

from tests import calibration_ref as CR
from tests import eval_ref as ER

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VARIANTS = (dict(), dict(reduce_zero_label=True), dict(label_map={2: 1, 1: 0}), dict(ignore_index=0))


def _brute(pred, conf, label, C, K, **kw):
    """Pixel by pixel, in exact arithmetic but for the ONE float32 product the bin is defined by."""
    t, keep = ER.transform_bytes(**kw)
    out = [[0] * K for _ in range(3)]
    for p, c, raw in zip(pred.ravel().tolist(), conf.ravel(), label.ravel().tolist()):
        l = int(t[raw])
        if not keep[raw] or l >= C:
            continue
        c = np.float32(c)
        if np.isnan(c) or c < 0:
            c = np.float32(0)
        elif c > 1:
            c = np.float32(1)
        prod = np.float32(c) * np.float32(K)
        k = min(K - 1, int(prod))
        exact = Fraction(float(c))                               # a float32 is a rational number
        q = (exact * 2 ** 24).__floor__()
        out[0][k] += 1
        out[1][k] += int(p == l)
        out[2][k] += q
    return np.array(out, dtype=np.int64)


@pytest.mark.parametrize("kw", VARIANTS, ids=("plain", "rzl", "map", "ignore0"))
def test_restatement_equals_the_brute_force_loop(kw):
    for C, K in ((2, 1), (5, 15), (25, 16), (7, 64)):
        pred, conf, label = CR.make_case(50 + C, 9, 31, C, K, B=2)
        for b in range(2):
            got = CR.bins_of(pred[b], conf[b], label[b], C, K, **kw)
            assert got.dtype == np.int64 and np.array_equal(got, _brute(pred[b], conf[b], label[b], C, K, **kw)), (C, K, b)


def test_specials_land_where_the_definitions_put_them():
    n = len(CR.SPECIALS)
    pred = (np.arange(n) % 5).astype(np.uint8)
    for K in (1, 2, 15, 64):
        b = CR.bins_of(pred, CR.SPECIALS, pred, 5, K)
        want = np.zeros((3, K), dtype=np.int64)
        # NaN, -1, 0, 1e-40, -inf, -0.0 -> bin 0 with confidence 0; 2, 1, +inf -> the last bin with 2^24; the float below 1 -> the last bin with 2^24 - 1
        want[:2, 0] += 6
        want[:2, K - 1] += 4
        want[2, K - 1] += 4 * 2 ** 24 - 1
        assert np.array_equal(b, want), K
    # exact edges j / K fall where the float32 product puts them, and 1 in the last bin
    for K in (2, 10, 15, 16, 64):
        e = (np.arange(K + 1) / K).astype(np.float32)
        k = CR.bin_index(e, K)
        assert k[0] == 0 and k[-1] == K - 1 and np.array_equal(k, np.minimum(K - 1, (e * np.float32(K)).astype(np.int64)))
        assert (np.abs(k[:-1] - np.arange(K)) <= 1).all()


@pytest.mark.parametrize("C", (2, 25, 126))
def test_generator_fills_every_bin_and_the_invariants_hold(C):
    """sum(total) = sum over l < C of counts[l, :], sum(correct) = trace(counts[:C, :C]): the calibration's accuracy is the reference's aAcc."""
    from mmsa.evaluate import accuracy_of, area_metrics, areas_of
    for K in (1, 2, 10, 15, 16, 64):
        pred, conf, label = CR.make_case(3 + K, 37, 257, C, K)
        for kw in VARIANTS:
            b = CR.bins_of(pred[0], conf[0], label[0], C, K, **kw)
            counts = ER.confusion(pred[0], label[0], C, **kw)
            assert b[0].sum() == counts[:C, :].sum() and b[1].sum() == np.trace(counts[:C, :C])
            assert (b[1] <= b[0]).all() and (b[2] <= b[0] * 2 ** 24).all()
            assert accuracy_of(b) == area_metrics(*areas_of(counts))["aAcc"]
        b = CR.bins_of(pred[0], conf[0], label[0], C, K)
        assert (b[0] > 0).all(), (C, K)                          # every bin is in play
        part, _ = CR.participates(label[0], C)
        assert (label[0] == 255).any() and (~part & (label[0] != 255)).any() and (pred[0] == 255).any()


@pytest.mark.parametrize("C", (2, 25, 126))
def test_ece_from_the_bins_is_within_2_to_minus_24_of_float64(C):
    """Every per-bin mean confidence is truncated by less than 2^-24, |acc - conf| moves by less than that, and the weights sum to 1."""
    from mmsa.evaluate import ece_of, mce_of
    worst = 0.0
    for K in (1, 2, 10, 15, 16, 64):
        pred, conf, label = CR.make_case(90 + K, 37, 257, C, K)
        b = CR.bins_of(pred[0], conf[0], label[0], C, K)
        err = abs(float(ece_of(b)) - CR.ece_float64(pred[0], conf[0], label[0], C, K))
        worst = max(worst, err)
        assert err < 2.0 ** -24, (C, K, err)
        assert 0 <= ece_of(b) <= mce_of(b) <= 1
    print("C", C, "worst |ECE(bins) - ECE(float64)|:", worst)


def test_metric_functions_on_hand_made_bins():
    from mmsa.evaluate import (BIN_CAPACITY, accuracy_of, calibration_summary_of, ece_of, mce_of, mean_confidence_of, reliability_of, risk_coverage_of)
    one = 2 ** 24
    #            bin:   0      1      2      3
    b = np.array([[10,     0,    30,    60],
                  [2,      0,    15,    57],
                  [one,    0,    18 * one, 57 * one]], dtype=np.int64)        # mean confidences 0.1, -, 0.6, 0.95
    r = reliability_of(b)
    assert list(r) == ["edges", "count", "accuracy", "confidence"]
    assert np.array_equal(r["edges"], [0, 0.25, 0.5, 0.75, 1.0]) and np.array_equal(r["count"], [10, 0, 30, 60]) and r["count"].dtype == np.int64
    assert np.array_equal(r["accuracy"], [0.2, np.nan, 0.5, 0.95], equal_nan=True)
    assert np.array_equal(r["confidence"], [0.1, np.nan, 0.6, 0.95], equal_nan=True)
    gaps = np.array([abs(0.2 - 0.1), abs(0.5 - 0.6), abs(0.95 - 0.95)])
    assert ece_of(b) == np.sum(np.array([10, 30, 60]) / 100.0 * gaps) and mce_of(b) == gaps.max()
    assert accuracy_of(b) == 74 / 100 and mean_confidence_of(b) == 76 / 100
    cov, acc = risk_coverage_of(b)
    assert np.array_equal(cov, [1.0, 0.9, 0.9, 0.6]) and np.array_equal(acc, [0.74, 72 / 90, 72 / 90, 57 / 60])
    assert cov[0] == 1 and acc[0] == accuracy_of(b) and (np.diff(cov) <= 0).all()                      # entry 0 is (1, accuracy); coverage is monotone
    s = calibration_summary_of(b)
    assert list(s) == ["ECE", "MCE", "aAcc", "mConf"] and s["aAcc"] == 74.0 and s["mConf"] == 76.0 and s["MCE"] == 10.0
    assert s["ECE"] == np.round(ece_of(b) * 100, 2)
    # an empty top bin: nothing kept there
    e = b.copy()
    e[:, 3] = 0
    cov, acc = risk_coverage_of(e)
    assert cov[3] == 0 and np.isnan(acc[3]) and np.isnan(reliability_of(e)["accuracy"][3])
    # N == 0: every metric is NaN, nothing raises
    z = np.zeros((3, 5), dtype=np.int64)
    assert all(np.isnan(f(z)) for f in (ece_of, mce_of, accuracy_of, mean_confidence_of))
    assert np.isnan(reliability_of(z)["accuracy"]).all() and np.isnan(reliability_of(z)["confidence"]).all() and not reliability_of(z)["count"].any()
    assert all(np.isnan(a).all() for a in risk_coverage_of(z)) and all(np.isnan(v) for v in calibration_summary_of(z).values())
    # capacity: 2^39 pixels in a bin is where the int64 confidence sum may wrap
    full = np.array([[2 ** 39 - 1, 5], [2 ** 38, 5], [(2 ** 39 - 1) * one, 5 * one]], dtype=np.int64)
    assert mean_confidence_of(full) == 1.0 and 0 < accuracy_of(full) < 1
    full[0, 0] = BIN_CAPACITY
    for f in (reliability_of, ece_of, mce_of, accuracy_of, mean_confidence_of, risk_coverage_of, calibration_summary_of):
        with pytest.raises(OverflowError, match="2\\^39"):
            f(full)
    with pytest.raises(ValueError, match=r"\[3, K\]"):
        ece_of(np.zeros((2, 5), dtype=np.int64))
    with pytest.raises(ValueError, match=r"\[3, K\]"):
        ece_of(np.zeros((3, 5)))


def test_calibration_object_without_a_device():
    from mmsa.evaluate import Calibration, Evaluator, LabelPrep, calibration
    lp = LabelPrep(5)
    cal = Calibration(lp, cases=["fog", "night"])
    assert cal.n_bins == 15 and cal.bins is None and cal.host_bins().shape == (2, 3, 15) and cal.host_bins().dtype == np.int64
    assert Calibration(lp, bins=10).host_bins().shape == (0, 3, 10)
    assert np.isnan(cal.ece()) and np.isnan(cal.accuracy(slot="fog")) and np.isnan(cal.risk_coverage()[0]).all()      # nothing added: N == 0
    assert list(cal.summary()) == ["ECE", "MCE", "aAcc", "mConf"]
    with pytest.raises(KeyError, match="Calibration"):
        cal.slots_for(2, case="rain")
    assert cal.slots_for(3, case="night") == [1, 1, 1] and cal._slot_index("night") == 1 and cal._slot_index(0) == 0
    per = Calibration(lp, images=3)
    assert per.slots_for(2) == [0, 1] == per.slots_for(2)                  # nothing is taken before a launch has gone through
    per._taken(2, None, None)
    assert per.used == 2 and per.slots_for(1) == [2]
    with pytest.raises(RuntimeError, match="Calibration: 2 \\+ 2 images but 3 per-image slots"):
        per.slots_for(2)
    per._taken(1, None, [0])                                               # slots named outright (or a case) take no per-image slot
    assert per.used == 2 and per.slots_for(2, slots=[5, 6]) == [5, 6]
    with pytest.raises(KeyError, match="a Calibration made with cases"):
        per.slots_for(1, case="fog")
    per.reset()
    assert per.used == 0
    # the Evaluator shares the bookkeeping and keeps its own words
    with pytest.raises(KeyError, match="an Evaluator made with cases"):
        Evaluator(lp).slots_for(1, case="fog")
    with pytest.raises(RuntimeError, match="Evaluator: 0 \\+ 2 images but 1 per-image slots \\(read areas\\(\\)"):
        Evaluator(lp, images=1).slots_for(2)
    for bad in (0, 65, 2.5, True, None):
        with pytest.raises(ValueError, match="1..64 confidence bins"):
            Calibration(lp, bins=bad)
    with pytest.raises(ValueError, match="at least one slot"):
        Calibration(lp, images=0)
    # there is no CPU path
    p, c = torch.zeros(1, 4, 4, dtype=torch.uint8), torch.zeros(1, 4, 4)
    with pytest.raises(RuntimeError, match="pred must be a GPU tensor"):
        calibration(p, c, p, lp)
    with pytest.raises(RuntimeError, match="pred must be a GPU tensor"):
        per.add(p, c, p)
    assert per.used == 0 and per.bins is None


def test_the_entry_is_declared_bound_and_versioned():
    import mmsa
    hdr = open(os.path.join(ROOT, "include", "mmsa.h")).read()
    ver = int(re.search(r"#define MMSA_ABI_VERSION (\d+)", open(os.path.join(ROOT, "include", "mmsa_version.h")).read()).group(1))
    assert "mmsa_eval_calibration" in hdr and "mmsa_eval_calibration" in mmsa.lib.SIGNATURES and hasattr(mmsa.lib.raw, "mmsa_eval_calibration")
    assert mmsa.lib.version() == mmsa.lib.ABI_VERSION == ver >= 112
    assert mmsa.Calibration is mmsa.evaluate.Calibration and mmsa.calibration is mmsa.evaluate.calibration and "Calibration" in mmsa.__all__
    # the library refuses bad arguments on the host, before any launch (no GPU needed)
    one = (ctypes.c_int * 1)(0)
    fake = ctypes.c_void_p(256)
    call = mmsa.lib.raw.mmsa_eval_calibration

    def refused(*a):
        return call(*a) != 0 and mmsa.lib.last_error()
    assert "2..254" in refused(fake, fake, fake, 1, 4, 4, 4, 4, fake, 255, None, None, one, 1, 15, fake, None)
    assert "2..254" in refused(fake, fake, fake, 1, 4, 4, 4, 4, fake, 1, None, None, one, 1, 15, fake, None)
    for bins in (0, 65):
        assert "1..64" in refused(fake, fake, fake, 1, 4, 4, 4, 4, fake, 25, None, None, one, 1, bins, fake, None)
    assert "images per call" in refused(fake, fake, fake, 65, 4, 4, 4, 4, fake, 25, None, None, one, 1, 15, fake, None)
    assert "size mismatch" in refused(fake, fake, fake, 1, 4, 4, 5, 4, fake, 25, None, None, one, 1, 15, fake, None)
    assert "come together" in refused(fake, fake, fake, 1, 4, 4, 5, 4, fake, 25, fake, None, one, 1, 15, fake, None)
    assert "4-byte aligned" in refused(fake, ctypes.c_void_p(258), fake, 1, 4, 4, 4, 4, fake, 25, None, None, one, 1, 15, fake, None)
    assert "are required" in refused(fake, None, fake, 1, 4, 4, 4, 4, fake, 25, None, None, one, 1, 15, fake, None)
    one[0] = 3
    assert "outside the 2 count slots" in refused(fake, fake, fake, 1, 4, 4, 4, 4, fake, 25, None, None, one, 2, 15, fake, None)


def test_inference_entries_refuse_a_calibration_without_its_inputs():
    """calibration= needs labels= and the confidence map, by name, before anything is looked at (no GPU needed: the check comes first)."""
    import mmsa.inference as inf
    from mmsa.evaluate import Calibration, LabelPrep
    cal = Calibration(LabelPrep(5))
    lab = torch.zeros(1, 8, 8, dtype=torch.uint8)
    x = torch.zeros(1, 6, 8, 8)
    with pytest.raises(RuntimeError, match="whole_class_map: calibration= needs labels="):
        inf.whole_class_map(None, None, x, confidence=True, calibration=cal)
    with pytest.raises(RuntimeError, match="slide_class_map: calibration= needs the confidence map"):
        inf.slide_class_map(None, None, x, (4, 4), (4, 4), labels=lab, calibration=cal)
    with pytest.raises(RuntimeError, match="class_map: calibration= needs labels="):
        inf.class_map(None, None, x, dict(mode="whole"), confidence=True, calibration=cal)
    with pytest.raises(RuntimeError, match="aug_class_map: calibration= needs the confidence map"):
        inf.aug_class_map(None, None, [x], dict(mode="whole"), labels=lab, calibration=cal)
    for kw in (dict(fused=True), dict(return_map=False)):
        with pytest.raises(RuntimeError, match="whole_class_map: confidence with fused=True / return_map=False"):
            inf.whole_class_map(None, None, x, labels=lab, confidence=True, calibration=cal, **kw)
    with pytest.raises(RuntimeError, match="takes an mmsa.evaluate.Calibration"):
        inf.whole_class_map(None, None, x, labels=lab, confidence=True, calibration=object())
    # labels= with neither an evaluator nor a calibration is refused as before, on the launch helper
    plan = inf.MapPlan.whole(1, 8, 8)
    with pytest.raises(RuntimeError, match="come together"):
        plan.class_map(None, None, None, labels=lab)
    with pytest.raises(RuntimeError, match="calibration= needs the confidence map"):
        plan.class_map(None, None, None, labels=lab, calibration=cal)
    assert cal.used == 0 and cal.bins is None
