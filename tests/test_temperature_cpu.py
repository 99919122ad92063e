"""Host side of temperature scaling (no GPU): the ABI number and the four entries, the argument refusals of mmsa_temperature_sweep_nchw and of the `_t`
entries reached with fake pointers, `inv_temperature` and `geometric_grid`, the metrics of a sweep on hand-made integers, the Python refusals of
`temperature=`, TemperatureSweep's buffer shapes and slot routing, and the planted-temperature case in float64."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from tests import temperature_ref as TR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("mmsa_slide_argmax_conf_t", "mmsa_slide_argmax_resized_conf_t", "mmsa_softmax_flip_accum_nchw_t", "mmsa_temperature_sweep_nchw")


def test_the_entries_are_declared_bound_and_versioned():
    import mmsa
    hdr = open(os.path.join(ROOT, "include", "mmsa.h")).read()
    ver = int(re.search(r"#define MMSA_ABI_VERSION (\d+)", open(os.path.join(ROOT, "include", "mmsa_version.h")).read()).group(1))
    assert mmsa.lib.version() == mmsa.lib.ABI_VERSION == ver == 114
    for name in ENTRIES:
        assert name in hdr and name in mmsa.lib.SIGNATURES and hasattr(mmsa.lib.raw, name), name
    assert mmsa.TemperatureSweep is mmsa.evaluate.TemperatureSweep and mmsa.temperature_sweep is mmsa.evaluate.temperature_sweep
    assert "TemperatureSweep" in mmsa.__all__ and "temperature_sweep" in mmsa.__all__


def test_the_sweep_entry_refuses_bad_arguments_on_the_host():
    """Before any launch, so no GPU is needed: every pointer is a fake but `slots` and `inv_temperatures`, which the entry reads on the host."""
    import mmsa
    one = (ctypes.c_int * 1)(0)
    fake = ctypes.c_void_p(256)
    call = mmsa.lib.raw.mmsa_temperature_sweep_nchw

    def its(*v):
        return (ctypes.c_float * max(len(v), 1))(*v)

    def refused(B=1, C=25, H=4, W=4, Hl=4, Wl=4, ymap=None, xmap=None, slots=one, n_slots=1, it=its(1.0), J=1, bins=15, logits=fake):
        rc = call(logits, fake, B, C, H, W, Hl, Wl, fake, ymap, xmap, slots, n_slots, it, J, bins, fake, None)
        return rc != 0 and mmsa.lib.last_error()

    for J in (0, 17):
        assert "1..16" in refused(J=J, it=its(*([1.0] * 17)))
    for bad in (0.0, -1.0, float("nan"), float("inf"), -float("inf")):
        assert "inv_temperature" in refused(it=its(bad)), bad
        assert "inv_temperature" in refused(it=its(1.0, 0.5, bad), J=3), bad
    for bins in (0, 65):
        assert "1..64" in refused(bins=bins)
    for C in (1, 255):
        assert "2..254" in refused(C=C)
    assert "images per call" in refused(B=65)
    assert "come together" in refused(ymap=fake) and "come together" in refused(xmap=fake)
    assert "size mismatch" in refused(Hl=5)
    assert "4-byte aligned" in refused(logits=ctypes.c_void_p(258))
    assert "are required" in refused(logits=None) and "are required" in refused(it=None)
    three = (ctypes.c_int * 1)(3)
    assert "outside the 2 count slots" in refused(slots=three, n_slots=2)


def test_the_apply_entries_refuse_a_bad_inverse_temperature():
    import mmsa
    fake = ctypes.c_void_p(256)
    win = (ctypes.c_int * 3)(0, 0, 0)
    raw = mmsa.lib.raw
    for bad in (0.0, -2.0, float("nan"), float("inf")):
        assert raw.mmsa_slide_argmax_conf_t(fake, 1, 5, 4, 4, win, fake, fake, 1, 16, 16, 16, 16, fake, bad, None) != 0
        assert "slide_argmax_conf_t: inv_temperature" in mmsa.lib.last_error()
        assert raw.mmsa_slide_argmax_resized_conf_t(fake, 1, 5, 4, 4, win, fake, fake, 1, 16, 16, 16, 16, 20, 20, 20, 20, fake, bad, None) != 0
        assert "slide_argmax_resized_conf_t: inv_temperature" in mmsa.lib.last_error()
        assert raw.mmsa_softmax_flip_accum_nchw_t(fake, ctypes.c_void_p(512), 1, 5, 4, 4, 0, 0, 0, bad, None) != 0
        assert "softmax_flip_accum_nchw_t: inv_temperature" in mmsa.lib.last_error()
    # the checks of the siblings come first and are the siblings'
    assert raw.mmsa_slide_argmax_conf_t(fake, 1, 5, 4, 4, win, fake, None, 1, 16, 16, 16, 16, fake, 1.0, None) != 0 and "bad args" in mmsa.lib.last_error()
    assert raw.mmsa_softmax_flip_accum_nchw_t(fake, fake, 1, 5, 4, 4, 0, 0, 0, 1.0, None) != 0 and "bad args" in mmsa.lib.last_error()
    assert raw.mmsa_softmax_flip_accum_nchw_t(fake, ctypes.c_void_p(512), 1, 5, 4, 4, 3, 0, 0, 1.0, None) != 0 and "flip is 0" in mmsa.lib.last_error()


def test_inv_temperature_and_geometric_grid():
    from mmsa.evaluate import geometric_grid, inv_temperature
    for T in (0.25, 0.5, 1, 2.5, 3.0, 1e-30, 1e30, np.float32(7.0), np.float64(0.3)):
        it = inv_temperature(T)
        assert isinstance(it, float) and it == float(np.float32(1.0 / np.float64(T))) and np.float32(it) == it
    assert inv_temperature(1) == 1.0 and inv_temperature(0.25) == 4.0
    for bad in (0, -1.0, float("nan"), float("inf"), -float("inf"), 1e-40, 1e50, None, "2", True):
        with pytest.raises(ValueError, match="temperature"):
            inv_temperature(bad)
    g = geometric_grid(0.25, 8, 6)
    assert g.dtype == np.float64 and g.shape == (6,) and g[0] == 0.25 and g[-1] == 8 and np.allclose(g[1:] / g[:-1], 2.0)
    assert np.array_equal(geometric_grid(3, 3, 1), [3.0]) and np.array_equal(geometric_grid(2, 2, 3), [2.0, 2.0, 2.0])
    assert geometric_grid(1, 2, 16).shape == (16,) and (np.diff(geometric_grid(1, 2, 16)) > 0).all()
    for lo, hi, J in ((0, 1, 4), (2, 1, 4), (1, float("inf"), 4), (1, 2, 0), (1, 2, 17), (1, 2, 2.5), (-1, 2, 3)):
        with pytest.raises(ValueError):
            geometric_grid(lo, hi, J)


def test_sweep_metrics_on_hand_made_integers():
    from mmsa.evaluate import ece_of, mce_of, reliability_of, risk_coverage_of, sweep_best_of, sweep_bins_of, sweep_ece_of, sweep_nll_of
    one, nl = 2 ** 24, 2 ** 20
    #               bin:   0        1         2
    s = np.array([[[10, 0, 30], [2, 0, 27], [one, 0, 27 * one], [40 * nl, 0, 0]],                    # T0: mean NLL 1.0;  gaps |.2-.1|, |.9-.9| -> ECE 0.025
                  [[0, 20, 20], [0, 9, 20], [0, 9 * one, 15 * one], [0, 10 * nl, 10 * nl]],          # T1: mean NLL 0.5;  gaps |.45-.45|, |1-.75| -> ECE 0.125
                  [[10, 0, 30], [2, 0, 27], [one, 0, 27 * one], [20 * nl, 0, 0]],                    # T2: mean NLL 0.5 (a tie with T1);  T0's bins -> ECE 0.025 (a tie with T0)
                  [[40, 0, 0], [29, 0, 0], [4 * one, 0, 0], [80 * nl + 3, 0, 0]]], dtype=np.int64)   # T3: mean NLL 2 + 3 / (40 * 2^20)
    grid = (0.5, 1.0, 2.0, 4.0)
    nll = sweep_nll_of(s)
    assert nll.dtype == np.float64 and np.array_equal(nll[:3], [1.0, 0.5, 0.5]) and nll[3] == (80 * nl + 3) / (nl * 40.0)
    ece = sweep_ece_of(s)
    assert np.allclose(ece, [0.025, 0.125, 0.025, 0.625], rtol=0, atol=1e-15)
    assert sweep_best_of(s, grid, "nll") == (1.0, 1) and sweep_best_of(s, grid, "ece") == (0.5, 0)        # the FIRST minimum wins
    assert sweep_best_of(s, grid) == (1.0, 1)
    b = sweep_bins_of(s, 1)
    assert b.shape == (3, 3) and b.dtype == np.int64 and np.array_equal(b, s[1, :3]) and ece_of(b) == ece[1] and mce_of(b) == 0.25
    assert np.array_equal(reliability_of(b)["count"], [0, 20, 20]) and risk_coverage_of(b)[0][0] == 1.0
    with pytest.raises(ValueError, match="'nll' or 'ece'"):
        sweep_best_of(s, grid, "mce")
    with pytest.raises(ValueError, match="4 temperatures|3 temperatures"):
        sweep_best_of(s, grid[:3])
    with pytest.raises(ValueError, match="j = 4"):
        sweep_bins_of(s, 4)
    with pytest.raises(ValueError, match=r"\[J, 4, K\]"):
        sweep_nll_of(s[:, :3])
    empty = np.zeros((2, 4, 5), dtype=np.int64)
    assert np.isnan(sweep_nll_of(empty)).all() and np.isnan(sweep_ece_of(empty)).all()
    with pytest.raises(ValueError, match="no participating pixel"):
        sweep_best_of(empty, (1.0, 2.0))
    wrapped = s.copy()
    wrapped[0, 3, 0] = -5
    with pytest.raises(OverflowError, match="wrapped"):
        sweep_nll_of(wrapped)


def test_python_refusals_of_temperature():
    """temperature= without confidence= is refused with the reason; a T that is not finite and positive is a ValueError -- before anything is looked at."""
    import mmsa.inference as inf
    x = torch.zeros(1, 6, 8, 8)
    why = "temperature= without confidence=: the class map does not depend on the temperature"
    with pytest.raises(RuntimeError, match="whole_class_map: " + why):
        inf.whole_class_map(None, None, x, temperature=2.0)
    with pytest.raises(RuntimeError, match="slide_class_map: " + why):
        inf.slide_class_map(None, None, x, (4, 4), (4, 4), temperature=2.0, confidence=False)
    with pytest.raises(RuntimeError, match="class_map: " + why):
        inf.class_map(None, None, x, dict(mode="whole"), temperature=2.0)
    with pytest.raises(RuntimeError, match="SlideRunner: " + why):
        inf.SlideRunner(None, None, x, (4, 4), (4, 4), temperature=2.0)
    plan = inf.MapPlan.whole(1, 8, 8)
    with pytest.raises(RuntimeError, match="inference: " + why):
        plan.class_map(None, None, None, temperature=2.0)
    for bad in (0, -1.5, float("nan"), float("inf"), 1e-40, "3"):
        with pytest.raises(ValueError, match="temperature"):
            inf.whole_class_map(None, None, x, confidence=True, temperature=bad)
        with pytest.raises(ValueError, match="temperature"):
            inf.slide_class_map(None, None, x, (4, 4), (4, 4), confidence=True, temperature=bad)
        with pytest.raises(ValueError, match="temperature"):
            inf.class_map(None, None, x, dict(mode="whole"), confidence=True, temperature=bad)
        with pytest.raises(ValueError, match="temperature"):
            inf.probabilities(None, None, x, dict(mode="whole"), temperature=bad)
        with pytest.raises(ValueError, match="temperature"):
            inf.SlideRunner(None, None, x, (4, 4), (4, 4), confidence=True, temperature=bad)
        with pytest.raises(ValueError, match="temperature"):
            plan.class_map(None, None, None, conf=torch.zeros(1, 8, 8), temperature=bad)
    # the augmented entries have no such argument
    import inspect
    assert "temperature" not in inspect.signature(inf.aug_class_map).parameters and "temperature" not in inspect.signature(inf.aug_inference).parameters
    for fn in (inf.slide_class_map, inf.whole_class_map, inf.class_map, inf.probabilities, inf.MapPlan.class_map, inf.SlideRunner.__init__):
        assert inspect.signature(fn).parameters["temperature"].default is None, fn


def test_temperature_sweep_owner_on_the_host():
    from mmsa.evaluate import LabelPrep, TemperatureSweep, temperature_sweep
    lp = LabelPrep(5)
    grid = (0.5, 1.0, 2.0)
    sw = TemperatureSweep(lp, grid, cases=["fog", "night"])
    assert sw.n_bins == 15 and sw.counts is None and sw.host().shape == (2, 3, 4, 15) and sw.host().dtype == np.int64
    assert np.array_equal(sw.temperatures, grid) and sw.inv_temperatures == [2.0, 1.0, 0.5]
    assert TemperatureSweep(lp, grid, bins=10).host().shape == (0, 3, 4, 10) and TemperatureSweep(lp, 2.5).host().shape == (0, 1, 4, 15)
    assert np.isnan(sw.nll()).all() and np.isnan(sw.ece(slot="fog")).all() and sw.bins(2).shape == (3, 15)
    assert list(sw.summary()) == ["T", "NLL", "ECE", "aAcc", "best_nll", "best_ece"] and np.isnan(sw.summary()["best_nll"])
    with pytest.raises(ValueError, match="no participating pixel"):
        sw.best()
    with pytest.raises(KeyError, match="TemperatureSweep"):
        sw.slots_for(2, case="rain")
    assert sw.slots_for(3, case="night") == [1, 1, 1] and sw._slot_index("night") == 1
    per = TemperatureSweep(lp, grid, images=3)
    assert per.slots_for(2) == [0, 1]
    per._taken(2, None, None)
    assert per.used == 2 and per.slots_for(1) == [2]
    with pytest.raises(RuntimeError, match=r"TemperatureSweep: 2 \+ 2 images but 3 per-image slots \(read host\(\)"):
        per.slots_for(2)
    with pytest.raises(KeyError, match="a TemperatureSweep made with cases"):
        per.slots_for(1, case="fog")
    per.reset()
    assert per.used == 0
    for bad in ((), tuple([1.0] * 17)):
        with pytest.raises(ValueError, match="1..16 per sweep"):
            TemperatureSweep(lp, bad)
    with pytest.raises(ValueError, match="temperature = 0"):
        TemperatureSweep(lp, (1.0, 0))
    with pytest.raises(ValueError, match="1..64 confidence bins"):
        TemperatureSweep(lp, grid, bins=65)
    # there is no CPU path, and nothing is taken by a call that raised
    lg, lab = torch.zeros(1, 5, 4, 4), torch.zeros(1, 4, 4, dtype=torch.uint8)
    with pytest.raises(RuntimeError, match="logits must be a GPU tensor"):
        temperature_sweep(lg, lab, lp, grid)
    with pytest.raises(RuntimeError, match="logits must be a GPU tensor"):
        per.add(lg, lab)
    assert per.used == 0 and per.counts is None


def test_the_planted_temperature_is_the_minimum_in_float64():
    """The inputs of the GPU fit test, in float64 on the host: the figures the issue quotes, and margins far above the device bounds."""
    x, lab, grid = TR.planted_temperature_case()
    nll, ece = TR.planted_float64(x, lab, grid)
    assert np.allclose(nll, [2.119, 1.212, 0.927, 0.888, 0.925, 1.015], atol=5e-4) and np.allclose(ece, [0.271, 0.193, 0.088, 0.012, 0.092, 0.184], atol=5e-4)
    assert int(np.argmin(nll)) == int(np.argmin(ece)) == 3 and grid[3] == 2.5
    assert np.sort(nll)[1] - nll[3] > 0.03 and np.sort(ece)[1] - ece[3] > 0.07
