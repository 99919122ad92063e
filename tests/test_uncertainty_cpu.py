"""Host side of the uncertainty maps (no GPU): the float32 restatement of the two scores (tests/uncertainty_ref.py) against their float64 values within
the derived bounds, the exact cases, the area under the selective curves on hand-made counts, every new refusal (raised before any launch), and the ABI."""
import ctypes
import inspect
import os
import re
from fractions import Fraction

import numpy as np
import pytest
import torch

from tests import confidence_ref as CR
from tests import uncertainty_ref as UR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("mmsa_argmax_score_nchw", "mmsa_slide_argmax_score", "mmsa_slide_argmax_resized_score")
KINDS = sorted(UR.KINDS)


# ---- 1. the restatement against float64

def _cases(C):
    """name -> float32 logits [2, C, 16, 16]: the planted head logits, equal logits, one class ahead by 300, a two-way tie at the top."""
    x = CR.planted_logits(2, C, 500 + C)
    equal = x[:, :1].expand(-1, C, -1, -1).contiguous()
    ahead = x.clone()
    ahead[:, C // 2] += 300.0
    tie = x.clone()
    tie[:, 0] = x.max(1).values + 2.0
    tie[:, C - 1] = tie[:, 0]
    return dict(planted=x, equal=equal, ahead=ahead, tie=tie)


@pytest.mark.parametrize("C", [2, 5, 33, 65])
@pytest.mark.parametrize("kind", KINDS)
def test_restatement_is_within_the_bounds_of_float64(kind, C):
    for name, x in _cases(C).items():
        got = UR.restated(x, kind)
        worst, D = UR.float64_check(got, x, kind)
        print(f"{kind} C={C} {name}: D up to {D:.1f}, worst error / bound {worst:.3f}; score in [{got.min().item():.3e}, {got.max().item():.3e}]")
        if name == "planted":
            assert 30 <= D < 87, "the bounds assume no denormal exponential; the planted pixel reaches a spread of 30"
        assert worst <= 1.0, f"{kind} C={C} {name}"
        assert bool((got >= 0).all()) and bool((got <= 1).all())
    for T in (0.5, 2.3):
        from mmsa.evaluate import inv_temperature
        it = inv_temperature(T)
        x = _cases(C)["planted"]
        worst, DT = UR.float64_check(UR.restated(x, kind, it), x, kind, it)
        print(f"{kind} C={C} T={T}: D_T up to {DT:.1f}, worst error / tempered bound {worst:.3f}")
        assert worst <= 1.0      # D_T passes 87 at T = 0.5 and 65 classes: an exponential that goes denormal there moves a score by less than 1e-35
    x = _cases(C)["planted"]
    assert torch.equal(UR.restated(x, kind, 1.0), UR.restated(x, kind)), "the product with 1.0f is exact"


@pytest.mark.parametrize("C", [1, 2, 5, 33, 65])
def test_exact_values(C):
    x = CR.planted_logits(2, C, 600 + C)
    one = torch.ones(2, 16, 16)
    if C == 1:
        for kind in KINDS:
            assert torch.equal(UR.restated(x, kind), one), f"{kind}: one class is certain"
            assert UR.float64_check(UR.restated(x, kind), x, kind)[0] == 0.0
        return
    c = _cases(C)
    for kind in KINDS:
        assert torch.equal(UR.restated(c["ahead"], kind), one), f"{kind}: every other exponential is 0.0f, -(1 * log 1) is -0"
    assert bool((UR.restated(c["tie"], "margin") == 0).all()), "two equal maxima: p[bi] - p2 is x - x"
    assert bool((UR.restated(c["equal"], "margin") == 0).all())
    ent = UR.restated(c["equal"], "entropy")
    ref = UR.float64_scores(c["equal"])
    assert bool((ent >= 0).all()) and bool((ent.double() <= UR.bound(ref, "entropy")).all()), "H = log C up to rounding: the score is 0 within its bound, never below"
    assert float(ref["entropy"].abs().max()) < 1e-15


def test_the_bounds_are_the_derived_ones():
    """DESIGN.md section 2, spelled out on one pixel: D = 30, C = 5, P = (0.6, 0.3, ...), H = 1."""
    ref = dict(C=5, D=torch.tensor([30.0], dtype=torch.float64), p12=torch.tensor([0.9], dtype=torch.float64), H=torch.tensor([1.0], dtype=torch.float64))
    eps, eps_t = (2 * 30 + 5 + 4) * 2.0 ** -23, (4 * 30 + 5 + 4) * 2.0 ** -23
    assert UR.bound(ref, "margin").item() == eps * 0.9 + 2.0 ** -24 and UR.bound(ref, "margin", tempered=True).item() == eps_t * 0.9 + 2.0 ** -24
    assert UR.bound(ref, "entropy").item() == (eps * 2.0 + 7 * 2.0 ** -24) / np.log(5.0) + 3 * 2.0 ** -24
    assert UR.bound(dict(ref, C=1), "entropy").item() == 0.0


def test_inv_log_classes():
    from mmsa.evaluate import SCORES, inv_log_classes
    assert SCORES == {"max": 0, "margin": 1, "entropy": 2} and UR.KINDS == {k: v for k, v in SCORES.items() if v}
    assert inv_log_classes(1) == 0.0
    for C in (2, 5, 25, 33, 65, 255):
        v = inv_log_classes(C)
        assert isinstance(v, float) and v == float(np.float32(1.0 / np.log(np.float64(C)))) == UR.inv_log_c(C).item() and np.float32(v) == v
    for bad in (0, -3, 2.0, None, True, "5"):
        with pytest.raises(ValueError, match="classes"):
            inv_log_classes(bad)


# ---- 2. the area under the selective curves

def _counts(*bins):
    """[K, 3, 3] counts of two classes from [[l0p0, l0p1], [l1p0, l1p1]] per bin (None: an empty bin)."""
    c = np.zeros((len(bins), 3, 3), dtype=np.int64)
    for k, b in enumerate(bins):
        if b is not None:
            c[k, :2, :2] = b
    return c


def test_auc_on_hand_made_counts():
    from mmsa.evaluate import selective_auc_of
    # bins 0 .. 2 hold 4 / 4 / 2 pixels with 2 / 3 / 2 correct, the top bin is empty: coverage 1, 6/10, 2/10 (and 0: dropped); risk 3/10, 1/6, 0
    c = _counts([[1, 1], [1, 1]], [[2, 0], [1, 1]], [[1, 0], [0, 1]], None)
    risk = Fraction(4, 10) * (Fraction(3, 10) + Fraction(1, 6)) / 2 + Fraction(4, 10) * (Fraction(1, 6) + 0) / 2 + Fraction(2, 10) * 0
    assert risk == Fraction(19, 150)
    miou = Fraction(4, 10) * (Fraction(15, 28) + Fraction(17, 24)) / 2 + Fraction(4, 10) * (Fraction(17, 24) + 1) / 2 + Fraction(2, 10) * 1
    assert miou == Fraction(83, 105)
    assert selective_auc_of(c) == pytest.approx(float(risk), abs=1e-15) and selective_auc_of(c, "risk") == selective_auc_of(c)
    assert selective_auc_of(c, "aAcc") == pytest.approx(float(1 - risk), abs=1e-15)
    assert selective_auc_of(c, "mIoU") == pytest.approx(float(miou), abs=1e-15)
    assert isinstance(selective_auc_of(c), np.float64)
    # an empty bin in the middle repeats a point (zero width): the same areas
    c2 = _counts([[1, 1], [1, 1]], None, [[2, 0], [1, 1]], [[1, 0], [0, 1]], None)
    for m in ("risk", "mIoU", "aAcc"):
        assert selective_auc_of(c2, m) == pytest.approx(selective_auc_of(c, m), abs=1e-15)
    # every pixel in one bin: the curve is that point, extended flat over all coverages
    one = _counts(None, None, [[3, 1], [0, 4]], None)
    assert selective_auc_of(one) == 1 / 8 and selective_auc_of(one, "aAcc") == 7 / 8
    assert selective_auc_of(one, "mIoU") == pytest.approx(31 / 40, abs=1e-15)
    # a score that puts the errors in the low bins has the smaller AURC on the same pixels
    good, bad = _counts([[0, 2], [2, 0]], [[3, 0], [0, 3]]), _counts([[3, 0], [0, 3]], [[0, 2], [2, 0]])
    assert selective_auc_of(good) == pytest.approx(0.4 * (0.4 + 0) / 2, abs=1e-15) and selective_auc_of(bad) == pytest.approx(0.6 * (0.4 + 1) / 2 + 0.4 * 1, abs=1e-15)
    # nothing took part (no pixel, or only labels outside the classes): NaN
    assert np.isnan(selective_auc_of(_counts(None, None)))
    outside = np.zeros((3, 3, 3), dtype=np.int64)
    outside[1, 2, 0] = 7
    for m in ("risk", "mIoU", "aAcc"):
        assert np.isnan(selective_auc_of(outside, m))
    with pytest.raises(ValueError, match="one of"):
        selective_auc_of(c, "ECE")
    with pytest.raises(ValueError, match=r"\[K, C \+ 1, C \+ 1\]"):
        selective_auc_of(c[0])


def _direct(curve, key):
    cov = curve["coverage"]
    val = 1.0 - curve["aAcc"] if key == "risk" else curve[key]
    pts = sorted(((cov[k], -k, val[k]) for k in range(len(cov)) if cov[k] > 0), reverse=True)
    area = 0.0
    for (c0, _, v0), (c1, _, v1) in zip(pts, pts[1:]):
        area += (c0 - c1) * (v0 + v1) / 2
    return area + pts[-1][0] * pts[-1][2]


def test_auc_is_the_trapezoid_over_the_coverage_curve():
    from mmsa.evaluate import LabelPrep, SelectiveEvaluator, selective_auc_of, selective_metrics_of
    rng = np.random.default_rng(3)
    for C, K in ((2, 4), (5, 15), (25, 15)):
        c = rng.integers(0, 50, size=(K, C + 1, C + 1)).astype(np.int64)
        c[K - 1] = 0
        c[K // 2] = 0
        curve = selective_metrics_of(c, metric=("mIoU",))
        for m in ("risk", "mIoU", "aAcc"):
            assert selective_auc_of(c, m) == pytest.approx(_direct(curve, m), abs=1e-14), (C, K, m)
        assert selective_auc_of(c, "risk") + selective_auc_of(c, "aAcc") == pytest.approx(1.0, abs=1e-14)
    se = SelectiveEvaluator(LabelPrep(5), bins=15, cases=["fog", "night"])
    host = rng.integers(0, 50, size=(2, 15, 6, 6)).astype(np.int64)
    se.host_counts = lambda: host
    for m in ("risk", "mIoU", "aAcc"):
        assert se.auc(m) == selective_auc_of(host.sum(0), m) == pytest.approx(_direct(se.coverage_curve(), m), abs=1e-14)
        assert se.auc(m, slot="night") == selective_auc_of(host[1], m)
    assert se.auc() == se.auc("risk")
    plain, with_auc = se.summary(), se.summary(auc=True)
    assert "AURC" not in plain and list(with_auc) == list(plain) + ["AURC"] and with_auc["AURC"] == np.round(se.auc() * 100, 2) / 100.0
    assert se.summary(slot="fog", auc=True)["AURC"] == np.round(se.auc(slot="fog") * 100, 2) / 100.0
    assert "trapezoid" in selective_auc_of.__doc__ and "FLAT" in selective_auc_of.__doc__


# ---- 3. refusals, all before any launch

def test_python_refusals_of_score():
    import mmsa
    import mmsa.inference as inf
    x = torch.zeros(1, 6, 8, 8)
    plan = inf.MapPlan.whole(1, 8, 8)
    for bad in ("top2", "", None, 1, ["margin"]):
        why = "score= must be one of"
        with pytest.raises(RuntimeError, match="whole_class_map: " + why):
            inf.whole_class_map(None, None, x, confidence=True, score=bad)
        with pytest.raises(RuntimeError, match="slide_class_map: " + why):
            inf.slide_class_map(None, None, x, (4, 4), (4, 4), confidence=True, score=bad)
        with pytest.raises(RuntimeError, match="class_map: " + why):
            inf.class_map(None, None, x, dict(mode="whole"), confidence=True, score=bad)
        with pytest.raises(RuntimeError, match="aug_class_map: " + why):
            inf.aug_class_map(None, None, [x], dict(mode="whole"), confidence=True, score=bad)
        with pytest.raises(RuntimeError, match="SlideRunner: " + why):
            inf.SlideRunner(None, None, x, (4, 4), (4, 4), confidence=True, score=bad)
        with pytest.raises(RuntimeError, match="inference: " + why):
            plan.class_map(None, None, None, conf=torch.zeros(1, 8, 8), score=bad)
        with pytest.raises(RuntimeError, match="argmax_score_map: " + why):
            mmsa.argmax_score_map(torch.zeros(1, 5, 4, 4), score=bad)
    for score in ("margin", "entropy"):
        why = f"score='{score}' without confidence=: the score is written in the confidence map's place"
        with pytest.raises(RuntimeError, match="whole_class_map: " + why):
            inf.whole_class_map(None, None, x, score=score)
        with pytest.raises(RuntimeError, match="slide_class_map: " + why):
            inf.slide_class_map(None, None, x, (4, 4), (4, 4), score=score, confidence=False)
        with pytest.raises(RuntimeError, match="class_map: " + why):
            inf.class_map(None, None, x, dict(mode="whole"), score=score)
        with pytest.raises(RuntimeError, match="aug_class_map: " + why):
            inf.aug_class_map(None, None, [x], dict(mode="whole"), score=score)
        with pytest.raises(RuntimeError, match="SlideRunner: " + why):
            inf.SlideRunner(None, None, x, (4, 4), (4, 4), score=score)
        with pytest.raises(RuntimeError, match="inference: " + why):
            plan.class_map(None, None, None, score=score)
        # fused=True / return_map=False: as for the confidence (the entries' own refusals need a frame on the device: tests/test_uncertainty_gpu.py)
        for kw in (dict(fused=True), dict(return_map=False)):
            with pytest.raises(RuntimeError, match="inference: confidence with fused=True / return_map=False"):
                plan.class_map(None, torch.zeros(1, 8, 8, dtype=torch.uint8), None, conf=torch.zeros(1, 8, 8), score=score, **kw)
        # augmented views: the canvas path only
        why = f"score='{score}' with one_pass=True: the one-pass augmented launch"
        with pytest.raises(RuntimeError, match="aug_class_map: " + why):
            inf.aug_class_map(None, None, [x, x], dict(mode="whole"), confidence=True, score=score, one_pass=True)
        aug = inf.AugPlan.make(dict(mode="whole"), [(1, 8, 8)] * 2)
        with pytest.raises(RuntimeError, match="inference: " + why):
            aug.class_map([None, None], None, None, one_pass=True, conf=torch.zeros(1, 8, 8), score=score)
        # a bad temperature next to a score is still the temperature's refusal
        with pytest.raises(ValueError, match="temperature"):
            inf.whole_class_map(None, None, x, confidence=True, score=score, temperature=0)
    # "max" is the default everywhere and the augmented entries still take no temperature
    for fn in (inf.slide_class_map, inf.whole_class_map, inf.class_map, inf.aug_class_map, inf.MapPlan.class_map, inf.AugPlan.class_map, inf.SlideRunner.__init__):
        assert inspect.signature(fn).parameters["score"].default == "max", fn
    assert "temperature" not in inspect.signature(inf.aug_class_map).parameters
    assert mmsa.argmax_score_map is inf.argmax_score_map and "argmax_score_map" in mmsa.__all__
    with pytest.raises(RuntimeError):                      # there is no CPU path
        mmsa.argmax_score_map(torch.zeros(1, 5, 4, 4), score="margin")


def test_the_entries_refuse_bad_arguments_on_the_host():
    """Before any launch, so no GPU is needed: every pointer is a fake but the window table, which the entries read on the host."""
    import mmsa
    fake = ctypes.c_void_p(256)
    win = (ctypes.c_int * 3)(0, 0, 0)
    raw = mmsa.lib.raw

    def canvas(kind=1, ilc=0.5, score=fake, C=5):
        rc = raw.mmsa_argmax_score_nchw(fake, fake, score, 1, C, 4, 4, kind, ilc, None)
        return rc != 0 and mmsa.lib.last_error()

    def frame(kind=1, it=1.0, ilc=0.5, score=fake):
        rc = raw.mmsa_slide_argmax_score(fake, 1, 5, 4, 4, win, fake, score, 1, 16, 16, 16, 16, fake, kind, it, ilc, None)
        return rc != 0 and mmsa.lib.last_error()

    def resized(kind=1, it=1.0, ilc=0.5, score=fake, Hcut=20):
        rc = raw.mmsa_slide_argmax_resized_score(fake, 1, 5, 4, 4, win, fake, score, 1, 16, 16, 16, 16, 20, 20, Hcut, 20, fake, kind, it, ilc, None)
        return rc != 0 and mmsa.lib.last_error()

    for kind in (0, 3, -1):
        assert "argmax_score_nchw: kind" in canvas(kind=kind) and "slide_argmax_score: kind" in frame(kind=kind)
        assert "slide_argmax_resized_score: kind" in resized(kind=kind)
    for bad in (-0.5, float("nan"), float("inf")):
        assert "argmax_score_nchw: inv_log_c" in canvas(ilc=bad) and "slide_argmax_score: inv_log_c" in frame(ilc=bad)
        assert "slide_argmax_resized_score: inv_log_c" in resized(ilc=bad)
    for bad in (0.0, -2.0, float("nan"), float("inf")):
        assert "slide_argmax_score: inv_temperature" in frame(it=bad) and "slide_argmax_resized_score: inv_temperature" in resized(it=bad)
    assert "bad args" in canvas(score=None) and "bad args" in frame(score=None) and "bad args" in resized(score=None)
    assert "bad args" in canvas(C=257)
    assert "must lie inside the target" in resized(Hcut=21)


def test_the_entries_are_declared_bound_and_versioned():
    import mmsa
    hdr = open(os.path.join(ROOT, "include", "mmsa.h")).read()
    header = int(re.search(r"#define MMSA_ABI_VERSION (\d+)", open(os.path.join(ROOT, "include", "mmsa_version.h")).read()).group(1))
    assert mmsa.lib.version() == mmsa.lib.ABI_VERSION == header and header >= 114
    for name in ENTRIES:
        assert name in hdr and name in mmsa.lib.SIGNATURES and hasattr(mmsa.lib.raw, name), name
