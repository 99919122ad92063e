"""Top-k maps without a GPU: the restatement of the rank list (tests/topk_ref.py) against the definition by a stable sort, the exact cases, the condition
the float64 order test of tests/test_topk_gpu.py rests on, TopKEvaluator's metrics on hand-made counts, every refusal of `topk=` before anything is launched,
the entries' argument checks on the host, and header / ctypes table / version."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import confidence_ref as CR
from tests import topk_ref as TR
from tests import uncertainty_ref as UR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("mmsa_slide_argmax_topk", "mmsa_argmax_topk_nchw", "mmsa_eval_topk_u8")
CK = [(1, 1), (1, 2), (2, 1), (2, 2), (2, 3), (5, 2), (5, 3), (5, 4), (5, 5), (5, 8), (33, 4), (33, 5), (33, 8), (65, 8)]      # (C, K), K > C included


# ---- 1. the restatement is the definition

@pytest.mark.parametrize("C,K", CK)
def test_the_rank_list_is_a_stable_sort_with_the_map_class_first(C, K):
    g = torch.Generator().manual_seed(10 * C + K)
    x = torch.randn(2, C, 9, 11, generator=g) * 6.0
    p = UR.probabilities(x)
    bi = UR.first_argmax(x)
    got = TR.topk(p, bi, K)
    want = TR.by_sort(p, bi, K)
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
    # planted ties: few distinct values per pixel, and a map class that is NOT the first maximum of the probabilities (a later class of the same value)
    q = (torch.randint(0, 3, (2, C, 9, 11), generator=g).float() + 1.0) / 8.0
    last = (C - 1) - q.flip(1).argmax(1)                                                  # the LAST class that holds the largest value
    for b in (UR.first_argmax(q), last, torch.randint(0, C, (2, 9, 11), generator=g)):
        got, want = TR.topk(q, b, K), TR.by_sort(q, b, K)
        assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
        assert torch.equal(got[0][0].long(), b) and torch.equal(got[1][0], q.gather(1, b.unsqueeze(1)).squeeze(1))
    # every slot count that holds K gives the same first K ranks
    base = TR.topk(p, bi, K)
    for S in (2, 4, 8):
        if S >= K:
            alt = TR.topk(p, bi, K, slots=S)
            assert torch.equal(alt[0], base[0]) and torch.equal(alt[1], base[1])
    # a pixel without a class
    none = bi.clone()
    none[0, 0, :] = 255
    cls, pr = TR.topk(p, none, K)
    assert bool((cls[:, 0, 0, :] == 255).all()) and bool((pr[:, 0, 0, :] == 0).all()) and torch.equal(cls[:, 1], TR.topk(p, bi, K)[0][:, 1])


@pytest.mark.parametrize("C,K", [(2, 2), (2, 3), (5, 3), (5, 8), (33, 8)])
def test_exact_cases_on_the_restatement(C, K):
    n = min(K, C)
    x = torch.randn(1, C, 6, 7, generator=torch.Generator().manual_seed(C)) * 6.0
    # every class the same plane: classes 0, 1, ... and all probabilities equal
    cls, pr = TR.restated(x[:, :1].expand(-1, C, -1, -1).contiguous(), K)
    for r in range(K):
        assert bool((cls[r] == (r if r < C else 255)).all())
    assert all(torch.equal(pr[r], pr[0]) for r in range(n)) and bool((pr[n:] == 0).all())
    # one class ahead by 300: probs[0] == 1, the rest exactly 0, the runners-up the lowest other indices in class order
    ahead = x.clone()
    ahead[:, C // 2] += 300.0
    cls, pr = TR.restated(ahead, K)
    others = [c for c in range(C) if c != C // 2]
    assert bool((cls[0] == C // 2).all()) and bool((pr[0] == 1).all()) and bool((pr[1:] == 0).all())
    for r in range(1, K):
        assert bool((cls[r] == (others[r - 1] if r < C else 255)).all())
    # classes 0 and C - 1 tied at the top
    tie = x.clone()
    tie[:, 0] = x.max(1).values + 2.0
    tie[:, C - 1] = tie[:, 0]
    cls, pr = TR.restated(tie, K)
    assert bool((cls[0] == 0).all()) and bool((cls[1] == C - 1).all()) and torch.equal(pr[0], pr[1])
    # the three identities on the restatement: the map, the confidence, the margin
    cls, pr = TR.restated(x, K)
    p = UR.probabilities(x)
    assert torch.equal(cls[0].long(), UR.first_argmax(x)) and torch.equal(pr[0], p.max(1).values)
    assert torch.equal(pr[0] - pr[1], UR.score(p, UR.first_argmax(x), "margin"))


@pytest.mark.parametrize("C,K", [(2, 2), (5, 3), (5, 8), (33, 8), (64, 8), (65, 8)])
def test_the_float64_order_is_decided_on_all_but_one_percent_of_the_pixels(C, K):
    """The condition of tests/test_topk_gpu.py's exact-order check, on the float64 side alone: randn * 6 head-resolution logits enlarged bilinearly 16 -> 64
    leave at most 1 % of the pixels with one of the first min(K, C - 1) gaps inside the bound."""
    x = F.interpolate(CR.planted_logits(4, C, 1000 + C), (64, 64), mode="bilinear", align_corners=False)
    for it in (None, float(np.float32(1 / 2.5))):
        P, D = TR.float64_probabilities(x, it)
        share = float(TR.undecided(P, TR.eps_of(D, C, it is not None), K).double().mean())
        print(f"C={C} K={K} it={it}: undecided share {share:.5f}, D up to {float(D.max()):.1f}")
        assert share <= 0.01 and float(D.max()) < 87


# ---- 2. the metrics

def test_topk_evaluator_metrics_on_hand_made_counts():
    from mmsa.evaluate import LabelPrep, TopKEvaluator, topk_accuracy_of, topk_recall_of
    # three classes, K = 2: rows = label class, columns = found at rank 0 / rank 1 / not among the two
    c = np.array([[6, 2, 2], [1, 3, 0], [0, 0, 0]], dtype=np.int64)
    acc = topk_accuracy_of(c)
    assert acc.dtype == np.float64 and acc.tolist() == [7 / 14, 12 / 14]
    rec = topk_recall_of(c)
    assert rec[0].tolist() == [0.6, 0.8] and rec[1].tolist() == [0.25, 1.0] and np.isnan(rec[2]).all()
    assert np.isnan(topk_accuracy_of(np.zeros((3, 3), dtype=np.int64))).all()
    te = TopKEvaluator(LabelPrep(3), 2, cases=["fog", "night"])
    host = np.stack([c, c[::-1].copy()])
    te.host_counts = lambda: host
    assert te.accuracy().tolist() == topk_accuracy_of(host.sum(0)).tolist() and te.accuracy(slot="night").tolist() == topk_accuracy_of(host[1]).tolist()
    assert np.array_equal(te.recall(slot="fog"), rec, equal_nan=True)
    s = te.summary(slot="fog")
    assert list(s) == ["top1", "top2", "mRecall1", "mRecall2"] and s["top1"] == 0.5 and s["top2"] == np.round(12 / 14 * 100, 2) / 100.0
    assert s["mRecall1"] == np.round((0.6 + 0.25) / 2 * 100, 2) / 100.0 and s["mRecall2"] == 0.9
    assert bool((np.diff(te.accuracy()) >= 0).all())
    assert te._trailing() == (3, 3) and te.k == 2 and te.host_counts().shape == (2, 3, 3)
    fresh = TopKEvaluator(LabelPrep(5), 8, images=4)
    assert fresh.host_counts().shape == (0, 5, 9) and fresh.n_slots == 4
    for bad in (0, 9, -1, 2.0, True, None):
        with pytest.raises(ValueError, match="TopKEvaluator: topk = .*1..8 ranks are supported"):
            TopKEvaluator(LabelPrep(3), bad)


# ---- 3. refusals, all before any launch

def test_python_refusals_of_topk():
    import mmsa
    import mmsa.inference as inf
    from mmsa.evaluate import MAX_TOPK, Calibration, Evaluator, LabelPrep, SelectiveEvaluator, TopKEvaluator
    assert MAX_TOPK == 8 and inf.TopK._fields == ("classes", "probs") and mmsa.TopK is inf.TopK
    x = torch.zeros(1, 6, 8, 8)
    lab = torch.zeros(1, 8, 8, dtype=torch.uint8)
    plan = inf.MapPlan.whole(1, 8, 8)
    aug = inf.AugPlan.make(dict(mode="whole"), [(1, 8, 8)] * 2)
    bufs = inf.TopK(torch.zeros(2, 1, 8, 8, dtype=torch.uint8), torch.zeros(2, 1, 8, 8))
    out = bufs.classes[0]

    def entries(**kw):
        """Every entry with `kw`, under its name: (name, call)."""
        return [("whole_class_map", lambda: inf.whole_class_map(None, None, x, **kw)),
                ("slide_class_map", lambda: inf.slide_class_map(None, None, x, (4, 4), (4, 4), **kw)),
                ("class_map", lambda: inf.class_map(None, None, x, dict(mode="whole"), **kw)),
                ("aug_class_map", lambda: inf.aug_class_map(None, None, [x], dict(mode="whole"), **kw))]

    for bad in (0, 9, -1, 2.0, True, "2"):
        for name, call in entries(topk=bad):
            with pytest.raises(ValueError, match=f"mmsa.{name}: topk = .*1..8 ranks are supported"):
                call()
        with pytest.raises(ValueError, match="mmsa.SlideRunner: topk = "):
            inf.SlideRunner(None, None, x, (4, 4), (4, 4), topk=bad)
        with pytest.raises(ValueError, match="mmsa.argmax_topk_map: topk = "):
            mmsa.argmax_topk_map(torch.zeros(1, 5, 4, 4), bad)
    # what a top-k map replaces, or has no variant of: by name, under the entry's name
    lp = LabelPrep(5)
    for kw, why in ((dict(confidence=True), "topk= with confidence=: the confidence map is plane 0 of the top-k probabilities; take topk.probs\\[0\\]"),
                    (dict(confidence=torch.zeros(1, 8, 8)), "topk= with confidence=: .*take topk.probs\\[0\\]"),
                    (dict(score="margin"), "topk= with score='margin': .*topk.probs\\[0\\] - topk.probs\\[1\\]"),
                    (dict(score="entropy", confidence=False), "topk= with score='entropy'"),
                    (dict(labels=lab, calibration=Calibration(lp)), "topk= with calibration=: .*run mmsa.calibration\\(topk.classes\\[r\\], topk.probs\\[r\\]"),
                    (dict(labels=lab, selective=SelectiveEvaluator(lp)), "topk= with selective=: .*run mmsa.selective\\(topk.classes\\[r\\], topk.probs\\[r\\]")):
        for name, call in entries(topk=2, **kw):
            with pytest.raises(RuntimeError, match=f"mmsa.{name}: " + why):
                call()
    for kw in (dict(fused=True), dict(return_map=False)):
        for name, call in entries(topk=2, **kw)[:2]:
            with pytest.raises(RuntimeError, match=f"mmsa.{name}: topk= with fused=True / return_map=False"):
                call()
        with pytest.raises(RuntimeError, match="mmsa.inference: topk= with fused=True / return_map=False"):
            plan.class_map(None, out, None, topk=bufs, **kw)
    for kw, why in ((dict(confidence=True), "topk= with confidence="), (dict(score="margin"), "topk= with score='margin'")):
        with pytest.raises(RuntimeError, match="mmsa.SlideRunner: " + why):
            inf.SlideRunner(None, None, x, (4, 4), (4, 4), topk=2, **kw)
    with pytest.raises(RuntimeError, match="mmsa.inference: topk= with confidence="):
        plan.class_map(None, out, None, topk=bufs, conf=torch.zeros(1, 8, 8))
    # one pass: not over augmented views, not at a rescaled or cut size
    why = "topk= with one_pass=True: there is no one-pass top-k launch at a rescaled or cut size or over augmented views"
    with pytest.raises(RuntimeError, match="mmsa.aug_class_map: " + why):
        inf.aug_class_map(None, None, [x, x], dict(mode="whole"), topk=2, one_pass=True)
    with pytest.raises(RuntimeError, match="mmsa.inference: " + why):
        aug.class_map([None, None], out, None, one_pass=True, topk=bufs)
    small = inf.MapPlan.whole(1, 8, 8, ori_shape=(6, 7))
    sb = inf.TopK(torch.zeros(2, 1, 6, 7, dtype=torch.uint8), torch.zeros(2, 1, 6, 7))
    with pytest.raises(RuntimeError, match="mmsa.inference: " + why):
        small.class_map(None, sb.classes[0], None, one_pass=True, topk=sb)
    # topk_evaluator= needs labels= and topk=, of the same K
    te = TopKEvaluator(lp, 2)
    for name, call in entries(topk_evaluator=te, labels=lab):
        with pytest.raises(RuntimeError, match=f"mmsa.{name}: topk_evaluator= needs the top-k map: pass topk=K"):
            call()
    for name, call in entries(topk_evaluator=te, topk=2):
        with pytest.raises(RuntimeError, match=f"mmsa.{name}: topk_evaluator= needs labels="):
            call()
    for name, call in entries(topk_evaluator=te, topk=3, labels=lab):
        with pytest.raises(RuntimeError, match=f"mmsa.{name}: topk_evaluator= counts 2 ranks, topk= gives 3"):
            call()
    for name, call in entries(topk_evaluator=Evaluator(lp), topk=2, labels=lab):
        with pytest.raises(RuntimeError, match=f"mmsa.{name}: topk_evaluator= takes an mmsa.evaluate.TopKEvaluator, got Evaluator"):
            call()
    # the buffers of a TopK are checked like the confidence buffer, at plan level on the host
    for bad, why in ((inf.TopK(torch.zeros(2, 1, 8, 8), bufs.probs), "the top-k classes buffer must be uint8"),
                     (inf.TopK(bufs.classes, torch.zeros(2, 1, 8, 8, dtype=torch.float64)), "the top-k probs buffer must be float32"),
                     (inf.TopK(torch.zeros(2, 1, 8, 9, dtype=torch.uint8), bufs.probs), "the top-k classes buffer has shape \\(2, 1, 8, 9\\)"),
                     (inf.TopK(torch.zeros(9, 1, 8, 8, dtype=torch.uint8), torch.zeros(9, 1, 8, 8)), "the top-k classes buffer has shape \\(9, 1, 8, 8\\).*with 1 <= K <= 8 is expected"),
                     (inf.TopK(bufs.classes, torch.zeros(3, 1, 8, 8)), "the top-k buffers disagree"),
                     (inf.TopK(bufs.classes, torch.zeros(1, 8, 8, 2).permute(3, 0, 1, 2)), "the top-k probs buffer must be contiguous"),
                     (inf.TopK(None, bufs.probs), "the top-k classes buffer must be a tensor")):
        with pytest.raises(RuntimeError, match="mmsa.inference: " + why):
            plan.class_map(None, out, None, topk=bad)
    with pytest.raises(RuntimeError, match="a plan's topk= is the TopK of buffers itself"):
        plan.class_map(None, out, None, topk=2)
    with pytest.raises(RuntimeError, match="pass out=topk.classes\\[0\\]"):
        plan.class_map(None, torch.zeros(1, 8, 8, dtype=torch.uint8), None, topk=bufs)
    # temperature= with topk= is accepted (a bad one is still the temperature's refusal); with neither it stays refused with today's message
    with pytest.raises(ValueError, match="temperature"):
        inf.whole_class_map(None, None, x, topk=2, temperature=0)
    with pytest.raises(RuntimeError, match="whole_class_map: temperature= without confidence=: the class map does not depend on the temperature"):
        inf.whole_class_map(None, None, x, temperature=2.0)
    # None is the default everywhere, and the augmented entries still take no temperature
    for fn in (inf.slide_class_map, inf.whole_class_map, inf.class_map, inf.aug_class_map, inf.MapPlan.class_map, inf.AugPlan.class_map, inf.SlideRunner.__init__):
        assert inspect.signature(fn).parameters["topk"].default is None, fn
    for fn in (inf.slide_class_map, inf.whole_class_map, inf.class_map, inf.aug_class_map, inf.MapPlan.class_map, inf.SlideRunner.run):
        assert inspect.signature(fn).parameters["topk_evaluator"].default is None, fn
    assert "temperature" not in inspect.signature(inf.aug_class_map).parameters
    assert inf.MapOptions().topk is None and inf.MapOptions().topk_evaluator is None
    for name in ("TopK", "argmax_topk_map", "TopKEvaluator", "topk_counts"):
        assert name in mmsa.__all__ and hasattr(mmsa, name)
    with pytest.raises(RuntimeError):                      # there is no CPU path
        mmsa.argmax_topk_map(torch.zeros(1, 5, 4, 4), 2)
    with pytest.raises(RuntimeError, match="classes must be a GPU tensor"):
        mmsa.topk_counts(bufs.classes, lab, lp)


# ---- 4. the C entries on the host

def test_the_entries_refuse_bad_arguments_on_the_host():
    """Before any launch, so no GPU is needed: every pointer is a fake but the window and slot tables, which the entries read on the host."""
    import mmsa
    fake = ctypes.c_void_p(256)
    win = (ctypes.c_int * 3)(0, 0, 0)
    slots = (ctypes.c_int * 1)(0)
    raw = mmsa.lib.raw

    def frame(K=2, C=5, it=1.0, logits=fake, classes=fake, probs=fake, unc=fake):
        rc = raw.mmsa_slide_argmax_topk(logits, 1, C, 4, 4, win, classes, probs, 1, 16, 16, 16, 16, unc, K, it, None)
        return (rc, mmsa.lib.last_error()) if rc else (0, "")

    def canvas(K=2, C=5, prob=fake, classes=fake, probs=fake):
        rc = raw.mmsa_argmax_topk_nchw(prob, None, classes, probs, 1, C, 4, 4, K, None)
        return (rc, mmsa.lib.last_error()) if rc else (0, "")

    def counts(K=2, C=5, classes=fake, label=fake, lut=fake, buf=fake, tab=slots):
        rc = raw.mmsa_eval_topk_u8(classes, K, label, 1, 4, 4, 4, 4, lut, C, None, None, tab, 1, buf, None)
        return (rc, mmsa.lib.last_error()) if rc else (0, "")

    ERR_ARG = -1     # MMSA_ERR_ARG (csrc/common.h)
    for K in (0, 9, -1, 100):
        for fn, name in ((frame, "slide_argmax_topk"), (canvas, "argmax_topk_nchw"), (counts, "eval_topk_u8")):
            rc, msg = fn(K=K)
            assert rc == ERR_ARG and f"{name}: K = {K}; 1..8 ranks are supported" in msg, (name, K, msg)
    for C in (256, 1000):
        for fn, name in ((frame, "slide_argmax_topk"), (canvas, "argmax_topk_nchw"), (counts, "eval_topk_u8")):
            rc, msg = fn(C=C)
            assert rc == ERR_ARG and f"{name}: {C} classes" in msg and "255" in msg, (name, C, msg)
    for kw in (dict(logits=None), dict(classes=None), dict(probs=None), dict(unc=None)):
        rc, msg = frame(**kw)
        assert rc == ERR_ARG and "slide_argmax_topk: logits, classes, probs and uncovered are required" in msg
    for kw in (dict(prob=None), dict(classes=None), dict(probs=None)):
        rc, msg = canvas(**kw)
        assert rc == ERR_ARG and "argmax_topk_nchw: prob, classes and probs are required" in msg
    rc, msg = counts(classes=None)
    assert rc == ERR_ARG and "eval_topk_u8: classes is required" in msg
    for kw in (dict(label=None), dict(lut=None), dict(buf=None), dict(tab=None)):
        rc, msg = counts(**kw)
        assert rc == ERR_ARG and "eval_topk_u8: label, lut, slots and counts are required" in msg
    for bad in (0.0, -2.0, float("nan"), float("inf")):
        rc, msg = frame(it=bad)
        assert rc == ERR_ARG and "slide_argmax_topk: inv_temperature" in msg


def test_the_entries_are_declared_bound_and_versioned():
    import mmsa
    hdr = open(os.path.join(ROOT, "include", "mmsa.h")).read()
    header = int(re.search(r"#define MMSA_ABI_VERSION (\d+)", open(os.path.join(ROOT, "include", "mmsa_version.h")).read()).group(1))
    assert mmsa.lib.version() == mmsa.lib.ABI_VERSION == header == 114
    for name in ENTRIES:
        assert re.search(r"\b" + name + r"\s*\(", hdr), f"{name} is not declared in include/mmsa.h"
        assert name in mmsa.lib.SIGNATURES and hasattr(mmsa.lib.raw, name)
        assert name.replace("mmsa_", "") in open(os.path.join(ROOT, "include", "mmsa_version.h")).read()
    assert len(mmsa.lib.SIGNATURES["mmsa_slide_argmax_topk"]) == len(mmsa.lib.SIGNATURES["mmsa_slide_argmax_conf_t"]) + 1
