"""Uncertainty maps on the device: the top-2 margin and the entropy score (csrc/softmax_px.h) written in the confidence's place by the launch that writes
the class map -- the `_score` launches against the canvas launch (mmsa_argmax_score_nchw on the canvas path's probabilities) bit for bit and against the
float64 scores within the bounds DESIGN.md section 2 derives, at the frame's size, at a rescaled / cut size, over augmented views and with a temperature;
uncovered pixels, the exact cases, the public entries of mmsa.inference on the tiny model, and the reference's own probabilities (tests/golden)."""
import dataclasses
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import aug_ref as AR
from tests import confidence_ref as CR
from tests import rescale_ref as RR
from tests import uncertainty_ref as UR
from tests.configs import CONFIGS, HEAD_CONFIGS, make_input
from tests.test_aug_gpu import GEOMETRIES
from tests.util import assert_close
from tests.weights import seeded_state_dict

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
RESCALES = [((77, 131), None), ((135, 201), None), ((135, 201), (60, 100))]      # down, up, a cut of the latter: those of tests/test_confidence_gpu.py
KINDS = sorted(UR.KINDS)


def _plan(geo, B=2, tgt=None, cut=None):
    import mmsa.inference as inf
    (H, W), stride = GEOMETRIES[geo]
    p = inf.MapPlan.slide(B, H, W, (64, 64), stride, tgt)
    return p if cut is None else dataclasses.replace(p, Ho=cut[0], Wo=cut[1])


def _run(plan, lg, **kw):
    """plan.class_map with a score buffer -> (map, score, uncovered count); both buffers are pre-filled with values no launch writes."""
    B, Ho, Wo = plan.size if hasattr(plan, "size") else (plan.B, plan.Ho, plan.Wo)
    out = torch.full((B, Ho, Wo), 77, dtype=torch.uint8, device=DEV)
    conf = torch.full((B, Ho, Wo), -1.0, device=DEV)
    unc = torch.zeros(1, dtype=torch.int32, device=DEV)
    plan.class_map(lg, out, unc, conf=conf, **kw)
    return out, conf, int(unc.item())


def _canvas(plan, lg, it=None):
    """One view the long way round -> (cut logits canvas, its argmax_map, its probabilities, canvas pixels without a window)."""
    import mmsa.inference as inf
    unc = torch.zeros(1, dtype=torch.int32, device=DEV)
    y = inf._canvas_logits(plan, lg, unc)[:, :, :plan.Ho, :plan.Wo].contiguous()
    p = torch.full_like(y, float("nan"))
    inf._softmax_accum(y, p, it=it)
    return y, inf.argmax_map(y), p, int(unc.item())


def _canvas_score(prob, kind):
    """mmsa_argmax_score_nchw alone -> (the argmax of the probabilities, the score)."""
    import mmsa
    return mmsa.argmax_score_map(prob, score=kind)


# ---- 1. the frame's size, one view

@pytest.mark.parametrize("geo", sorted(GEOMETRIES))
@pytest.mark.parametrize("C", [1, 2, 5, 33])
def test_frame_size_equals_the_canvas_launch_and_float64(C, geo):
    _frame_size_case(C, geo)


@pytest.mark.parametrize("geo", ["s40", "s24"])
@pytest.mark.parametrize("C", [64, 65])
def test_frame_size_on_both_sides_of_the_lds_limit(C, geo):
    """mmsa_slide_argmax_score keeps the pixel's values in LDS up to 64 classes (exactly 64 KiB at 64) and recomputes them in two more passes from 65 on."""
    _frame_size_case(C, geo)


def _frame_size_case(C, geo):
    from mmsa import lib, ops
    plan = _plan(geo)
    lg = CR.planted_logits(plan.n, C, 1000 + C).to(DEV)
    plain = torch.empty(plan.B, plan.Ho, plan.Wo, dtype=torch.uint8, device=DEV)
    lib.call("mmsa_slide_argmax", *plan._args(lg, plain), torch.zeros(1, dtype=torch.int32, device=DEV).data_ptr(), ops._stream())
    y, want, prob, unc2 = _canvas(plan, lg)
    same = lg[:, :1].expand(-1, C, -1, -1).contiguous()
    ahead = lg.clone()
    ahead[:, C // 2] += 300.0
    tie = lg.clone()
    tie[:, 0] = lg.max(1).values + 2.0
    tie[:, C - 1] = tie[:, 0]
    one = torch.ones(plan.B, plan.Ho, plan.Wo, device=DEV)
    for kind in KINDS:
        got, score, unc = _run(plan, lg, score=kind)
        _, want_score = _canvas_score(prob, kind)
        worst, D = UR.float64_check(score, y, kind)
        diff = int((score != want_score).sum().item())
        print(f"{kind} {geo} C={C}: {diff} of {score.numel()} scores differ from the canvas launch; D up to {D:.1f}, worst error / float64 bound {worst:.3f}; "
              f"score in [{score.min().item():.3e}, {score.max().item():.3e}]")
        assert unc == 0 and unc2 == 0 and torch.equal(got, plain) and torch.equal(got, want)
        assert torch.equal(score, want_score), f"{kind} {geo} C={C}: the one-pass score is not the canvas launch's, bit for bit"
        assert (30 <= D or C == 1) and D < 87 and worst <= 1.0
        assert bool((score >= 0).all()) and bool((score <= 1).all())
        if C == 1:
            assert torch.equal(score, one), f"{kind}: one class is certain"
            continue
        # one class ahead by more than 104: every other exponential is 0.0f -- both scores exactly 1
        got, score, _ = _run(plan, ahead, score=kind)
        assert bool((got == C // 2).all()) and torch.equal(score, one), f"{kind}: one class ahead"
        # every class the same plane: margin exactly 0; entropy score within its bound of 0 and never below
        got, score, _ = _run(plan, same, score=kind)
        ys = _canvas(plan, same)[0]
        assert bool((got == 0).all()) and bool((score >= 0).all())
        if kind == "margin":
            assert bool((score == 0).all()), "equal logits: margin exactly 0"
            assert bool((_run(plan, tie, score=kind)[1] == 0).all()), "a two-way tie at the top: margin exactly 0"
        else:
            assert UR.float64_check(score, ys, kind)[0] <= 1.0 and float(UR.float64_scores(ys)["entropy"].abs().max()) < 1e-15


# ---- 2. the rescaled / cut size

@pytest.mark.parametrize("geo", sorted(GEOMETRIES))
@pytest.mark.parametrize("C", [5, 33])
def test_rescaled_size_both_launches_equal_the_canvas_launch(C, geo):
    for tgt, cut in RESCALES:
        plan = _plan(geo, 2, tgt, cut)
        lg = CR.planted_logits(plan.n, C, 2000 + C).to(DEV)
        y, want, prob, unc2 = _canvas(plan, lg)
        for kind in KINDS:
            _, want_score = _canvas_score(prob, kind)
            res = {}
            for one_pass in (True, False):
                got, score, unc = res[one_pass] = _run(plan, lg, one_pass=one_pass, score=kind)
                diff = int((score != want_score).sum().item())
                print(f"{kind} {geo} C={C} target {tgt} cut {cut} one_pass={one_pass}: {diff} of {score.numel()} scores differ, uncovered {unc}")
                assert unc == 0 and unc2 == 0 and got.shape == (2,) + (cut or tgt) and torch.equal(got, want), f"map, one_pass={one_pass}"
                assert torch.equal(score, want_score), f"{kind} {geo} C={C} target {tgt} cut {cut} one_pass={one_pass}"
            assert torch.equal(res[True][0], res[False][0]) and torch.equal(res[True][1], res[False][1])
            worst, D = UR.float64_check(res[True][1], y, kind)
            assert D < 87 and worst <= 1.0


# ---- 3. augmented views

def _aug_plan(tgt, cut):
    import mmsa.inference as inf
    return inf.AugPlan(tuple(_plan(g, 2, tgt, cut) for g in ("s40", "s64", "s24", "s40")), (0, 1, 2, 1))


def _aug_logits(plan, C, seed):
    g = torch.Generator().manual_seed(seed)
    return [torch.randn(p.n, C, 16, 16, generator=g).to(DEV) for p in plan.plans]


@pytest.mark.parametrize("C", [5, 33])
def test_augmented_equals_the_canvas_launch_on_the_mean_probabilities(C):
    """Four views (overlap up to 4, shifted windows), flips [-, h, v, h]: the score of the MEAN probabilities, by the canvas path whatever the default."""
    import mmsa.inference as inf
    for tgt, cut in RESCALES:
        plan = _aug_plan(tgt, cut)
        lgs = _aug_logits(plan, C, 200 + C)
        prob = plan.mean_probabilities(lgs, torch.zeros(1, dtype=torch.int32, device=DEV))
        want = inf.argmax_map(prob)
        for kind in KINDS:
            want_map, want_score = _canvas_score(prob, kind)
            assert torch.equal(want_map, want)
            for one_pass in (None, False):
                got, score, unc = _run(plan, lgs, one_pass=one_pass, score=kind)
                assert unc == 0 and torch.equal(got, want) and torch.equal(score, want_score), f"{kind} C={C} target {tgt} cut {cut} one_pass={one_pass}"
            assert bool((want_score >= 0).all()) and bool((want_score <= 1).all())
            p64 = prob.double().cpu()
            if kind == "margin":                 # one float32 subtraction of two stored float32 values
                top = p64.topk(2, dim=1).values
                assert float((want_score.double().cpu() - (top[:, 0] - top[:, 1])).abs().max()) <= 2.0 ** -24
            with pytest.raises(RuntimeError, match="with one_pass=True: the one-pass augmented launch"):
                _run(plan, lgs, one_pass=True, score=kind)


# ---- 4. with a temperature

@pytest.mark.parametrize("C", [5, 33])
def test_temperature_combines_with_the_score(C):
    from mmsa.evaluate import inv_temperature
    for tgt in (None, (77, 131)):
        plan = _plan("s40", 2, tgt)
        lg = CR.planted_logits(plan.n, C, 3000 + C).to(DEV)
        ops = (None,) if tgt is None else (True, False)
        for kind in KINDS:
            for op in ops:
                plain = _run(plan, lg, one_pass=op, score=kind)
                at1 = _run(plan, lg, one_pass=op, score=kind, temperature=1)
                assert torch.equal(at1[0], plain[0]) and torch.equal(at1[1], plain[1]), f"{kind} target {tgt} one_pass={op}: T = 1 is the untempered result"
            for T in (0.5, 2.3):
                it = inv_temperature(T)
                y, want, prob, _ = _canvas(plan, lg, it=it)
                _, want_score = _canvas_score(prob, kind)
                for op in ops:
                    got, score, unc = _run(plan, lg, one_pass=op, score=kind, temperature=T)
                    assert unc == 0 and torch.equal(got, want) and torch.equal(score, want_score), f"{kind} T={T} target {tgt} one_pass={op}"
                worst, DT = UR.float64_check(want_score, y, kind, it)
                print(f"{kind} C={C} T={T} target {tgt}: D_T up to {DT:.1f}, worst error / tempered bound {worst:.3f}")
                assert DT < 87 and worst <= 1.0


# ---- 5. uncovered pixels

def test_uncovered_pixels_have_score_zero_and_are_counted_once():
    """The strip of tests/test_confidence_gpu.py::test_uncovered_pixels_have_confidence_zero_and_are_counted_once: two windows leave columns 64 .. 87 of
    a 64 x 88 frame uncovered -- at the rescaled size (a tap without a window) and at the frame's own size (no window over a pixel)."""
    import mmsa.inference as inf
    tgt = (96, 120)
    strip = inf.MapPlan(2, 64, 88, 64, 64, ((0, 0, 0), (1, 0, 0)), tgt[0], tgt[1], tgt[0], tgt[1])
    lg = torch.randn(2, 5, 16, 16, generator=torch.Generator().manual_seed(3)).to(DEV)
    count = np.zeros((2, 64, 88), dtype=np.float32)
    count[:, :, :64] = 1
    bad = torch.from_numpy(RR.touches_uncovered(count, tgt[0], tgt[1])).to(DEV)
    flat = dataclasses.replace(strip, Hd=64, Wd=88, Ho=64, Wo=88)
    for kind in KINDS:
        got, score, unc = _run(strip, lg, one_pass=True, score=kind)
        _, want, prob, _ = _canvas(strip, lg)
        _, want_score = _canvas_score(prob, kind)
        assert 0 < int(bad.sum()) < bad.numel() and unc == int(bad.sum()) and bool((got[bad] == 255).all()) and bool((score[bad] == 0).all())
        assert torch.equal(got[~bad], want[~bad]) and torch.equal(score[~bad], want_score[~bad])
        got, score, unc = _run(flat, lg, score=kind)
        _, want, prob, _ = _canvas(flat, lg)
        _, want_score = _canvas_score(prob, kind)
        assert unc == 2 * 64 * 24 and bool((got[:, :, 64:] == 255).all()) and bool((score[:, :, 64:] == 0).all())
        assert torch.equal(got[:, :, :64], want[:, :, :64]) and torch.equal(score[:, :, :64], want_score[:, :, :64])


# ---- 6. the public entries on the tiny model

@pytest.fixture(scope="module")
def models():
    import mmsa
    cfg, hcfg = CONFIGS["tiny256"], HEAD_CONFIGS["head_tiny"]
    m = mmsa.build_backbone(dict(type="SAMAdapterbimodalMixModNewInTwinConvNEW", **cfg["kwargs"]))
    m.load_state_dict(seeded_state_dict(m, seed=cfg["seed"]))
    h = mmsa.build_head(dict(type="SegformerHead", **hcfg["kwargs"]))
    h.load_state_dict(seeded_state_dict(h, seed=hcfg["seed"]))
    h = h.to(DEV)
    g = torch.Generator().manual_seed(9)
    frame = torch.randn(1, 6, 320, 400, generator=g)
    frame[:, 3:] = (torch.rand(1, 3, 320, 400, generator=g) < 0.05).float() * torch.rand(1, 3, 320, 400, generator=g)
    return cfg, m, h, frame.to(DEV), make_input(cfg, batch=2, seed=17).to(DEV)


SLIDE_CFG = dict(mode="slide", crop_size=(256, 256), stride=(170, 170))
NUM_CLASSES = HEAD_CONFIGS["head_tiny"]["kwargs"]["num_classes"]


def _buffer(shape):
    return torch.full(shape, -1.0, device=DEV)


@pytest.mark.parametrize("kind", KINDS)
def test_slide_and_whole_entries(models, kind):
    import mmsa
    import mmsa.inference as inf
    cfg, m, h, frame, x = models
    for ori in (None, (300, 380, 3)):
        want = mmsa.argmax_score_map(inf.probabilities(m, h, frame, SLIDE_CFG, ori_shape=ori, max_batch=2), score=kind)[1]
        plain = inf.slide_class_map(m, h, frame, (256, 256), (170, 170), max_batch=2, ori_shape=ori)
        for given in (True, _buffer(want.shape)):
            cm, unc, conf = inf.slide_class_map(m, h, frame, (256, 256), (170, 170), max_batch=2, ori_shape=ori, confidence=given, score=kind)
            assert int(unc.item()) == 0 and torch.equal(cm, plain[0]) and torch.equal(conf, want) and (given is True or conf is given), f"slide ori_shape={ori}"
        if ori is not None:
            for one_pass in (True, False):          # None is the measured default, the canvas path: both launches by name as well
                conf = inf.slide_class_map(m, h, frame, (256, 256), (170, 170), max_batch=2, ori_shape=ori, confidence=True, one_pass=one_pass, score=kind)[2]
                assert torch.equal(conf, want), f"slide ori_shape={ori} one_pass={one_pass}"
            wt = mmsa.argmax_score_map(inf.probabilities(m, h, frame, SLIDE_CFG, ori_shape=ori, max_batch=2, temperature=2.3), score=kind)[1]
            for one_pass in (None, True):
                conf = inf.slide_class_map(m, h, frame, (256, 256), (170, 170), max_batch=2, ori_shape=ori, confidence=True, score=kind, temperature=2.3,
                                           one_pass=one_pass)[2]
                assert torch.equal(conf, wt) and not torch.equal(wt, want)
    cases = [(dict(ori_shape=(200, 310)), dict(mode="whole"), dict(ori_shape=(200, 310))), (dict(dim=(192, 240)), dict(mode="whole_dim", dim=(192, 240)), {}),
             (dict(dim=(200, 300), cut_dim=(260, 150)), dict(mode="whole_dim_cut", dim=(200, 300), cut_dim=(260, 150)), {}), ({}, dict(mode="whole"), {})]
    for kw, tc, pkw in cases:
        want = mmsa.argmax_score_map(inf.probabilities(m, h, x, tc, **pkw), score=kind)[1]
        plain = inf.whole_class_map(m, h, x, **kw)
        for given in (True, _buffer(want.shape)):
            cm, conf = inf.whole_class_map(m, h, x, confidence=given, score=kind, **kw)
            assert torch.equal(cm, plain) and torch.equal(conf, want) and (given is True or conf is given), f"whole {kw}"
        if kw:
            cm, conf = inf.whole_class_map(m, h, x, confidence=True, score=kind, one_pass=True, **kw)
            assert torch.equal(cm, plain) and torch.equal(conf, want), f"whole {kw} one_pass=True"
    # score="max" is the confidence, and the refusals of the confidence hold for a score: by name, before anything runs
    assert torch.equal(inf.whole_class_map(m, h, x, confidence=True, score="max")[1], inf.whole_class_map(m, h, x, confidence=True)[1])
    assert torch.equal(mmsa.argmax_score_map(inf.probabilities(m, h, x, dict(mode="whole")), score="max")[1], inf.whole_class_map(m, h, x, confidence=True)[1])
    for kw in (dict(fused=True), dict(return_map=False)):
        with pytest.raises(RuntimeError, match="whole_class_map: confidence with fused=True / return_map=False"):
            inf.whole_class_map(m, h, x, confidence=True, score=kind, **kw)
        with pytest.raises(RuntimeError, match="slide_class_map: confidence with fused=True / return_map=False"):
            inf.slide_class_map(m, h, frame, (256, 256), (170, 170), confidence=True, score=kind, **kw)


@pytest.mark.parametrize("kind", KINDS)
def test_class_map_modes_and_aug_entry(models, kind):
    import mmsa
    import mmsa.inference as inf
    cfg, m, h, frame, x = models
    cfgs = [SLIDE_CFG, dict(mode="whole"), dict(mode="whole_dim", dim=(300, 280)), dict(mode="whole_dim_cut", dim=(300, 280), cut_dim=(250, 270))]
    for tc in cfgs:
        img = frame if tc["mode"] == "slide" else x
        want = mmsa.argmax_score_map(inf.probabilities(m, h, img, tc, ori_shape=(210, 333, 3)), score=kind)[1]
        plain = inf.class_map(m, h, img, tc, ori_shape=(210, 333, 3))
        for given in (True, _buffer(want.shape)):
            cm, conf = inf.class_map(m, h, img, tc, ori_shape=(210, 333, 3), confidence=given, score=kind)
            assert torch.equal(cm, plain) and torch.equal(conf, want) and (given is True or conf is given), f"class_map {tc}"
    big = F.interpolate(frame, (400, 500), mode="bilinear", align_corners=False)
    imgs, flips, ori = [frame, frame.flip(3), big, big.flip(3)], [None, "horizontal", None, "horizontal"], (300, 380, 3)
    want = mmsa.argmax_score_map(inf.aug_inference(m, h, imgs, SLIDE_CFG, ori_shape=ori, flips=flips, max_batch=4), score=kind)[1]
    plain = inf.aug_class_map(m, h, imgs, SLIDE_CFG, ori_shape=ori, flips=flips, max_batch=4)
    for one_pass in (None, False):
        for given in (True, _buffer(want.shape)):
            cm, unc, conf = inf.aug_class_map(m, h, imgs, SLIDE_CFG, ori_shape=ori, flips=flips, max_batch=4, one_pass=one_pass, confidence=given, score=kind)
            assert int(unc.item()) == 0 and torch.equal(cm, plain[0]) and torch.equal(conf, want) and (given is True or conf is given), f"aug one_pass={one_pass}"
    with pytest.raises(RuntimeError, match="aug_class_map: score='" + kind + "' with one_pass=True"):
        inf.aug_class_map(m, h, imgs, SLIDE_CFG, ori_shape=ori, flips=flips, max_batch=4, one_pass=True, confidence=True, score=kind)


def test_calibration_and_selective_see_the_margin(models):
    """calibration= / selective= fed by a margin map are mmsa.calibration / mmsa.selective of the stored map and margin, byte for byte; and the area under
    the selective curve is a number per score."""
    import mmsa
    import mmsa.inference as inf
    from mmsa.evaluate import Calibration, LabelPrep, SelectiveEvaluator
    cfg, m, h, frame, x = models
    lp = LabelPrep(NUM_CLASSES)
    g = torch.Generator().manual_seed(4)
    lab_w = torch.randint(0, NUM_CLASSES, (2, 256, 256), generator=g, dtype=torch.uint8).to(DEV)
    lab_o = torch.randint(0, NUM_CLASSES, (2, 200, 310), generator=g, dtype=torch.uint8).to(DEV)
    for call, lab in ((lambda **kw: inf.whole_class_map(m, h, x, **kw), lab_w), (lambda **kw: inf.whole_class_map(m, h, x, ori_shape=(200, 310), **kw), lab_o),
                      (lambda **kw: inf.aug_class_map(m, h, [x, x.flip(3)], dict(mode="whole"), ori_shape=(200, 310), flips=[None, "horizontal"], **kw), lab_o)):
        cal, se = Calibration(lp, images=2, device=DEV), SelectiveEvaluator(lp, images=2, device=DEV)
        r = call(labels=lab, confidence=True, score="margin", calibration=cal, selective=se)
        cm, margin = r[0], r[-1]
        assert not torch.equal(margin, call(confidence=True)[-1])
        assert cal.bins.cpu().numpy().tobytes() == mmsa.calibration(cm, margin, lab, lp).cpu().numpy().tobytes() and int(cal.bins[:, 0].sum()) == lab.numel()
        assert se.counts.cpu().numpy().tobytes() == mmsa.selective(cm, margin, lab, lp).cpu().numpy().tobytes() and int(se.counts.sum()) == lab.numel()
        auc = se.auc()
        assert 0.0 <= auc <= 1.0 and se.summary(auc=True)["AURC"] == np.round(auc * 100, 2) / 100.0


def test_score_launches_replay_from_a_captured_graph(models):
    import mmsa.inference as inf
    cfg, m, h, frame, x = models
    lg = h(m(x)[0]).contiguous()
    prob = inf.probabilities(m, h, x, dict(mode="whole"))
    for kind in KINDS:
        for plan, kw in ((inf.MapPlan.whole(2, 256, 256), {}), (inf.MapPlan.whole(2, 256, 256, ori_shape=(200, 310)), dict(one_pass=True))):
            want_map, want_score, _ = _run(plan, lg, score=kind, **kw)
            out, conf, unc = torch.zeros_like(want_map), torch.zeros_like(want_score), torch.zeros(1, dtype=torch.int32, device=DEV)
            torch.cuda.synchronize()
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph):
                plan.class_map(lg, out, unc, conf=conf, score=kind, **kw)
            out.zero_()
            conf.zero_()
            graph.replay()
            torch.cuda.synchronize()
            assert torch.equal(out, want_map) and torch.equal(conf, want_score) and int(unc.item()) == 0, (kind, kw)
        want_map, want_score = _canvas_score(prob, kind)
        out, conf = torch.zeros_like(want_map), torch.zeros_like(want_score)
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            inf._argmax_score_into(prob, out, conf, UR.KINDS[kind])
        out.zero_()
        conf.zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, want_map) and torch.equal(conf, want_score), kind


@pytest.mark.parametrize("kind", KINDS)
def test_runner_keeps_a_static_score_buffer(models, kind):
    import mmsa.inference as inf
    cfg, m, h, frame, x = models
    for ori in (None, (300, 380, 3)):
        cm, _, want = inf.slide_class_map(m, h, frame, (256, 256), (170, 170), max_batch=2, ori_shape=ori, confidence=True, score=kind)
        sr = inf.SlideRunner(m, h, frame, (256, 256), (170, 170), chains=2, ori_shape=ori, confidence=True, score=kind, one_pass=None if ori is None else True)
        assert sr.conf.shape == want.shape and sr.conf.dtype == torch.float32
        for _ in range(2):
            res = sr.run()
            conf = res.confidence()
            torch.cuda.synchronize()
            assert conf is sr.conf and torch.equal(conf, want) and torch.equal(res.outputs()[0], cm)
        with pytest.raises(RuntimeError, match="SlideRunner.run: confidence with fused=True"):
            sr.run(fused=True)


# ---- 7. against the reference's own outputs

def _toy():
    w = torch.randn(RR.NUM_CLASSES, 6, 1, 1, generator=torch.Generator().manual_seed(RR.TOY_SEED)).to(DEV)
    return (lambda im: ([F.avg_pool2d(im, 4)], None)), (lambda feats: F.conv2d(feats[0], w).contiguous())


def _scores64(p):
    """Both scores in float64 from float64 probabilities [B, C, H, W]."""
    top = p.topk(2, dim=1).values
    H = -(torch.where(p > 0, p * torch.log(torch.where(p > 0, p, torch.ones_like(p))), torch.zeros_like(p))).sum(1)
    return dict(margin=top[:, 0] - top[:, 1], entropy=(1.0 - H / np.log(float(p.shape[1]))).clamp_min(0.0))


@pytest.mark.parametrize("tag", sorted(AR.CASES))
def test_against_the_reference_aug_fixture(golden_dir, tag):
    """The scores against those formed in float64 from the reference's own averaged probabilities.  Case `slide` (3 x 3 windows on some pixels) is refused by
    aug_class_map as it is without a score; its scores come from argmax_score_map(aug_inference(...))."""
    import mmsa.inference as inf
    g = np.load(os.path.join(golden_dir, "aug.npz"))
    case = AR.case_of(g[f"{tag}_cfg"])
    hw, crop, stride, ori, _ = case
    imgs, flips = AR.views_of(case)
    imgs = [v.to(DEV) for v in imgs]
    want = _scores64(torch.from_numpy(g[f"{tag}_prob"]).double())
    bb, hd = _toy()
    tc = dict(mode="whole") if crop is None else dict(mode="slide", crop_size=crop, stride=stride)
    for kind in KINDS:
        if tag == "slide":
            with pytest.raises(RuntimeError, match="covers some pixels 9 times"):
                inf.aug_class_map(bb, hd, imgs, tc, ori_shape=ori, flips=flips, confidence=True, score=kind)
            _, score = inf.argmax_score_map(inf.aug_inference(bb, hd, imgs, tc, ori_shape=ori, flips=flips), score=kind)
        else:
            _, unc, score = inf.aug_class_map(bb, hd, imgs, tc, ori_shape=ori, flips=flips, confidence=True, score=kind)
            assert int(unc.item()) == 0
        r, mx = assert_close(score, want[kind], what=f"{kind}, case {tag}")
        print(f"aug {tag}: {kind} rel_l2 {r:.2e} max_rel {mx:.2e}")


@pytest.mark.parametrize("tag", ["a", "c", "w"])
def test_against_the_reference_rescale_fixture(golden_dir, tag):
    import mmsa.inference as inf
    g = np.load(os.path.join(golden_dir, "rescale.npz"))
    hw, crop, stride, ori = RR.case_of(g[f"{tag}_cfg"])
    want = _scores64(torch.softmax(torch.from_numpy(g[f"{tag}_out"]).double(), 1))
    bb, hd = _toy()
    img = RR.frame(hw).to(DEV)
    for kind in KINDS:
        for one_pass in (None, True, False):
            if crop is None:
                _, score = inf.whole_class_map(bb, hd, img, ori_shape=ori, confidence=True, one_pass=one_pass, score=kind)
            else:
                _, unc, score = inf.slide_class_map(bb, hd, img, crop, stride, ori_shape=ori, confidence=True, one_pass=one_pass, score=kind)
                assert int(unc.item()) == 0
            r, mx = assert_close(score, want[kind], what=f"{kind}, case {tag}, one_pass={one_pass}")
            print(f"rescale {tag} one_pass={one_pass}: {kind} rel_l2 {r:.2e} max_rel {mx:.2e}")
