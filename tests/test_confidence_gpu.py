"""Confidence maps on the device: conf = max_c P[c] (ED:449,460) written by the launch that writes the class map -- the `_conf` siblings of the one-pass
kernels against the canvas path (logits canvas -> mmsa_softmax_flip_accum_nchw -> max over the classes) bit for bit and against the float64 softmax, at the
frame's size, at a rescaled / cut size and over augmented views; uncovered pixels, exact ties, the public entries of mmsa.inference on the tiny model, and
the reference's own probabilities (tests/golden/aug.npz, tests/golden/rescale.npz)."""
import dataclasses
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import aug_ref as AR
from tests import confidence_ref as CR
from tests import rescale_ref as RR
from tests.configs import CONFIGS, HEAD_CONFIGS, make_input
from tests.test_aug_gpu import GEOMETRIES
from tests.util import assert_close
from tests.weights import seeded_state_dict

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
RESCALES = [((77, 131), None), ((135, 201), None), ((135, 201), (60, 100))]      # down, up, a cut of the latter


def _plan(geo, B=2, tgt=None, cut=None):
    import mmsa.inference as inf
    (H, W), stride = GEOMETRIES[geo]
    p = inf.MapPlan.slide(B, H, W, (64, 64), stride, tgt)
    return p if cut is None else dataclasses.replace(p, Ho=cut[0], Wo=cut[1])


def _run(plan, lg, **kw):
    """plan.class_map with a confidence buffer -> (map, conf, uncovered count); both buffers are pre-filled with values no launch writes."""
    B, Ho, Wo = plan.size if hasattr(plan, "size") else (plan.B, plan.Ho, plan.Wo)
    out = torch.full((B, Ho, Wo), 77, dtype=torch.uint8, device=DEV)
    conf = torch.full((B, Ho, Wo), -1.0, device=DEV)
    unc = torch.zeros(1, dtype=torch.int32, device=DEV)
    plan.class_map(lg, out, unc, conf=conf, **kw)
    return out, conf, int(unc.item())


def _canvas(plan, lg):
    """One view the long way round -> (cut logits canvas, its argmax_map, the maximum over the classes of its softmax, canvas pixels without a window)."""
    import mmsa.inference as inf
    unc = torch.zeros(1, dtype=torch.int32, device=DEV)
    y = inf._canvas_logits(plan, lg, unc)[:, :, :plan.Ho, :plan.Wo].contiguous()
    p = torch.full_like(y, float("nan"))
    inf._softmax_accum(y, p)
    return y, inf.argmax_map(y), p.max(1).values, int(unc.item())


# ---- 1. the frame's size, one view

@pytest.mark.parametrize("geo", sorted(GEOMETRIES))
@pytest.mark.parametrize("C", [1, 5, 33])
def test_frame_size_equals_the_canvas_path_and_float64(C, geo):
    _frame_size_case(C, geo)


@pytest.mark.parametrize("geo", ["s40", "s24"])
@pytest.mark.parametrize("C", [64, 65])
def test_frame_size_on_both_sides_of_the_lds_limit(C, geo):
    """mmsa_slide_argmax_conf keeps the pixel's values in LDS up to 64 classes (exactly 64 KiB at 64) and recomputes them in a second pass from 65 on."""
    _frame_size_case(C, geo)


def _frame_size_case(C, geo):
    from mmsa import lib, ops
    plan = _plan(geo)
    one = torch.tensor(1.0) / torch.tensor(float(C))
    lg = CR.planted_logits(plan.n, C, 1000 + C).to(DEV)
    got, conf, unc = _run(plan, lg)
    plain = torch.empty_like(got)
    word = torch.zeros(1, dtype=torch.int32, device=DEV)
    lib.call("mmsa_slide_argmax", *plan._args(lg, plain), word.data_ptr(), ops._stream())
    y, want, want_conf, unc2 = _canvas(plan, lg)
    worst, D = CR.float64_check(conf, y)
    diff = int((conf != want_conf).sum().item())
    print(f"{geo} C={C}: {diff} of {conf.numel()} confidences differ from the canvas path; D up to {D:.1f}, worst error / float64 bound {worst:.3f}; "
          f"conf in [{conf.min().item():.3e}, {conf.max().item():.3e}]")
    assert unc == 0 and unc2 == 0 and torch.equal(got, plain) and torch.equal(got, want)
    assert torch.equal(conf, want_conf), f"{geo} C={C}: the one-pass confidence is not the canvas path's, bit for bit"
    assert (D >= 30 or C == 1) and worst <= 1.0
    assert bool((conf >= one.item()).all()) and bool((conf <= 1).all())
    if C == 1:
        assert bool((conf == 1).all())
    # every class the same plane: exactly 1.0f / (float)C, first class
    same = lg[:, :1].expand(-1, C, -1, -1).contiguous()
    got, conf, _ = _run(plan, same)
    assert bool((got == 0).all()) and bool((conf == one.item()).all()), "equal logits must give exactly 1 / C"
    # one class ahead by more than 104: every other exponential is 0.0f, exactly 1.0
    ahead = lg.clone()
    ahead[:, C // 2] += 300.0
    got, conf, _ = _run(plan, ahead)
    assert bool((got == C // 2).all()) and bool((conf == 1).all())


# ---- 2. the rescaled / cut size

@pytest.mark.parametrize("geo", sorted(GEOMETRIES))
@pytest.mark.parametrize("C", [5, 33])
def test_rescaled_size_both_launches_equal_the_canvas_path(C, geo):
    for tgt, cut in RESCALES:
        plan = _plan(geo, 2, tgt, cut)
        lg = CR.planted_logits(plan.n, C, 2000 + C).to(DEV)
        y, want, want_conf, unc2 = _canvas(plan, lg)
        res = {}
        for one_pass in (True, False):
            got, conf, unc = res[one_pass] = _run(plan, lg, one_pass=one_pass)
            diff = int((conf != want_conf).sum().item())
            print(f"{geo} C={C} target {tgt} cut {cut} one_pass={one_pass}: {diff} of {conf.numel()} confidences differ, uncovered {unc}")
            assert unc == 0 and unc2 == 0 and got.shape == (2,) + (cut or tgt) and torch.equal(got, want), f"map, one_pass={one_pass}"
            assert torch.equal(conf, want_conf), f"{geo} C={C} target {tgt} cut {cut} one_pass={one_pass}"
        assert torch.equal(res[True][0], res[False][0]) and torch.equal(res[True][1], res[False][1])
        worst, _ = CR.float64_check(res[True][1], y)
        assert worst <= 1.0
        # the plain launch next to it still writes the same map
        plain = torch.empty_like(want)
        plan.class_map(lg, plain, torch.zeros(1, dtype=torch.int32, device=DEV), one_pass=True)
        assert torch.equal(plain, want)


# ---- 3. augmented views

def _aug_plan(tgt, cut):
    import mmsa.inference as inf
    return inf.AugPlan(tuple(_plan(g, 2, tgt, cut) for g in ("s40", "s64", "s24", "s40")), (0, 1, 2, 1))


def _aug_logits(plan, C, seed):
    g = torch.Generator().manual_seed(seed)
    return [torch.randn(p.n, C, 16, 16, generator=g).to(DEV) for p in plan.plans]


@pytest.mark.parametrize("C", [5, 33, 70])
def test_augmented_both_launches_equal_the_mean_probabilities(C):
    """Four views (overlap up to 4, shifted windows, the scanning form), flips [-, h, v, h]; 256 / 128 / 64 lanes per workgroup."""
    import mmsa.inference as inf
    for tgt, cut in RESCALES:
        plan = _aug_plan(tgt, cut)
        lgs = _aug_logits(plan, C, 200 + C)
        prob = plan.mean_probabilities(lgs, torch.zeros(1, dtype=torch.int32, device=DEV))
        want, want_conf = inf.argmax_map(prob), prob.max(1).values
        for one_pass in (True, None):
            got, conf, unc = _run(plan, lgs, one_pass=one_pass)
            diff = int((conf != want_conf).sum().item())
            print(f"aug C={C} target {tgt} cut {cut} one_pass={one_pass}: {diff} of {conf.numel()} confidences differ, uncovered {unc}")
            assert unc == 0 and torch.equal(got, want) and torch.equal(conf, want_conf), f"C={C} target {tgt} cut {cut} one_pass={one_pass}"
        assert bool((want_conf >= 1.0 / C - 1e-6).all()) and bool((want_conf <= 1).all())
        m2, c2 = inf.argmax_max_map(prob)
        assert torch.equal(m2, want) and torch.equal(c2, want_conf)


def test_one_unflipped_view_is_the_rescaled_result():
    import mmsa.inference as inf
    one = _plan("s40", 2, (77, 131))
    plan = inf.AugPlan((one,), (0,))
    lgs = _aug_logits(plan, 5, 301)
    single_map, single_conf, _ = _run(one, lgs[0], one_pass=True)
    near = RR.near_ties(_canvas(one, lgs[0])[0], 1e-6)      # logits so close that their exponentials may round to the same float
    for one_pass in (True, None):
        got, conf, unc = _run(plan, lgs, one_pass=one_pass)
        assert unc == 0 and torch.equal(got[~near], single_map[~near]) and near.float().mean().item() < 0.01
        assert torch.equal(conf, single_conf), "p / 1.0f is p: the confidence of one view is the single-view confidence everywhere"


# ---- 4. uncovered pixels

def test_uncovered_pixels_have_confidence_zero_and_are_counted_once():
    """The geometry of tests/test_aug_gpu.py::test_uncovered_pixels_are_255_mirrored_and_counted_once: the second view's windows leave columns 64 .. 87 of its
    64 x 88 frame uncovered, and the view is flipped horizontally."""
    import mmsa.inference as inf
    tgt = (96, 120)
    strip = inf.MapPlan(2, 64, 88, 64, 64, ((0, 0, 0), (1, 0, 0)), tgt[0], tgt[1], tgt[0], tgt[1])
    plan = inf.AugPlan((_plan("s40", 2, tgt), strip, _plan("s64", 2, tgt)), (0, 1, 2))
    lgs = _aug_logits(plan, 5, 3)
    count = np.zeros((2, 64, 88), dtype=np.float32)
    count[:, :, :64] = 1
    view_bad = torch.from_numpy(RR.touches_uncovered(count, tgt[0], tgt[1])).to(DEV)
    bad = view_bad.flip(2)
    prob = plan.mean_probabilities(lgs, torch.zeros(1, dtype=torch.int32, device=DEV))
    got, conf, unc = _run(plan, lgs, one_pass=True)
    assert 0 < int(bad.sum()) < bad.numel() and unc == int(bad.sum())
    assert bool((got[bad] == 255).all()) and bool((conf[bad] == 0).all())
    assert torch.equal(got[~bad], inf.argmax_map(prob)[~bad]) and torch.equal(conf[~bad], prob.max(1).values[~bad]) and bool((conf[~bad] > 0).all())
    # the same strip in one view: at the rescaled size, and at the frame's own size (no window over a pixel)
    got, conf, unc = _run(strip, lgs[1], one_pass=True)
    _, want, want_conf, _ = _canvas(strip, lgs[1])
    assert unc == int(view_bad.sum()) and bool((got[view_bad] == 255).all()) and bool((conf[view_bad] == 0).all())
    assert torch.equal(got[~view_bad], want[~view_bad]) and torch.equal(conf[~view_bad], want_conf[~view_bad])
    flat = dataclasses.replace(strip, Hd=64, Wd=88, Ho=64, Wo=88)
    got, conf, unc = _run(flat, lgs[1])
    _, want, want_conf, _ = _canvas(flat, lgs[1])
    assert unc == 2 * 64 * 24 and bool((got[:, :, 64:] == 255).all()) and bool((conf[:, :, 64:] == 0).all())
    assert torch.equal(got[:, :, :64], want[:, :, :64]) and torch.equal(conf[:, :, :64], want_conf[:, :, :64])


# ---- 5. exact ties

def test_exact_ties_same_confidence_first_class():
    """Class 5 is a copy of class 2 and both are the maximum everywhere: the map is 2 and the confidence is the same in every path."""
    import mmsa.inference as inf

    def tied(p, seed):
        lg = torch.randn(p.n, 7, 16, 16, generator=torch.Generator().manual_seed(seed)) * 0.1
        lg[:, 2] += 3.0
        lg[:, 5] = lg[:, 2]
        return lg.to(DEV)
    for geo in ("s40", "s24"):
        for tgt in (None, (135, 201), (77, 131)):
            plan = _plan(geo, 1, tgt)
            lg = tied(plan, 11)
            _, want, want_conf, _ = _canvas(plan, lg)
            assert bool((want == 2).all())
            for one_pass in ((None,) if tgt is None else (True, False)):
                got, conf, unc = _run(plan, lg, one_pass=one_pass)
                assert unc == 0 and bool((got == 2).all()) and torch.equal(conf, want_conf), f"{geo} target {tgt} one_pass={one_pass}"
            assert bool((want_conf < 0.5).all()), "two equal maxima share the probability"
    plan = inf.AugPlan(tuple(_plan(g, 1, (135, 201)) for g in ("s40", "s24", "s64")), (1, 0, 2))
    lgs = [tied(p, 11 + k) for k, p in enumerate(plan.plans)]
    prob = plan.mean_probabilities(lgs, torch.zeros(1, dtype=torch.int32, device=DEV))
    assert torch.equal(prob[:, 2], prob[:, 5])
    for one_pass in (True, None):
        got, conf, unc = _run(plan, lgs, one_pass=one_pass)
        assert unc == 0 and bool((got == 2).all()) and torch.equal(conf, prob.max(1).values)


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


def test_slide_and_whole_entries(models):
    import mmsa.inference as inf
    cfg, m, h, frame, x = models
    for ori in (None, (300, 380, 3)):
        want = inf.probabilities(m, h, frame, SLIDE_CFG, ori_shape=ori, max_batch=2).max(1).values
        plain = inf.slide_class_map(m, h, frame, (256, 256), (170, 170), max_batch=2, ori_shape=ori)
        assert len(plain) == 2 and plain[0].dtype == torch.uint8
        for given in (True, _buffer(want.shape)):
            cm, unc, conf = inf.slide_class_map(m, h, frame, (256, 256), (170, 170), max_batch=2, ori_shape=ori, confidence=given)
            assert int(unc.item()) == 0 and torch.equal(cm, plain[0]) and torch.equal(conf, want) and (given is True or conf is given), f"slide ori_shape={ori}"
        if ori is not None:
            conf = inf.slide_class_map(m, h, frame, (256, 256), (170, 170), max_batch=2, ori_shape=ori, confidence=True, one_pass=False)[2]
            assert torch.equal(conf, want)
    cases = [(dict(ori_shape=(200, 310)), dict(mode="whole"), dict(ori_shape=(200, 310))), (dict(dim=(192, 240)), dict(mode="whole_dim", dim=(192, 240)), {}),
             (dict(dim=(200, 300), cut_dim=(260, 150)), dict(mode="whole_dim_cut", dim=(200, 300), cut_dim=(260, 150)), {}), ({}, dict(mode="whole"), {})]
    for kw, tc, pkw in cases:
        want = inf.probabilities(m, h, x, tc, **pkw).max(1).values
        plain = inf.whole_class_map(m, h, x, **kw)
        assert isinstance(plain, torch.Tensor)
        for given in (True, _buffer(want.shape)):
            cm, conf = inf.whole_class_map(m, h, x, confidence=given, **kw)
            assert torch.equal(cm, plain) and torch.equal(conf, want) and (given is True or conf is given), f"whole {kw}"


def test_class_map_modes_and_aug_entry(models):
    import mmsa.inference as inf
    cfg, m, h, frame, x = models
    cfgs = [SLIDE_CFG, dict(mode="whole"), dict(mode="whole_dim", dim=(300, 280)), dict(mode="whole_dim_cut", dim=(300, 280), cut_dim=(250, 270))]
    for tc in cfgs:
        img = frame if tc["mode"] == "slide" else x
        want = inf.probabilities(m, h, img, tc, ori_shape=(210, 333, 3)).max(1).values
        plain = inf.class_map(m, h, img, tc, ori_shape=(210, 333, 3))
        assert isinstance(plain, torch.Tensor)
        for given in (True, _buffer(want.shape)):
            cm, conf = inf.class_map(m, h, img, tc, ori_shape=(210, 333, 3), confidence=given)
            assert torch.equal(cm, plain) and torch.equal(conf, want) and (given is True or conf is given), f"class_map {tc}"
    big = F.interpolate(frame, (400, 500), mode="bilinear", align_corners=False)
    imgs, flips, ori = [frame, frame.flip(3), big, big.flip(3)], [None, "horizontal", None, "horizontal"], (300, 380, 3)
    want = inf.aug_inference(m, h, imgs, SLIDE_CFG, ori_shape=ori, flips=flips, max_batch=4).max(1).values
    plain = inf.aug_class_map(m, h, imgs, SLIDE_CFG, ori_shape=ori, flips=flips, max_batch=4)
    assert len(plain) == 2
    for one_pass in (None, True):
        for given in (True, _buffer(want.shape)):
            cm, unc, conf = inf.aug_class_map(m, h, imgs, SLIDE_CFG, ori_shape=ori, flips=flips, max_batch=4, one_pass=one_pass, confidence=given)
            assert int(unc.item()) == 0 and torch.equal(cm, plain[0]) and torch.equal(conf, want) and (given is True or conf is given), f"aug one_pass={one_pass}"


def test_with_render_and_with_an_evaluator(models):
    import mmsa.inference as inf
    from mmsa.evaluate import Evaluator, LabelPrep
    from mmsa.preprocess import Preprocess
    from mmsa.render import Renderer
    cfg, m, h, frame, x = models
    rgb = dict(mean=[0.485, 0.456, 0.406, 0, 0, 0], std=[0.229, 0.224, 0.225, 1, 1, 1], to_rgb=[True, True], modalities_name=["rgb", "lidar"],
               modalities_ch=[3, 3], norm_by_max=True)
    r = Renderer(np.arange(3 * NUM_CLASSES).reshape(NUM_CLASSES, 3) % 256, opacity=0.5, preprocess=Preprocess(**rgb))
    want_w = inf.probabilities(m, h, x, dict(mode="whole")).max(1).values
    want_s = inf.probabilities(m, h, frame, SLIDE_CFG, max_batch=2).max(1).values
    cm0, pic0 = inf.whole_class_map(m, h, x, render=r)
    cm, pic, conf = inf.whole_class_map(m, h, x, render=r, confidence=True)
    assert torch.equal(cm, cm0) and torch.equal(pic, pic0) and torch.equal(conf, want_w)
    cm0, unc0, pic0 = inf.slide_class_map(m, h, frame, (256, 256), (170, 170), max_batch=2, render=r)
    cm, unc, pic, conf = inf.slide_class_map(m, h, frame, (256, 256), (170, 170), max_batch=2, render=r, confidence=True)
    assert torch.equal(cm, cm0) and torch.equal(pic, pic0) and torch.equal(conf, want_s)
    cm, pic, conf = inf.class_map(m, h, frame, SLIDE_CFG, render=r, confidence=True)
    assert torch.equal(cm, cm0) and torch.equal(pic, pic0) and torch.equal(conf, want_s)
    # labels= + evaluator=: the same counts as without the confidence map (which come from the fused launch or from the stored map)
    lp = LabelPrep(NUM_CLASSES)
    g = torch.Generator().manual_seed(4)
    lab_w = torch.randint(0, NUM_CLASSES, (2, 256, 256), generator=g, dtype=torch.uint8).to(DEV)
    lab_s = torch.randint(0, NUM_CLASSES, (1, 320, 400), generator=g, dtype=torch.uint8).to(DEV)
    lab_o = torch.randint(0, NUM_CLASSES, (2, 200, 310), generator=g, dtype=torch.uint8).to(DEV)
    for call, lab, want in ((lambda **kw: inf.whole_class_map(m, h, x, **kw), lab_w, want_w),
                            (lambda **kw: inf.slide_class_map(m, h, frame, (256, 256), (170, 170), max_batch=2, **kw), lab_s, want_s),
                            (lambda **kw: inf.whole_class_map(m, h, x, ori_shape=(200, 310), **kw), lab_o, None),
                            (lambda **kw: inf.aug_class_map(m, h, [x, x.flip(3)], dict(mode="whole"), ori_shape=(200, 310), flips=[None, "horizontal"], **kw), lab_o, None)):
        ev0, ev1 = Evaluator(lp, images=lab.shape[0], device=DEV), Evaluator(lp, images=lab.shape[0], device=DEV)
        r0 = call(labels=lab, evaluator=ev0)
        r1 = call(labels=lab, evaluator=ev1, confidence=True)
        cm0 = r0 if isinstance(r0, torch.Tensor) else r0[0]
        assert torch.equal(r1[0], cm0) and torch.equal(ev1.counts, ev0.counts) and int(ev1.counts.sum()) == lab.numel()
        assert want is None or torch.equal(r1[-1], want)
    # refusals, by name, before anything runs
    ev = Evaluator(lp, images=2, device=DEV)
    for kw in (dict(fused=True), dict(return_map=False)):
        with pytest.raises(RuntimeError, match="whole_class_map: confidence with fused=True / return_map=False"):
            inf.whole_class_map(m, h, x, labels=lab_w, evaluator=ev, confidence=True, **kw)
        with pytest.raises(RuntimeError, match="slide_class_map: confidence with fused=True / return_map=False"):
            inf.slide_class_map(m, h, frame, (256, 256), (170, 170), labels=lab_s, evaluator=ev, confidence=True, **kw)
    assert int(ev.counts.sum()) == 0
    with pytest.raises(RuntimeError, match="has shape"):
        inf.whole_class_map(m, h, x, confidence=torch.empty(2, 256, 255, device=DEV))
    with pytest.raises(RuntimeError, match="must be float32"):
        inf.class_map(m, h, x, dict(mode="whole"), confidence=torch.empty(2, 256, 256, device=DEV, dtype=torch.float16))
    with pytest.raises(RuntimeError, match="is on cpu"):
        inf.slide_class_map(m, h, frame, (256, 256), (170, 170), confidence=torch.empty(1, 320, 400))
    with pytest.raises(RuntimeError, match="must be contiguous"):
        inf.aug_class_map(m, h, [x], dict(mode="whole"), confidence=torch.empty(2, 256, 512, device=DEV)[:, :, ::2])


def test_conf_launches_replay_from_a_captured_graph(models):
    import mmsa.inference as inf
    cfg, m, h, frame, x = models
    # the three one-pass _conf launches in captured graphs replay to the same bits
    lg = h(m(x)[0]).contiguous()
    plans = [(inf.MapPlan.whole(2, 256, 256), lg, {}), (inf.MapPlan.whole(2, 256, 256, ori_shape=(200, 310)), lg, dict(one_pass=True)),
             (inf.AugPlan.of(dict(mode="whole"), [(2, 256, 256)] * 2, [None, "horizontal"], (200, 310)), [lg, h(m(x.flip(3))[0]).contiguous()], dict(one_pass=True))]
    for plan, lgs, kw in plans:
        want_map, want_conf, _ = _run(plan, lgs, **kw)
        out, conf, unc = torch.zeros_like(want_map), torch.zeros_like(want_conf), torch.zeros(1, dtype=torch.int32, device=DEV)
        plan.class_map(lgs, out, unc, conf=conf, **kw)      # a first call outside the capture (the augmented plan uploads its window table)
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            plan.class_map(lgs, out, unc, conf=conf, **kw)
        out.zero_()
        conf.zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, want_map) and torch.equal(conf, want_conf) and int(unc.item()) == 0, type(plan).__name__


@pytest.mark.parametrize("ori", [None, (300, 380, 3)])
def test_runner_keeps_a_static_confidence_buffer(models, ori):
    import mmsa.inference as inf
    cfg, m, h, frame, x = models
    cm, _, want = inf.slide_class_map(m, h, frame, (256, 256), (170, 170), max_batch=2, ori_shape=ori, confidence=True)
    sr = inf.SlideRunner(m, h, frame, (256, 256), (170, 170), chains=2, ori_shape=ori, confidence=True)
    assert sr.conf.shape == want.shape and sr.conf.dtype == torch.float32
    for _ in range(2):
        res = sr.run()
        conf = res.confidence()
        torch.cuda.synchronize()
        assert conf is sr.conf and torch.equal(conf, want) and torch.equal(res.outputs()[0], cm)
    for kw in (dict(fused=True), dict(return_map=False)):
        with pytest.raises(RuntimeError, match="SlideRunner.run: confidence with fused=True"):
            sr.run(**kw)


# ---- 7. against the reference's own outputs

def _toy():
    w = torch.randn(RR.NUM_CLASSES, 6, 1, 1, generator=torch.Generator().manual_seed(RR.TOY_SEED)).to(DEV)
    return (lambda im: ([F.avg_pool2d(im, 4)], None)), (lambda feats: F.conv2d(feats[0], w).contiguous())


@pytest.mark.parametrize("tag", sorted(AR.CASES))
def test_against_the_reference_aug_fixture(golden_dir, tag):
    """conf against the maximum over the classes of the reference's own averaged probabilities.  Case `slide` (3 x 3 windows on some pixels) is refused by
    aug_class_map as it is without confidence; its confidence comes from argmax_max_map(aug_inference(...))."""
    import mmsa.inference as inf
    g = np.load(os.path.join(golden_dir, "aug.npz"))
    case = AR.case_of(g[f"{tag}_cfg"])
    hw, crop, stride, ori, _ = case
    imgs, flips = AR.views_of(case)
    imgs = [v.to(DEV) for v in imgs]
    want = torch.from_numpy(g[f"{tag}_prob"]).max(1).values
    bb, hd = _toy()
    tc = dict(mode="whole") if crop is None else dict(mode="slide", crop_size=crop, stride=stride)
    if tag == "slide":
        with pytest.raises(RuntimeError, match="covers some pixels 9 times"):
            inf.aug_class_map(bb, hd, imgs, tc, ori_shape=ori, flips=flips, confidence=True)
        _, conf = inf.argmax_max_map(inf.aug_inference(bb, hd, imgs, tc, ori_shape=ori, flips=flips))
    else:
        for one_pass in (None, True):
            _, unc, conf = inf.aug_class_map(bb, hd, imgs, tc, ori_shape=ori, flips=flips, confidence=True, one_pass=one_pass)
            assert int(unc.item()) == 0
            assert_close(conf, want, what=f"confidence, case {tag}, one_pass={one_pass}")
    r, mx = assert_close(conf, want, what=f"confidence, case {tag}")
    print(f"aug {tag}: confidence rel_l2 {r:.2e} max_rel {mx:.2e}")


@pytest.mark.parametrize("tag", ["a", "c", "w"])
def test_against_the_reference_rescale_fixture(golden_dir, tag):
    import mmsa.inference as inf
    g = np.load(os.path.join(golden_dir, "rescale.npz"))
    hw, crop, stride, ori = RR.case_of(g[f"{tag}_cfg"])
    want = torch.softmax(torch.from_numpy(g[f"{tag}_out"]).double(), 1).max(1).values
    bb, hd = _toy()
    img = RR.frame(hw).to(DEV)
    for one_pass in (None, False):
        if crop is None:
            _, conf = inf.whole_class_map(bb, hd, img, ori_shape=ori, confidence=True, one_pass=one_pass)
        else:
            _, unc, conf = inf.slide_class_map(bb, hd, img, crop, stride, ori_shape=ori, confidence=True, one_pass=one_pass)
            assert int(unc.item()) == 0
        r, mx = assert_close(conf, want, what=f"confidence, case {tag}, one_pass={one_pass}")
        print(f"rescale {tag} one_pass={one_pass}: confidence rel_l2 {r:.2e} max_rel {mx:.2e}")
