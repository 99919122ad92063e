"""Top-k maps on the device: the first K classes of every pixel and their probabilities (csrc/softmax_px.h, TopkPx) written rank-major by the launch that
writes the class map -- mmsa_slide_argmax_topk against the canvas launch (mmsa_argmax_topk_nchw on the canvas path's probabilities) bit for bit, the three
identities (plane 0 of the classes is the map, plane 0 of the probabilities the confidence, probs[0] - probs[1] the margin), the exact cases, uncovered pixels,
the rescaled / cut size, a temperature, augmented views, the float64 order of the same float32 logits within the bound DESIGN.md section 2 derives for one
softmax element, the evaluation pass (mmsa_eval_topk_u8) against a numpy restatement, and the public entries of mmsa.inference on the tiny model."""
import dataclasses

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import confidence_ref as CR
from tests import topk_ref as TR
from tests.configs import CONFIGS, HEAD_CONFIGS, make_input
from tests.test_aug_gpu import GEOMETRIES
from tests.weights import seeded_state_dict

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
RESCALES = [((77, 131), None), ((135, 201), None), ((135, 201), (60, 100))]      # down, up, a cut of the latter: those of tests/test_uncertainty_gpu.py
KS = (1, 2, 3, 4, 5, 8)                                                           # every slot-count bucket (2 / 4 / 8) and its edge


def _plan(geo, B=2, tgt=None, cut=None):
    import mmsa.inference as inf
    (H, W), stride = GEOMETRIES[geo]
    p = inf.MapPlan.slide(B, H, W, (64, 64), stride, tgt)
    return p if cut is None else dataclasses.replace(p, Ho=cut[0], Wo=cut[1])


def _buffers(K, size):
    """A TopK pre-filled with values no launch writes."""
    import mmsa.inference as inf
    return inf.TopK(torch.full((K,) + tuple(size), 77, dtype=torch.uint8, device=DEV), torch.full((K,) + tuple(size), -1.0, device=DEV))


def _run(plan, lg, K, **kw):
    """plan.class_map with a TopK of buffers -> (classes, probs, uncovered count)."""
    tk = _buffers(K, plan.size if hasattr(plan, "size") else (plan.B, plan.Ho, plan.Wo))
    unc = torch.zeros(1, dtype=torch.int32, device=DEV)
    plan.class_map(lg, tk.classes[0], unc, topk=tk, **kw)
    return tk.classes, tk.probs, int(unc.item())


def _other(plan, lg, **kw):
    """plan.class_map without topk= -> (map, confidence or score or None, uncovered count)."""
    size = plan.size if hasattr(plan, "size") else (plan.B, plan.Ho, plan.Wo)
    out = torch.full(size, 77, dtype=torch.uint8, device=DEV)
    conf = torch.full(size, -1.0, device=DEV) if kw.pop("conf", False) else None
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


def _same(a, b):
    return torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


def _structure(classes, probs, C):
    """Probabilities non-increasing over the ranks; the classes of a pixel below rank min(K, C) distinct and < C; ranks >= C are 255 / 0."""
    K = classes.shape[0]
    n = min(K, C)
    assert bool((probs[:-1] >= probs[1:]).all()) and bool((probs >= 0).all()) and bool((probs <= 1).all())
    assert bool((classes[:n] < C).all()) and bool((classes[n:] == 255).all()) and bool((probs[n:] == 0).all())
    srt = classes[:n].long().sort(0).values
    assert n < 2 or bool((srt[1:] != srt[:-1]).all()), "a class is ranked twice"


# ---- 1, 2, 3, 8. the frame's size, one view

@pytest.mark.parametrize("geo", sorted(GEOMETRIES))
@pytest.mark.parametrize("C", [1, 2, 5, 33])
def test_frame_size_equals_the_canvas_launch_the_identities_and_float64(C, geo):
    _frame_size_case(C, geo)


@pytest.mark.parametrize("geo", ["s40", "s24"])
@pytest.mark.parametrize("C", [64, 65])
def test_frame_size_on_both_sides_of_the_lds_limit(C, geo):
    """mmsa_slide_argmax_topk keeps the pixel's values in LDS up to 64 classes (exactly 64 KiB at 64) and recomputes them in two more passes from 65 on."""
    _frame_size_case(C, geo)


def _frame_size_case(C, geo):
    import mmsa
    plan = _plan(geo)
    lg = CR.planted_logits(plan.n, C, 1000 + C).to(DEV)
    plain, _, unc0 = _other(plan, lg)                                  # mmsa_slide_argmax
    _, conf, _ = _other(plan, lg, conf=True)                           # the confidence=True launch
    margin = _other(plan, lg, conf=True, score="margin")[1]            # the score="margin" launch
    y, want, prob, unc2 = _canvas(plan, lg)
    P, D = TR.float64_probabilities(y)
    eps = TR.eps_of(D, C)
    assert unc0 == 0 and unc2 == 0 and torch.equal(plain, want)
    assert (30 <= float(D.max()) or C == 1) and float(D.max()) < 87
    for K in KS:
        classes, probs, unc = _run(plan, lg, K)
        canvas = mmsa.argmax_topk_map(prob, K, first=want)
        diff = int((classes != canvas.classes).sum().item()) + int((probs != canvas.probs).sum().item())
        worst, bad, wrong, und = TR.float64_check(classes, probs, P, eps, K)
        print(f"{geo} C={C} K={K}: {diff} values differ from the canvas launch; D up to {float(D.max()):.1f}, worst error / float64 bound {worst:.3f}, "
              f"{bad} order violations, {wrong} decided pixels out of order, undecided share {und:.5f}")
        assert unc == 0 and _same((classes, probs), canvas), f"{geo} C={C} K={K}: the one-pass planes are not the canvas launch's, bit for bit"
        # the three identities
        assert torch.equal(classes[0], plain), "classes[0] is the class map"
        assert torch.equal(probs[0], conf), "probs[0] is the confidence=True map"
        if C >= 2 and K >= 2:
            assert torch.equal(probs[0] - probs[1], margin), "probs[0] - probs[1] is the score='margin' map"
        _structure(classes, probs, C)
        # float64 of the same float32 logits: (a) the values, (b) a valid order, (c) the exact order where it is decided
        assert worst <= 1.0 and bad == 0 and wrong == 0 and und <= 0.01
    if C == 1:
        return
    # the exact cases
    same = lg[:, :1].expand(-1, C, -1, -1).contiguous()
    ahead = lg.clone()
    ahead[:, C // 2] += 300.0
    tie = lg.clone()
    tie[:, 0] = lg.max(1).values + 2.0
    tie[:, C - 1] = tie[:, 0]
    others = [c for c in range(C) if c != C // 2]
    for K in (2, 8):
        n = min(K, C)
        classes, probs, _ = _run(plan, same, K)                        # every class the same plane: classes 0, 1, ... and all probabilities equal
        assert all(bool((classes[r] == (r if r < C else 255)).all()) for r in range(K))
        assert all(torch.equal(probs[r], probs[0]) for r in range(n)) and bool((probs[n:] == 0).all())
        classes, probs, _ = _run(plan, ahead, K)                       # one class ahead by 300: every other exponential is 0.0f
        assert bool((classes[0] == C // 2).all()) and bool((probs[0] == 1).all()) and bool((probs[1:] == 0).all())
        assert all(bool((classes[r] == (others[r - 1] if r < C else 255)).all()) for r in range(1, K)), "the runners-up at probability 0, in class order"
        classes, probs, _ = _run(plan, tie, K)                         # classes 0 and C - 1 tied at the top
        assert bool((classes[0] == 0).all()) and bool((classes[1] == C - 1).all()) and torch.equal(probs[0], probs[1])


def test_the_canvas_launch_alone():
    """mmsa.argmax_topk_map against the restatement on probabilities with planted ties, with and without first=, and in place over plane 0."""
    import mmsa
    import mmsa.inference as inf
    g = torch.Generator().manual_seed(5)
    for C, K in ((1, 2), (2, 3), (5, 4), (5, 8), (33, 5)):
        q = (torch.randint(0, 3, (2, C, 37, 61), generator=g).float() + 1.0) / 8.0
        first = torch.randint(0, C, (2, 37, 61), generator=g)
        first[1, :3] = 255
        got = mmsa.argmax_topk_map(q.to(DEV), K)
        assert _same((got.classes.cpu(), got.probs.cpu()), TR.topk(q, TR.UR.first_argmax(q), K)), (C, K)
        want = TR.topk(q, first, K)
        got = mmsa.argmax_topk_map(q.to(DEV), K, first=first.to(torch.uint8).to(DEV))
        assert _same((got.classes.cpu(), got.probs.cpu()), want) and bool((got.classes[:, 1, :3] == 255).all()) and bool((got.probs[:, 1, :3] == 0).all())
        tk = _buffers(K, (2, 37, 61))
        tk.classes[0].copy_(first.to(torch.uint8))
        inf._argmax_topk_into(q.to(DEV), tk.classes[0], tk)            # first = plane 0 itself: a lane reads its byte before it writes
        assert _same((tk.classes.cpu(), tk.probs.cpu()), want)


# ---- 4. uncovered pixels

def test_uncovered_pixels_are_255_and_0_at_every_rank_and_counted_once():
    """The strip of tests/test_uncertainty_gpu.py: two windows leave columns 64 .. 87 of a 64 x 88 frame uncovered."""
    import mmsa
    import mmsa.inference as inf
    flat = inf.MapPlan(2, 64, 88, 64, 64, ((0, 0, 0), (1, 0, 0)), 64, 88, 64, 88)
    lg = torch.randn(2, 5, 16, 16, generator=torch.Generator().manual_seed(3)).to(DEV)
    plain, _, unc0 = _other(flat, lg)
    _, want, prob, _ = _canvas(flat, lg)
    for K in (1, 3, 8):
        classes, probs, unc = _run(flat, lg, K)
        assert unc == unc0 == 2 * 64 * 24 and bool((classes[:, :, :, 64:] == 255).all()) and bool((probs[:, :, :, 64:] == 0).all())
        assert torch.equal(classes[0], plain)
        canvas = mmsa.argmax_topk_map(prob, K, first=plain)            # the stored map carries the 255s to the canvas launch
        assert _same((classes, probs), canvas)
        _structure(classes[:, :, :, :64], probs[:, :, :, :64], 5)


# ---- 5. the rescaled / cut size

@pytest.mark.parametrize("geo", sorted(GEOMETRIES))
@pytest.mark.parametrize("C", [5, 33])
def test_rescaled_size_is_the_canvas_launch_on_the_stored_map(C, geo):
    import mmsa
    for tgt, cut in RESCALES:
        plan = _plan(geo, 2, tgt, cut)
        lg = CR.planted_logits(plan.n, C, 2000 + C).to(DEV)
        y, want, prob, unc2 = _canvas(plan, lg)
        maps = [_other(plan, lg, one_pass=op)[0] for op in (True, False)]
        P, D = TR.float64_probabilities(y)
        for K in (1, 3, 8):
            for op in (None, False):
                classes, probs, unc = _run(plan, lg, K, one_pass=op)
                assert unc == 0 and unc2 == 0 and classes.shape == (K, 2) + (cut or tgt)
                assert _same((classes, probs), mmsa.argmax_topk_map(prob, K, first=want)), f"{geo} C={C} K={K} target {tgt} cut {cut} one_pass={op}"
                assert torch.equal(classes[0], maps[0]) and torch.equal(classes[0], maps[1]), "the plain rescaled map of both launches"
            _structure(classes, probs, C)
            worst, bad, wrong, und = TR.float64_check(classes, probs, P, TR.eps_of(D, C), K)
            assert worst <= 1.0 and bad == 0 and wrong == 0 and und <= 0.01 and float(D.max()) < 87
            with pytest.raises(RuntimeError, match="topk= with one_pass=True: there is no one-pass top-k launch at a rescaled or cut size"):
                _run(plan, lg, K, one_pass=True)


# ---- 6. with a temperature

@pytest.mark.parametrize("C", [5, 33, 65])
def test_temperature_combines_with_topk(C):
    import mmsa
    from mmsa.evaluate import inv_temperature
    for tgt in (None, (77, 131)):
        plan = _plan("s40", 2, tgt)
        lg = CR.planted_logits(plan.n, C, 3000 + C).to(DEV)
        it = inv_temperature(2.5)
        y, want, prob, _ = _canvas(plan, lg, it=it)                    # mmsa_softmax_flip_accum_nchw_t
        P, DT = TR.float64_probabilities(y, it)
        for K in (2, 4, 8):
            assert _same(_run(plan, lg, K, temperature=1.0)[:2], _run(plan, lg, K)[:2]), f"C={C} K={K} target {tgt}: T = 1 is the untempered result"
            classes, probs, unc = _run(plan, lg, K, temperature=2.5)
            assert unc == 0 and _same((classes, probs), mmsa.argmax_topk_map(prob, K, first=want)), f"C={C} K={K} T=2.5 target {tgt}"
            assert torch.equal(classes[0], _run(plan, lg, K)[0][0]) and not torch.equal(probs, _run(plan, lg, K)[1])
            worst, bad, wrong, und = TR.float64_check(classes, probs, P, TR.eps_of(DT, C, tempered=True), K)
            print(f"C={C} K={K} T=2.5 target {tgt}: D_T up to {float(DT.max()):.1f}, worst error / tempered bound {worst:.3f}, undecided share {und:.5f}")
            assert worst <= 1.0 and bad == 0 and wrong == 0 and und <= 0.01 and float(DT.max()) < 87


# ---- 7. augmented views

def _aug_plan(tgt, cut, views):
    import mmsa.inference as inf
    geos, flips = (("s40", "s64", "s24", "s40"), (0, 1, 2, 1)) if views == 4 else (("s40", "s24"), (0, 1))
    return inf.AugPlan(tuple(_plan(g, 2, tgt, cut) for g in geos), flips)


@pytest.mark.parametrize("views", [2, 4])
@pytest.mark.parametrize("C", [5, 33])
def test_augmented_is_the_canvas_launch_on_the_mean_probabilities(C, views):
    """Flips [-, h] / [-, h, v, h]: the top-k of the MEAN probabilities, rank 0 their first maximum, by the canvas path whatever the default.  Float64: the
    mean of the views' float64 softmaxes; a view's element is within (2 D_a + C + 4) 2^-23 (tests/test_aug_gpu.py), the sum of positive terms within the
    largest of those, and the A - 1 additions and the division add 2^-24 each: eps = max_a eps_a + A 2^-24."""
    import mmsa
    import mmsa.inference as inf
    for tgt, cut in RESCALES[1:]:
        plan = _aug_plan(tgt, cut, views)
        g = torch.Generator().manual_seed(200 + C)
        lgs = [torch.randn(p.n, C, 16, 16, generator=g).to(DEV) * 3.0 for p in plan.plans]
        prob = plan.mean_probabilities(lgs, torch.zeros(1, dtype=torch.int32, device=DEV))
        plain = _other(plan, lgs)[0]
        P, eps = 0.0, 0.0
        for p, f, lg in zip(plan.plans, plan.flips, lgs):
            Pa, Da = TR.float64_probabilities(_canvas(p, lg)[0])
            dims = {0: (), 1: (3,), 2: (2,)}[f]
            P = P + (Pa.flip(*dims) if dims else Pa)
            eps = torch.maximum(torch.as_tensor(eps, dtype=torch.float64), TR.eps_of(Da.flip(*[d - 1 for d in dims]) if dims else Da, C))
        P, eps = P / plan.A, eps + plan.A * 2.0 ** -24
        for K in (2, 3, 8):
            want = mmsa.argmax_topk_map(prob, K)
            for op in (None, False):
                classes, probs, unc = _run(plan, lgs, K, one_pass=op)
                assert unc == 0 and _same((classes, probs), want), f"C={C} K={K} views={views} target {tgt} cut {cut} one_pass={op}"
            assert torch.equal(classes[0], plain) and torch.equal(classes[0], inf.argmax_map(prob)) and torch.equal(probs[0], prob.max(1).values)
            _structure(classes, probs, C)
            worst, bad, wrong, und = TR.float64_check(classes, probs, P, eps, K)
            print(f"aug C={C} K={K} views={views}: worst error / bound {worst:.3f}, {bad} order violations, undecided share {und:.5f}")
            assert worst <= 1.0 and bad == 0 and wrong == 0 and und <= 0.01
            with pytest.raises(RuntimeError, match="topk= with one_pass=True"):
                _run(plan, lgs, K, one_pass=True)


# ---- 9. the evaluation pass

def _planes(K, C, B, H, W, g):
    """Class planes as a top-k launch writes them: K distinct classes per pixel, 255 from a pixel's own rank on for some, 255 everywhere for a few."""
    cls = torch.rand(B, H, W, C, generator=g).argsort(-1)[..., :K].permute(3, 0, 1, 2).contiguous()
    if K > C:
        cls = torch.cat([cls, torch.full((K - C, B, H, W), 255)], 0)
    stop = torch.randint(1, 3 * K, (B, H, W), generator=g)
    cls = torch.where(torch.arange(K).view(K, 1, 1, 1) >= stop, torch.full_like(cls, 255), cls)
    cls[:, torch.rand(B, H, W, generator=g) < 0.03] = 255
    return cls.to(torch.uint8)


@pytest.mark.parametrize("W", [61, 62, 63, 64])
def test_rank_counts_equal_the_numpy_restatement(W):
    """Odd sizes and every start alignment of a row; reduce_zero_label, ignored labels, a label_map, resized labels through the tables, 255 bytes in the
    planes, slots that repeat; the ties to mmsa.confusion; the same bytes run after run."""
    import mmsa
    from mmsa.evaluate import Evaluator, LabelPrep, TopKEvaluator, nearest_axis_table
    g = torch.Generator().manual_seed(W)
    B, H, C = 3, 151, 7                                                 # 151 * W > 8192: more than one workgroup per image
    for K, kw in ((1, {}), (3, dict(reduce_zero_label=True)), (4, dict(ignore_index=3)), (8, dict(label_map={0: 2, 5: 200})), (2, dict(resize=(97, 45)))):
        cls = _planes(K, C, B, H, W, g)
        rs = kw.pop("resize", None)
        Hl, Wl = rs or (H, W)
        lab = torch.randint(0, C + 2, (B, Hl, Wl), generator=g, dtype=torch.uint8)
        lab[torch.rand(B, Hl, Wl, generator=g) < 0.05] = 255
        lp = LabelPrep(C, resize=None if rs is None else dict(seg_scale=(W, H), keep_ratio=False), **kw)
        tabs = (None, None) if rs is None else (nearest_axis_table(Hl, H), nearest_axis_table(Wl, W))
        d_cls, d_lab = cls.to(DEV), lab.to(DEV)
        for slots in (None, [1, 0, 1]):
            want = TR.rank_counts(cls.numpy(), lab.numpy(), lp.lut, C, *tabs, slots=slots)
            got = mmsa.topk_counts(d_cls, d_lab, lp, slots=slots)
            again = mmsa.topk_counts(d_cls, d_lab, lp, slots=slots)
            assert got.shape == want.shape and got.dtype == torch.int64
            assert got.cpu().numpy().tobytes() == want.tobytes(), (W, K, kw, slots)
            assert again.cpu().numpy().tobytes() == got.cpu().numpy().tobytes(), "two runs, the same bytes"
            mmsa.topk_counts(d_cls, d_lab, lp, counts=got, slots=slots)                       # ADDED to
            assert got.cpu().numpy().tobytes() == (2 * want).tobytes()
        per = mmsa.topk_counts(d_cls, d_lab, lp).cpu().numpy()
        conf = [mmsa.confusion(d_cls[r], d_lab, lp).cpu().numpy() for r in range(K)]
        for r in range(K):
            assert np.array_equal(per[:, :, r], np.diagonal(conf[r], axis1=1, axis2=2)[:, :C]), f"column {r} is the diagonal of plane {r}'s confusion matrix"
        assert np.array_equal(per.sum(2), conf[0].sum(2)[:, :C]), "row sums are those of plane 0's confusion matrix"
        te, ev = TopKEvaluator(lp, K, images=B, device=DEV), Evaluator(lp, images=B, device=DEV)
        te.add(d_cls, d_lab)
        ev.add(d_cls[0], d_lab)
        acc = te.accuracy()
        assert te.host_counts().tobytes() == per.tobytes() and acc[0] == ev.metrics()["aAcc"] and bool((np.diff(acc) >= 0).all()) and acc.shape == (K,)
        assert te.recall().shape == (C, K) and list(te.summary())[:K] == [f"top{j + 1}" for j in range(K)]


# ---- 10. the public entries on the tiny model

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


def _is(tk, classes, probs):
    return torch.equal(tk.classes, classes) and torch.equal(tk.probs, probs)


@pytest.mark.parametrize("K", [2, 5])
def test_slide_and_whole_entries(models, K):
    import mmsa
    import mmsa.inference as inf
    cfg, m, h, frame, x = models
    cut = inf._intake(frame, None, "slide_class_map")[5]
    for ori in (None, (300, 380, 3)):
        plan = inf.MapPlan.slide(1, 320, 400, (256, 256), (170, 170), ori)
        lg = inf._window_logits(m, h, cut, plan.windows, 2)
        want = _run(plan, lg, K)                                       # the plan-level launch on the same logits
        plain = inf.slide_class_map(m, h, frame, (256, 256), (170, 170), max_batch=2, ori_shape=ori)
        conf = inf.slide_class_map(m, h, frame, (256, 256), (170, 170), max_batch=2, ori_shape=ori, confidence=True)[2]
        for given in (K, _buffers(K, plain[0].shape)):
            cm, unc, tk = inf.slide_class_map(m, h, frame, (256, 256), (170, 170), max_batch=2, ori_shape=ori, topk=given)
            assert int(unc.item()) == 0 and torch.equal(cm, plain[0]) and _is(tk, *want[:2]) and torch.equal(tk.probs[0], conf), f"slide ori_shape={ori}"
            assert cm.data_ptr() == tk.classes.data_ptr() and (given is K or tk is given), "the map is plane 0 itself; caller buffers are written in place"
        wt = mmsa.argmax_topk_map(inf.probabilities(m, h, frame, SLIDE_CFG, ori_shape=ori, max_batch=2, temperature=2.5), K, first=plain[0])
        tk = inf.slide_class_map(m, h, frame, (256, 256), (170, 170), max_batch=2, ori_shape=ori, topk=K, temperature=2.5)[2]
        assert _is(tk, *wt) and not torch.equal(tk.probs, want[1])
        if ori is not None:
            with pytest.raises(RuntimeError, match="topk= with one_pass=True"):
                inf.slide_class_map(m, h, frame, (256, 256), (170, 170), max_batch=2, ori_shape=ori, topk=K, one_pass=True)
    lg = h(m(x)[0]).contiguous()
    for kw in (dict(ori_shape=(200, 310)), dict(dim=(192, 240)), dict(dim=(200, 300), cut_dim=(260, 150)), {}):
        want = _run(inf.MapPlan.whole(2, 256, 256, **kw), lg, K)
        plain = inf.whole_class_map(m, h, x, **kw)
        for given in (K, _buffers(K, plain.shape)):
            cm, tk = inf.whole_class_map(m, h, x, topk=given, **kw)
            assert torch.equal(cm, plain) and _is(tk, *want[:2]) and cm.data_ptr() == tk.classes.data_ptr() and (given is K or tk is given), f"whole {kw}"
    for kw in (dict(fused=True), dict(return_map=False)):
        with pytest.raises(RuntimeError, match="whole_class_map: topk= with fused=True / return_map=False"):
            inf.whole_class_map(m, h, x, topk=K, **kw)
        with pytest.raises(RuntimeError, match="slide_class_map: topk= with fused=True / return_map=False"):
            inf.slide_class_map(m, h, frame, (256, 256), (170, 170), topk=K, **kw)
    with pytest.raises(RuntimeError, match="whole_class_map: topk= with confidence="):
        inf.whole_class_map(m, h, x, topk=K, confidence=True)
    with pytest.raises(RuntimeError, match="whole_class_map: the top-k classes buffer has shape"):
        inf.whole_class_map(m, h, x, topk=_buffers(K, (2, 256, 255)))


@pytest.mark.parametrize("K", [3])
def test_class_map_modes_and_aug_entry(models, K):
    import mmsa
    import mmsa.inference as inf
    from mmsa.evaluate import LabelPrep, TopKEvaluator
    cfg, m, h, frame, x = models
    cfgs = [SLIDE_CFG, dict(mode="whole"), dict(mode="whole_dim", dim=(300, 280)), dict(mode="whole_dim_cut", dim=(300, 280), cut_dim=(250, 270))]
    for tc in cfgs:
        img = frame if tc["mode"] == "slide" else x
        plain = inf.class_map(m, h, img, tc, ori_shape=(210, 333, 3))
        want = mmsa.argmax_topk_map(inf.probabilities(m, h, img, tc, ori_shape=(210, 333, 3)), K, first=plain)
        for given in (K, _buffers(K, plain.shape)):
            cm, tk = inf.class_map(m, h, img, tc, ori_shape=(210, 333, 3), topk=given)
            assert torch.equal(cm, plain) and _is(tk, *want) and cm.data_ptr() == tk.classes.data_ptr() and (given is K or tk is given), f"class_map {tc}"
    big = F.interpolate(frame, (400, 500), mode="bilinear", align_corners=False)
    imgs, flips, ori = [frame, frame.flip(3), big, big.flip(3)], [None, "horizontal", None, "horizontal"], (300, 380, 3)
    want = mmsa.argmax_topk_map(inf.aug_inference(m, h, imgs, SLIDE_CFG, ori_shape=ori, flips=flips, max_batch=4), K)
    plain = inf.aug_class_map(m, h, imgs, SLIDE_CFG, ori_shape=ori, flips=flips, max_batch=4)
    lp = LabelPrep(NUM_CLASSES)
    lab = torch.randint(0, NUM_CLASSES, (1, 300, 380), generator=torch.Generator().manual_seed(4), dtype=torch.uint8).to(DEV)
    for given in (K, _buffers(K, plain[0].shape)):
        te = TopKEvaluator(lp, K, images=1, device=DEV)
        cm, unc, tk = inf.aug_class_map(m, h, imgs, SLIDE_CFG, ori_shape=ori, flips=flips, max_batch=4, topk=given, labels=lab, topk_evaluator=te)
        assert int(unc.item()) == 0 and torch.equal(cm, plain[0]) and _is(tk, *want) and (given is K or tk is given)
        assert te.counts.cpu().numpy().tobytes() == mmsa.topk_counts(tk.classes, lab, lp).cpu().numpy().tobytes() and int(te.counts.sum()) == lab.numel()
    with pytest.raises(RuntimeError, match="aug_class_map: topk= with one_pass=True"):
        inf.aug_class_map(m, h, imgs, SLIDE_CFG, ori_shape=ori, flips=flips, max_batch=4, one_pass=True, topk=K)


def test_runner_keeps_static_topk_buffers(models):
    import mmsa
    import mmsa.inference as inf
    from mmsa.evaluate import Evaluator, LabelPrep, TopKEvaluator
    cfg, m, h, frame, x = models
    K = 4
    lp = LabelPrep(NUM_CLASSES)
    for ori in (None, (300, 380, 3)):
        cm, _, want = inf.slide_class_map(m, h, frame, (256, 256), (170, 170), max_batch=2, ori_shape=ori, topk=K)
        lab = torch.randint(0, NUM_CLASSES, (1,) + tuple(cm.shape[1:]), generator=torch.Generator().manual_seed(6), dtype=torch.uint8).to(DEV)
        sr = inf.SlideRunner(m, h, frame, (256, 256), (170, 170), chains=2, ori_shape=ori, topk=K)
        te, ev = TopKEvaluator(lp, K, cases=["all"], device=DEV), Evaluator(lp, cases=["all"], device=DEV)
        assert sr.topk.classes.shape == want.classes.shape and sr.out.data_ptr() == sr.topk.classes.data_ptr()
        for _ in range(2):                                              # two frames
            res = sr.run(labels=lab, evaluator=ev, topk_evaluator=te, case="all")
            tk = res.topk()
            torch.cuda.synchronize()
            assert tk is sr.topk and _is(tk, *want) and torch.equal(res.outputs()[0], cm)
        one = mmsa.topk_counts(want.classes, lab, lp, slots=[0]).cpu().numpy()
        assert te.host_counts().tobytes() == (2 * one).tobytes() and te.accuracy()[0] == ev.metrics()["aAcc"]
        with pytest.raises(RuntimeError, match="SlideRunner.run: topk= with fused=True"):
            sr.run(fused=True)
        with pytest.raises(RuntimeError, match="SlideRunner.run: topk_evaluator= needs labels="):
            sr.run(topk_evaluator=te)
    plain = inf.SlideRunner(m, h, frame, (256, 256), (170, 170), chains=2)
    with pytest.raises(RuntimeError, match="FrameResult.topk: the SlideRunner was made without topk="):
        plain.run().topk()
    with pytest.raises(RuntimeError, match="SlideRunner.run: topk_evaluator= needs the top-k map"):
        plain.run(labels=lab, topk_evaluator=te)


def test_topk_launches_replay_from_a_captured_graph(models):
    import mmsa.inference as inf
    cfg, m, h, frame, x = models
    lg = h(m(x)[0]).contiguous()
    plan = inf.MapPlan.whole(2, 256, 256)
    want = _run(plan, lg, 3)
    tk, unc = _buffers(3, (2, 256, 256)), torch.zeros(1, dtype=torch.int32, device=DEV)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        plan.class_map(lg, tk.classes[0], unc, topk=tk)
    tk.classes.zero_()
    tk.probs.zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert _is(tk, *want[:2]) and int(unc.item()) == 0
