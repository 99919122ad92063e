"""Test-time augmentation on the device (aug_test, ED:509-546): the softmax / un-flip / accumulate kernel against float64 and against itself, the
one-pass class map mmsa_aug_argmax against the canvas path bit for bit (all three workgroup sizes, exact ties, uncovered pixels), the public entries of
mmsa.inference on the tiny model, and both against the reference's own aug_test (tests/golden/aug.npz)."""
import ctypes
import dataclasses
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import aug_ref as AR
from tests import rescale_ref as RR
from tests.configs import CONFIGS, HEAD_CONFIGS, make_input
from tests.util import REL_TOL, assert_close
from tests.weights import seeded_state_dict

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

GEOMETRIES = dict(s40=((90, 150), (40, 40)), s64=((70, 70), (64, 64)), s24=((90, 150), (32, 24)))      # those of tests/test_rescale_class_map_gpu.py


def _softmax(x, flip=0, acc=None, accumulate=False, finish_div=0):
    from mmsa import lib, ops
    B, C, H, W = x.shape
    if acc is None:
        acc = torch.full_like(x, float("nan"))
    lib.call("mmsa_softmax_flip_accum_nchw", x.data_ptr(), acc.data_ptr(), B, C, H, W, flip, 1 if accumulate else 0, finish_div, ops._stream())
    return acc


# ---- the softmax kernel

@pytest.mark.parametrize("hw", [(7, 13), (64, 300)])
@pytest.mark.parametrize("C", [1, 5, 33])
def test_softmax_against_float64_flips_and_accumulation(C, hw):
    """Relative error per element against the float64 softmax of the same float32 logits <= (2 D + C + 4) 2^-23, D = the pixel's max |x - m|: the derived
    bound is half of it -- one rounding of x - m, which enters the exponent (D 2^-24, numerator and denominator), expf within 1 ulp (2 x 2 x 2^-24), C - 1
    additions of positive terms, one division -- and the factor 2 is margin for the quoted, not measured, 1 ulp of expf."""
    g = torch.Generator().manual_seed(1000 + C)
    x = torch.randn(2, C, hw[0], hw[1], generator=g) * 6.0
    if C > 1:
        x[0, 0, 3, 5], x[0, 1, 3, 5] = 15.0, -15.0                   # D reaches 30 whatever the noise does
    xd = x.to(DEV)
    p0 = _softmax(xd)
    want = torch.softmax(x.double(), dim=1)
    D = (x.double() - x.double().max(1, keepdim=True).values).abs().max(1, keepdim=True).values
    bound = (2 * D + C + 4) * 2.0 ** -23
    rel = (p0.cpu().double() - want).abs() / want
    print(f"softmax C={C} {hw}: D up to {D.max().item():.1f}, smallest p {want.min().item():.1e}, worst error / bound {(rel / bound).max().item():.3f}")
    assert D.max() >= 30 or C == 1
    assert torch.isfinite(p0).all() and bool((rel <= bound).all())
    # flipped back: the same values at the mirrored positions, bit for bit
    p1, p2 = _softmax(xd, 1), _softmax(xd, 2)
    assert torch.equal(p1, p0.flip(3)) and torch.equal(p2, p0.flip(2))
    # three views accumulated in view order, divided with the last: ((p0 + p1) + p2) / 3 of the kernel's own single-view outputs
    acc = _softmax(xd)
    _softmax(xd, 1, acc, accumulate=True)
    _softmax(xd, 2, acc, accumulate=True, finish_div=3)
    assert torch.equal(acc, ((p0 + p1) + p2) / torch.full_like(p0, 3.0))       # a tensor divisor: a true division, not a multiplication by 1 / 3
    with pytest.raises(RuntimeError, match="flip is 0"):
        _softmax(xd, 3)


# ---- one pass against the canvas path

def _view_plan(geo, B, tgt, cut=None):
    import mmsa.inference as inf
    (H, W), stride = GEOMETRIES[geo]
    p = inf.MapPlan.slide(B, H, W, (64, 64), stride, tgt)
    return p if cut is None else dataclasses.replace(p, Ho=cut[0], Wo=cut[1])


def _both_paths(plan, lgs):
    """-> (one-pass map, its uncovered count, canvas-path map, averaged probabilities of the canvas path, canvas pixels without a window)"""
    import mmsa.inference as inf
    B, Ho, Wo = plan.size
    got = torch.full((B, Ho, Wo), 77, dtype=torch.uint8, device=DEV)
    unc, unc2 = torch.zeros(1, dtype=torch.int32, device=DEV), torch.zeros(1, dtype=torch.int32, device=DEV)
    plan.class_map(lgs, got, unc, one_pass=True)
    prob = plan.mean_probabilities(lgs, unc2)
    return got, int(unc.item()), inf.argmax_map(prob), prob, int(unc2.item())


def _logits(plan, C, seed):
    g = torch.Generator().manual_seed(seed)
    return [torch.randn(p.n, C, 16, 16, generator=g).to(DEV) for p in plan.plans]


@pytest.mark.parametrize("C", [5, 7, 33, 70])
def test_one_pass_equals_the_canvas_path(C):
    """Four views of different frame sizes and strides (overlap up to 4, shifted windows, overlap up to 8: the scanning form), flips [-, h, v, h], to a smaller
    target, a larger one and a cut of it; C = 5 / 7 and 33 and 70 run 256, 128 and 64 lanes per workgroup."""
    import mmsa.inference as inf
    for tgt, cut in (((77, 131), None), ((135, 201), None), ((135, 201), (60, 100))):
        plan = inf.AugPlan(tuple(_view_plan(g, 2, tgt, cut) for g in ("s40", "s64", "s24", "s40")), (0, 1, 2, 1))
        lgs = _logits(plan, C, 200 + C)
        got, unc, want, prob, unc2 = _both_paths(plan, lgs)
        diff = int((got != want).sum().item())
        print(f"C={C} target {tgt} cut {cut}: {diff} of {want.numel()} pixels differ, uncovered {unc} / {unc2}")
        assert unc == 0 and unc2 == 0 and got.shape == (2,) + (cut or tgt) and torch.equal(got, want), f"C={C} target {tgt} cut {cut}"
        assert_close(prob.sum(1), torch.ones_like(prob[:, 0]), tol=1e-5, what="the averaged probabilities sum to one")


def test_view_counts_and_class_limits():
    import mmsa.inference as inf
    from mmsa import lib, ops
    one = _view_plan("s40", 2, (77, 131))
    for A in (1, 12):
        plan = inf.AugPlan((one,) * A, tuple(a % 3 for a in range(A)))
        got, unc, want, _, _ = _both_paths(plan, _logits(plan, 5, 300 + A))
        assert unc == 0 and torch.equal(got, want), f"A={A}"
    # one view, not flipped: the class map of mmsa_slide_argmax_resized itself (softmax and the division by 1 keep the argmax of a single view)
    plan = inf.AugPlan((one,), (0,))
    lgs = _logits(plan, 5, 301)
    single = torch.empty(2, 77, 131, dtype=torch.uint8, device=DEV)
    unc = torch.zeros(1, dtype=torch.int32, device=DEV)
    one.class_map(lgs[0], single, unc, one_pass=True)
    near = RR.near_ties(inf._canvas_logits(one, lgs[0], unc), 1e-6)      # logits so close that their exponentials may round to the same float
    assert torch.equal(_both_paths(plan, lgs)[0][~near], single[~near]) and near.float().mean().item() < 0.01
    # 13 views and 129 classes are refused by name; 129 classes take the canvas path by default
    plan13 = inf.AugPlan((one,) * 13, (0,) * 13)
    out = torch.empty(2, 77, 131, dtype=torch.uint8, device=DEV)
    with pytest.raises(RuntimeError, match="13 views"):
        plan13.class_map(_logits(plan13, 5, 302), out, unc, one_pass=True)
    plan = inf.AugPlan((one, one), (0, 1))
    lgs = _logits(plan, 129, 303)
    with pytest.raises(RuntimeError, match="129 classes"):
        plan.class_map(lgs, out, unc, one_pass=True)
    plan.class_map(lgs, out, unc)
    assert torch.equal(out, inf.argmax_map(plan.mean_probabilities(lgs, unc)))
    # the entry validates the host copy of the window table as the other class-map entries do
    tab = (ctypes.c_int * 6)(0, 0, 0, 1, 30, 0)                                  # the second window leaves the 90 x 150 canvas
    rows = (ctypes.c_int * 11)(0, 2, 16, 16, 90, 150, 64, 64, 77, 131, 0)
    lg = torch.zeros(2, 5, 16, 16, device=DEV)
    dtab = torch.tensor(list(tab), dtype=torch.int32, device=DEV)
    with pytest.raises(RuntimeError, match="outside the"):
        lib.call("mmsa_aug_argmax", (ctypes.c_void_p * 1)(lg.data_ptr()), rows, 1, 5, dtab.data_ptr(), tab, 2, out.data_ptr(), 2, 77, 131, unc.data_ptr(), ops._stream())


def test_exact_ties_first_class_wins_in_both_paths():
    """Class 5 is a copy of class 2 and both are the maximum everywhere, in three views: every pixel is an exact tie of two probabilities, which a softmax
    or an interpolation that rounds differently in the two paths would break."""
    import mmsa.inference as inf
    plan = inf.AugPlan(tuple(_view_plan(g, 1, (135, 201)) for g in ("s40", "s24", "s64")), (1, 0, 2))
    lgs = []
    for k, p in enumerate(plan.plans):
        lg = torch.randn(p.n, 7, 16, 16, generator=torch.Generator().manual_seed(11 + k)) * 0.1
        lg[:, 2] += 3.0
        lg[:, 5] = lg[:, 2]
        lgs.append(lg.to(DEV))
    got, unc, want, prob, _ = _both_paths(plan, lgs)
    assert torch.equal(prob[:, 2], prob[:, 5]) and bool((want == 2).all()), "the canvas path must see exact ties and pick the first class"
    assert unc == 0 and torch.equal(got, want)


def test_uncovered_pixels_are_255_mirrored_and_counted_once():
    """The second view's windows sit at x0 = 0 only: columns 64 .. 87 of its 64 x 88 frame are a strip no window covers, and the view is flipped
    horizontally.  Output pixels whose MIRROR image has a tap in the strip are 255 and counted once each; all others equal the canvas path."""
    import mmsa.inference as inf
    tgt = (96, 120)
    strip = inf.MapPlan(2, 64, 88, 64, 64, ((0, 0, 0), (1, 0, 0)), tgt[0], tgt[1], tgt[0], tgt[1])
    plan = inf.AugPlan((_view_plan("s40", 2, tgt), strip, _view_plan("s64", 2, tgt)), (0, 1, 2))
    lgs = _logits(plan, 5, 3)
    count = np.zeros((2, 64, 88), dtype=np.float32)
    count[:, :, :64] = 1
    bad = torch.from_numpy(RR.touches_uncovered(count, tgt[0], tgt[1])[:, :, ::-1].copy()).to(DEV)
    got, unc, want, _, unc2 = _both_paths(plan, lgs)
    assert 0 < int(bad.sum()) < bad.numel() and unc == int(bad.sum()) and unc2 == 2 * 64 * 24, f"uncovered {unc}, the count == 0 taps imply {int(bad.sum())}"
    assert bool((got[bad] == 255).all()) and torch.equal(got[~bad], want[~bad])
    assert not bool(bad[:, :, -1].any()) and bool(bad[:, :, 0].all())          # the strip is on the right of the view, so on the left of the frame


# ---- the public entries on the tiny model

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
    return cfg, m, h, frame.to(DEV)


SLIDE_CFG = dict(mode="slide", crop_size=(256, 256), stride=(170, 170))


def test_slide_entries_two_scales_two_flips(models):
    """The 320 x 400 frame (2 x 2 windows) and its 400 x 500 resize (2 x 3 windows, up to 6 on a pixel), each plain and flipped, to ori_shape (300, 380)."""
    import mmsa.inference as inf
    cfg, m, h, frame = models
    big = F.interpolate(frame, (400, 500), mode="bilinear", align_corners=False)
    imgs, flips, ori = [frame, frame.flip(3), big, big.flip(3)], [None, "horizontal", None, "horizontal"], (300, 380, 3)
    prob = inf.aug_inference(m, h, imgs, SLIDE_CFG, ori_shape=ori, flips=flips, max_batch=4)
    want = inf.argmax_map(prob)
    assert prob.shape[0] == 1 and prob.shape[2:] == (300, 380) and want.shape == (1, 300, 380)
    assert_close(prob.sum(1), torch.ones_like(prob[:, 0]), tol=1e-5, what="the averaged probabilities sum to one")
    for one_pass in (None, True, False):
        got, unc = inf.aug_class_map(m, h, imgs, SLIDE_CFG, ori_shape=ori, flips=flips, max_batch=4, one_pass=one_pass)
        assert int(unc.item()) == 0 and got.dtype == torch.uint8 and torch.equal(got, want), f"one_pass={one_pass}"
    single = inf.argmax_map(inf.inference(m, h, frame, SLIDE_CFG, ori_shape=ori, max_batch=4))
    print(f"augmented vs single-view map: {(single != want).float().mean().item():.2%} of the pixels differ")
    # probabilities = softmax of inference's logits, flipped back
    p = inf.probabilities(m, h, big, SLIDE_CFG, ori_shape=ori, max_batch=4)
    assert torch.equal(inf.probabilities(m, h, big, SLIDE_CFG, ori_shape=ori, flip="horizontal", max_batch=4), p.flip(3))
    assert torch.equal(inf.probabilities(m, h, big, SLIDE_CFG, ori_shape=ori, flip="vertical", max_batch=4), p.flip(2))
    assert_close(p, torch.softmax(inf.inference(m, h, big, SLIDE_CFG, ori_shape=ori, max_batch=4), 1), tol=1e-5, what="probabilities vs torch.softmax")
    assert torch.equal(inf.aug_inference(m, h, [big], SLIDE_CFG, ori_shape=ori, max_batch=4), p)          # one view: p / 1
    # refusals of the entries
    with pytest.raises(RuntimeError, match="ori_shape="):
        inf.aug_class_map(m, h, [frame, big], SLIDE_CFG)
    with pytest.raises(RuntimeError, match="ori_shape="):
        inf.aug_inference(m, h, [frame, big], SLIDE_CFG)
    with pytest.raises(RuntimeError, match="same length"):
        inf.aug_class_map(m, h, imgs, SLIDE_CFG, ori_shape=ori, flips=[None])


def test_whole_mode_evaluator_table_reuse_and_graph(models):
    import mmsa.inference as inf
    from mmsa.evaluate import Evaluator, LabelPrep, confusion
    cfg, m, h, frame = models
    x = make_input(cfg, batch=2, seed=17).to(DEV)
    imgs, flips, tc, ori = [x, x.flip(3), x.flip(2)], [None, "horizontal", "vertical"], dict(mode="whole"), (200, 310)
    want = inf.argmax_map(inf.aug_inference(m, h, imgs, tc, ori_shape=ori, flips=flips))
    C = HEAD_CONFIGS["head_tiny"]["kwargs"]["num_classes"]
    lab = torch.randint(0, C, (2, 200, 310), generator=torch.Generator().manual_seed(4), dtype=torch.uint8).to(DEV)
    lp = LabelPrep(C)
    ev = Evaluator(lp, images=2, device=DEV)
    got, unc = inf.aug_class_map(m, h, imgs, tc, ori_shape=ori, flips=flips, labels=lab, evaluator=ev)
    assert int(unc.item()) == 0 and got.shape == (2, 200, 310) and torch.equal(got, want)
    assert torch.equal(ev.counts, confusion(got, lab, lp)) and int(ev.counts.sum()) == lab.numel()
    with pytest.raises(RuntimeError, match="come together"):
        inf.aug_class_map(m, h, imgs, tc, ori_shape=ori, flips=flips, labels=lab)
    # the second call finds the plan, and its window table on the device
    plan = inf.AugPlan.of(tc, [(2, 256, 256)] * 3, flips, ori)
    table = plan.table_on(DEV)
    ptr = table.data_ptr()
    again, _ = inf.aug_class_map(m, h, imgs, tc, ori_shape=ori, flips=flips)
    assert inf.AugPlan.of(tc, [(2, 256, 256)] * 3, flips, ori) is plan and plan.table_on(DEV) is table and table.data_ptr() == ptr and torch.equal(again, want)
    assert table.cpu().tolist() == [[0, 0, 0], [1, 0, 0]] * 3
    # the one-pass launch in a captured graph (single stream) replays to the same map
    lgs = [h(m(v)[0]).contiguous() for v in imgs]
    out = torch.zeros(2, 200, 310, dtype=torch.uint8, device=DEV)
    unc = torch.zeros(1, dtype=torch.int32, device=DEV)
    plan.class_map(lgs, out, unc, one_pass=True)
    torch.cuda.synchronize()
    assert torch.equal(out, want)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        plan.class_map(lgs, out, unc, one_pass=True)
    out.zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, want) and int(unc.item()) == 0


def test_raw_frames_with_preprocess(models):
    """`imgs` as (rgb, aux) pairs of raw frames with `preprocess=`, one object for all views or one per view: the same maps and probabilities as from the
    normalised tensors (normalising is per pixel, so a flipped raw frame is the flipped tensor)."""
    import mmsa.inference as inf
    from mmsa.preprocess import Preprocess
    cfg, m, h, frame = models
    pre = Preprocess(mean=[0.485, 0.456, 0.406, 0, 0, 0], std=[0.229, 0.224, 0.225, 1, 1, 1], to_rgb=[True, True], modalities_name=["rgb", "lidar"],
                     modalities_ch=[3, 3], norm_by_max=True)
    g = torch.Generator().manual_seed(21)
    flips, ori = [None, "horizontal"], (300, 380)
    for tc, (H, W) in ((SLIDE_CFG, (320, 400)), (dict(mode="whole"), (256, 256))):
        rgb = torch.randint(0, 256, (1, H, W, 3), generator=g, dtype=torch.uint8).to(DEV)
        aux = torch.randint(0, 256, (1, H, W, 3), generator=g, dtype=torch.uint8).to(DEV)
        raw = [(rgb, aux), (rgb.flip(2).contiguous(), aux.flip(2).contiguous())]
        tens = [pre(*v) for v in raw]
        assert torch.equal(tens[1], tens[0].flip(3))
        want_p = inf.aug_inference(m, h, tens, tc, ori_shape=ori, flips=flips, max_batch=4)
        want = inf.argmax_map(want_p)
        assert torch.equal(inf.aug_inference(m, h, raw, tc, ori_shape=ori, flips=flips, preprocess=pre, max_batch=4), want_p)
        for one_pass, pp in ((True, pre), (False, [pre, pre])):
            got, unc = inf.aug_class_map(m, h, raw, tc, ori_shape=ori, flips=flips, preprocess=pp, max_batch=4, one_pass=one_pass)
            assert int(unc.item()) == 0 and torch.equal(got, want), f"{tc['mode']} one_pass={one_pass}"
    with pytest.raises(RuntimeError, match="same length"):
        inf.aug_class_map(m, h, raw, tc, ori_shape=ori, flips=flips, preprocess=[pre])


# ---- against the reference's own aug_test

@pytest.mark.parametrize("tag", sorted(AR.CASES))
def test_against_the_reference_fixture(golden_dir, tag):
    """The toy encode_decode of the fixture as a backbone / head pair on the device: 4 x 4 average pooling, then the seeded 1 x 1 conv.  The averaged
    probabilities come from the canvas path (aug_inference), the class map from aug_class_map -- except for case `slide`, whose 1.25 x views (113 x 188 under
    stride 40) have 3 x 3 windows on some pixels: one more than the one-pass kernels take, so aug_class_map refuses it as slide_class_map would, and its
    class map is argmax_map of the canvas path."""
    import mmsa.inference as inf
    g = np.load(os.path.join(golden_dir, "aug.npz"))
    case = AR.case_of(g[f"{tag}_cfg"])
    hw, crop, stride, ori, _ = case
    imgs, flips = AR.views_of(case)
    imgs = [v.to(DEV) for v in imgs]
    want, want_map = torch.from_numpy(g[f"{tag}_prob"]), torch.from_numpy(g[f"{tag}_map"]).long()
    w = torch.randn(RR.NUM_CLASSES, 6, 1, 1, generator=torch.Generator().manual_seed(RR.TOY_SEED)).to(DEV)
    bb = lambda im: ([F.avg_pool2d(im, 4)], None)
    hd = lambda feats: F.conv2d(feats[0], w).contiguous()
    tc = dict(mode="whole") if crop is None else dict(mode="slide", crop_size=crop, stride=stride)
    prob = inf.aug_inference(bb, hd, imgs, tc, ori_shape=ori, flips=flips)
    if tag == "slide":
        with pytest.raises(RuntimeError, match="covers some pixels 9 times"):
            inf.aug_class_map(bb, hd, imgs, tc, ori_shape=ori, flips=flips)
        cm = inf.argmax_map(prob)
    else:
        cm, unc = inf.aug_class_map(bb, hd, imgs, tc, ori_shape=ori, flips=flips)
        assert int(unc.item()) == 0 and torch.equal(cm, inf.argmax_map(prob))
    r, mx = assert_close(prob, want, what=f"averaged probabilities, case {tag}")
    skip = AR.near_ties(want, REL_TOL)
    share = skip.float().mean().item()
    wrong = int(((cm.cpu().long() != want_map[None]) & ~skip).sum())
    print(f"aug {tag}: probabilities rel_l2 {r:.2e} max_rel {mx:.2e}; {share:.4%} near-tie pixels excluded; {wrong} other pixels differ")
    assert share <= 0.01 and wrong == 0
