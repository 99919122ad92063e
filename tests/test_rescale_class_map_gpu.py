"""Class maps at the rescaled size (`rescale=True`): the one-pass kernel mmsa_slide_argmax_resized against the canvas path (bilinear_accum with
accumulate + div_count + bilinear_accum in write mode + argmax_nchw + crop) bit for bit, the public entries of mmsa.inference on the tiny model, and
both against the reference's own rescaled predictions (tests/golden/rescale.npz)."""
import ctypes
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import rescale_ref as RR
from tests.configs import CONFIGS, HEAD_CONFIGS, make_input
from tests.util import REL_TOL, assert_close
from tests.weights import seeded_state_dict

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

TARGETS = [(135, 201), (77, 131), (90, 300), (45, 75), (90, 150)]      # up, down, mixed, exactly half, identity (of the 90 x 150 frame)
GEOMETRIES = dict(s40=((90, 150), (40, 40)),       # a 2 x 4 grid with shifted last row and column, overlap up to 4
                  s64=((70, 70), (64, 64)),        # 2 x 2 windows shifted by 6
                  s24=((90, 150), (32, 24)))       # overlap up to 8: taps under 5 .. 8 windows (the kernel's scanning form)


def _windows(hw, stride, B):
    import mmsa.inference as inf
    return [(b, y1, x1) for (y1, x1, _, _) in inf.crop_boxes(hw[0], hw[1], (64, 64), stride) for b in range(B)]


def _canvas_path(lg, wins, B, H, W, hc, wc, tgt, cut=None):
    """The parent's launches: canvas (accumulate, count), division, second canvas, argmax, crop -> (map, canvas count)."""
    import mmsa.inference as inf
    from mmsa import lib, ops
    C = lg.shape[1]
    canvas = torch.zeros(B, C, H, W, device=DEV)
    count = torch.zeros(B, H, W, device=DEV)
    for k, (b, y0, x0) in enumerate(wins):
        inf._resize_into(lg[k:k + 1], canvas[b:b + 1], y0, x0, hc, wc, count=count[b:b + 1], accumulate=True)
    lib.call("mmsa_div_count_nchw", canvas.data_ptr(), count.data_ptr(), B, C, H * W, ops._stream())
    second = torch.empty(B, C, tgt[0], tgt[1], device=DEV)
    inf._resize_into(canvas, second, 0, 0, tgt[0], tgt[1])
    m = inf.argmax_map(second)
    if cut is not None:
        m = m[:, :cut[0], :cut[1]].contiguous()
    return m, count, second


def _one_pass(lg, wins, B, H, W, hc, wc, tgt, cut=None):
    from mmsa import lib, ops
    cut = cut or tgt
    out = torch.full((B, cut[0], cut[1]), 77, dtype=torch.uint8, device=DEV)
    unc = torch.zeros(1, dtype=torch.int32, device=DEV)
    tab = (ctypes.c_int * (3 * len(wins)))(*[v for w in wins for v in w])
    lib.call("mmsa_slide_argmax_resized", lg.data_ptr(), len(wins), lg.shape[1], lg.shape[2], lg.shape[3], tab, out.data_ptr(), B, H, W, hc, wc,
             tgt[0], tgt[1], cut[0], cut[1], unc.data_ptr(), ops._stream())
    return out, int(unc.item())


@pytest.mark.parametrize("C", [5, 7])
@pytest.mark.parametrize("geo", sorted(GEOMETRIES))
def test_kernel_equals_the_canvas_path(geo, C):
    from mmsa import lib, ops
    (H, W), stride = GEOMETRIES[geo]
    B = 2
    wins = _windows((H, W), stride, B)
    lg = torch.randn(len(wins), C, 16, 16, generator=torch.Generator().manual_seed(100 + C)).to(DEV)
    for tgt in TARGETS + [(H, W)]:
        want, count, _ = _canvas_path(lg, wins, B, H, W, 64, 64, tgt)
        got, unc = _one_pass(lg, wins, B, H, W, 64, 64, tgt)
        diff = int((got != want).sum().item())
        print(f"{geo} C={C} {H}x{W} -> {tgt}: {diff} of {want.numel()} pixels differ, uncovered {unc}, overlap up to {int(count.max().item())}")
        assert unc == 0 and torch.equal(got, want), f"{geo} C={C} target {tgt}"
    # the identity target is mmsa_slide_argmax itself
    same = torch.empty(B, H, W, dtype=torch.uint8, device=DEV)
    unc = torch.zeros(1, dtype=torch.int32, device=DEV)
    tab = (ctypes.c_int * (3 * len(wins)))(*[v for w in wins for v in w])
    lib.call("mmsa_slide_argmax", lg.data_ptr(), len(wins), C, 16, 16, tab, same.data_ptr(), B, H, W, 64, 64, unc.data_ptr(), ops._stream())
    assert torch.equal(_one_pass(lg, wins, B, H, W, 64, 64, (H, W))[0], same) and int(unc.item()) == 0
    # a cut: the top-left corner of the rescaled map, and of the map at the frame's own size (whole_dim_cut without rescale)
    for tgt, cut in (((135, 201), (60, 100)), ((H, W), (60, 50))):
        got, unc = _one_pass(lg, wins, B, H, W, 64, 64, tgt, cut)
        assert unc == 0 and got.shape == (B,) + cut and torch.equal(got, _canvas_path(lg, wins, B, H, W, 64, 64, tgt, cut)[0]), f"cut {cut} of {tgt}"
    with pytest.raises(RuntimeError, match="inside the target"):
        _one_pass(lg, wins, B, H, W, 64, 64, (77, 131), (78, 131))


@pytest.mark.parametrize("stride", [(40, 40), (32, 24)])
def test_exact_ties_first_class_wins_in_both_paths(stride):
    """Class 5 is a copy of class 2 and both are the maximum everywhere: every pixel of both stages is an exact tie, which a fused multiply-add in one
    path and not the other would break."""
    H, W, B = 90, 150, 1
    wins = _windows((H, W), stride, B)
    lg = torch.randn(len(wins), 7, 16, 16, generator=torch.Generator().manual_seed(11)) * 0.1
    lg[:, 2] += 3.0
    lg[:, 5] = lg[:, 2]
    lg = lg.to(DEV)
    for tgt in ((135, 201), (77, 131), (90, 300)):
        want, _, second = _canvas_path(lg, wins, B, H, W, 64, 64, tgt)
        got, unc = _one_pass(lg, wins, B, H, W, 64, 64, tgt)
        assert torch.equal(second[:, 2], second[:, 5]) and bool((want == 2).all()), "the canvas path must see exact ties and pick the first class"
        assert unc == 0 and torch.equal(got, want), f"target {tgt}: the one-pass map rounds differently from the canvas path"


def test_uncovered_taps_are_255_and_counted():
    """Windows at x0 = 0 only: columns 64 .. 87 of the 64 x 88 frame are a strip no window covers.  Output pixels with a tap in the strip are 255 and
    counted once each; all others equal the canvas path."""
    H, W, B = 64, 88, 2
    wins = [(0, 0, 0), (1, 0, 0)]
    lg = torch.randn(2, 5, 16, 16, generator=torch.Generator().manual_seed(3)).to(DEV)
    for tgt in ((96, 120), (40, 50)):
        want, count, _ = _canvas_path(lg, wins, B, H, W, 64, 64, tgt)
        bad = torch.from_numpy(RR.touches_uncovered(count.cpu().numpy(), tgt[0], tgt[1])).to(DEV)
        got, unc = _one_pass(lg, wins, B, H, W, 64, 64, tgt)
        assert 0 < int(bad.sum()) < bad.numel() and unc == int(bad.sum()), f"uncovered {unc}, the count == 0 taps imply {int(bad.sum())}"
        assert bool((got[bad] == 255).all()) and torch.equal(got[~bad], want[~bad])


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


def test_slide_entries_at_ori_shape(models):
    """A 320 x 400 frame, 256 x 256 windows, stride 170 (2 x 2 windows, every pixel count from 1 to 4), rescaled to (300, 380)."""
    import mmsa.inference as inf
    cfg, m, h, frame = models
    ori = (300, 380, 3)
    want = inf.argmax_map(inf.slide_inference(m, h, frame, (256, 256), (170, 170), max_batch=2, ori_shape=ori))
    assert want.shape == (1, 300, 380)
    for one_pass in (None, True, False):
        got, unc = inf.slide_class_map(m, h, frame, (256, 256), (170, 170), max_batch=2, ori_shape=ori, one_pass=one_pass)
        assert int(unc.item()) == 0 and got.dtype == torch.uint8 and torch.equal(got, want), f"one_pass={one_pass}"
    sr = inf.SlideRunner(m, h, frame, (256, 256), (170, 170), chains=2, ori_shape=ori)
    assert sr.out.shape == (1, 300, 380)
    for _ in range(2):
        cm, unc = sr.run().outputs()
        torch.cuda.synchronize()
        assert int(unc.item()) == 0 and torch.equal(cm, want)
    # rescale=False and the frame's own size leave everything as it was
    plain = inf.slide_inference(m, h, frame, (256, 256), (170, 170), max_batch=2)
    assert torch.equal(inf.slide_inference(m, h, frame, (256, 256), (170, 170), max_batch=2, ori_shape=ori, rescale=False), plain)
    assert torch.equal(inf.slide_inference(m, h, frame, (256, 256), (170, 170), max_batch=2, ori_shape=(320, 400, 3)), plain)
    assert torch.equal(inf.slide_class_map(m, h, frame, (256, 256), (170, 170), max_batch=2, ori_shape=(320, 400))[0], inf.argmax_map(plain))


def test_whole_entries_and_class_map_dispatch(models):
    import mmsa.inference as inf
    cfg, m, h, frame = models
    x = make_input(cfg, batch=2, seed=17).to(DEV)
    am = inf.argmax_map
    assert torch.equal(inf.whole_class_map(m, h, x, ori_shape=(200, 310)), am(inf.whole_inference(m, h, x, ori_shape=(200, 310))))
    assert torch.equal(inf.whole_class_map(m, h, x, dim=(192, 240)), am(inf.whole_inference_dim(m, h, x, (192, 240))))
    for dim, cut, rescale in (((200, 300), (260, 150), True), ((192, 256), (256, 192), False), ((200, 300), (400, 400), True)):
        got = inf.whole_class_map(m, h, x, dim=dim, cut_dim=cut, rescale=rescale)
        want = am(inf.whole_inference_dim_cut(m, h, x, dim, cut, rescale=rescale))
        assert got.shape == want.shape and got.is_contiguous() and torch.equal(got, want), f"whole_dim_cut {dim} {cut} rescale={rescale}"
    cfgs = [dict(mode="slide", crop_size=(256, 256), stride=(170, 170)), dict(mode="whole"), dict(mode="whole_dim", dim=(300, 280)),
            dict(mode="whole_dim_cut", dim=(300, 280), cut_dim=(250, 270))]
    for tc in cfgs:
        img = frame if tc["mode"] == "slide" else x
        for rescale in (True, False):
            if tc["mode"] == "whole_dim" and not rescale:
                for fn in (inf.inference, inf.class_map):
                    with pytest.raises(RuntimeError, match="no defined result"):
                        fn(m, h, img, tc, rescale=False)
                continue
            want = am(inf.inference(m, h, img, tc, rescale=rescale, ori_shape=(210, 333, 3)))
            got = inf.class_map(m, h, img, tc, rescale=rescale, ori_shape=(210, 333, 3))
            assert torch.equal(got, want), f"class_map {tc} rescale={rescale}"
    assert inf.class_map(m, h, x, dict(mode="whole"), ori_shape=(210, 333, 3)).shape == (2, 210, 333)
    with pytest.raises(RuntimeError, match="not one of"):
        inf.class_map(m, h, x, dict(mode="slide_mod_sel"))


def test_evaluator_and_refusals(models):
    import mmsa.inference as inf
    from mmsa.evaluate import Evaluator, LabelPrep, confusion
    from mmsa.preprocess import Preprocess
    from mmsa.render import Renderer
    cfg, m, h, frame = models
    x = make_input(cfg, batch=2, seed=17).to(DEV)
    C = HEAD_CONFIGS["head_tiny"]["kwargs"]["num_classes"]
    lab = torch.randint(0, C, (2, 200, 310), generator=torch.Generator().manual_seed(4), dtype=torch.uint8).to(DEV)
    lp = LabelPrep(C)
    ev = Evaluator(lp, images=2, device=DEV)
    got = inf.class_map(m, h, x, dict(mode="whole"), ori_shape=(200, 310), labels=lab, evaluator=ev)
    assert torch.equal(ev.counts, confusion(got, lab, lp)) and int(ev.counts.sum()) == lab.numel()
    ev1 = Evaluator(lp, images=1, device=DEV)
    cm, unc = inf.slide_class_map(m, h, frame, (256, 256), (170, 170), max_batch=2, ori_shape=(200, 310), labels=lab[:1], evaluator=ev1)
    assert torch.equal(ev1.counts, confusion(cm, lab[:1], lp))
    for kw in (dict(fused=True), dict(return_map=False)):
        with pytest.raises(RuntimeError, match="no variant at a rescaled"):
            inf.whole_class_map(m, h, x, ori_shape=(200, 310), labels=lab, evaluator=Evaluator(lp, images=2, device=DEV), **kw)
        with pytest.raises(RuntimeError, match="no variant at a rescaled"):
            inf.slide_class_map(m, h, frame, (256, 256), (170, 170), ori_shape=(200, 310), labels=lab[:1], evaluator=Evaluator(lp, images=1, device=DEV), **kw)
    rgb = dict(mean=[0.485, 0.456, 0.406, 0, 0, 0], std=[0.229, 0.224, 0.225, 1, 1, 1], to_rgb=[True, True], modalities_name=["rgb", "lidar"],
               modalities_ch=[3, 3], norm_by_max=True)
    r = Renderer(np.arange(3 * C).reshape(C, 3) % 256, opacity=0.5, preprocess=Preprocess(**rgb))
    with pytest.raises(RuntimeError, match="no source for the picture"):       # the normalised tensor is no source for a map of another size
        inf.whole_class_map(m, h, x, ori_shape=(200, 310), render=r)
    with pytest.raises(RuntimeError, match="no source for the picture"):
        inf.slide_class_map(m, h, frame, (256, 256), (170, 170), ori_shape=(200, 310), render=r)
    cm, pic = inf.whole_class_map(m, h, x, dim=(256, 256), cut_dim=(200, 180), render=r)      # a cut alone: the top-left of the input tensor is the source
    assert cm.shape == (2, 180, 200) and pic.shape == (2, 180, 200, 3)
    with pytest.raises(RuntimeError, match="comes with dim"):
        inf.whole_class_map(m, h, x, cut_dim=(200, 180))
    with pytest.raises(RuntimeError, match="give one of them"):
        inf.whole_class_map(m, h, x, dim=(200, 180), ori_shape=(200, 180))
    with pytest.raises(RuntimeError, match="RESCALED"):
        inf.whole_class_map(m, h, x, one_pass=True)


# ---- against the reference's own rescaled predictions

@pytest.mark.parametrize("tag", ["a", "c", "w"])
def test_against_the_reference_fixture(golden_dir, tag):
    """The toy encode_decode of the fixture as a backbone / head pair on the device: 4 x 4 average pooling, then the seeded 1 x 1 conv."""
    import mmsa.inference as inf
    g = np.load(os.path.join(golden_dir, "rescale.npz"))
    hw, crop, stride, ori = RR.case_of(g[f"{tag}_cfg"])
    want = torch.from_numpy(g[f"{tag}_out"])
    w = torch.randn(RR.NUM_CLASSES, 6, 1, 1, generator=torch.Generator().manual_seed(RR.TOY_SEED)).to(DEV)
    bb = lambda im: ([F.avg_pool2d(im, 4)], None)
    hd = lambda feats: F.conv2d(feats[0], w).contiguous()
    img = RR.frame(hw).to(DEV)
    if crop is None:
        logits = inf.whole_inference(bb, hd, img, ori_shape=ori)
        cm = inf.whole_class_map(bb, hd, img, ori_shape=ori)
    else:
        logits = inf.slide_inference(bb, hd, img, crop, stride, ori_shape=ori)
        cm, unc = inf.slide_class_map(bb, hd, img, crop, stride, ori_shape=ori)
        assert int(unc.item()) == 0
    r, mx = assert_close(logits, want, what=f"rescaled logits, case {tag}")
    skip = RR.near_ties(want, REL_TOL)
    share = skip.float().mean().item()
    wrong = int(((cm.cpu().long() != want.argmax(1)) & ~skip).sum())
    print(f"rescale {tag}: logits rel_l2 {r:.2e} max_rel {mx:.2e}; {share:.4%} near-tie pixels excluded; {wrong} other pixels differ")
    assert share <= 0.01 and wrong == 0
