"""mmsa.render on the GPU against the numpy restatement of tensor2imgs + crop + show_result (tests/render_ref.py): bit for bit, no tolerance."""
import numpy as np
import pytest
import torch

from tests import preprocess_ref as PR
from tests import render_ref as RR

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
LIDAR = dict(mean=[0.485, 0.456, 0.406, 1.4628459, 1.8271197, 0.07808967], std=[0.229, 0.224, 0.225, 7.55678107, 9.85001751, 0.67012253],
             modalities_name=["rgb", "lidar"], modalities_ch=[3, 3])
PAL256 = np.array([(i, 255 - i, (37 * i) % 256) for i in range(256)])
GUARD = 64      # bytes in front of and behind a guarded buffer


def _pp(variant, to_rgb=(True, False), norm_by_max=True, pad_size=None):
    from mmsa.preprocess import Preprocess
    return Preprocess(to_rgb=list(to_rgb), norm_by_max=norm_by_max, variant=variant, pad_size=pad_size, **LIDAR)


def _guarded(shape):
    """A contiguous uint8 view of `shape` inside a larger buffer filled with 0xA5 -> (view, whole buffer)."""
    n = int(np.prod(shape))
    buf = torch.full((n + 2 * GUARD,), 0xA5, dtype=torch.uint8, device=DEV)
    return buf[GUARD:GUARD + n].view(*shape), buf


def _guard_intact(buf):
    return bool((buf[:GUARD] == 0xA5).all()) and bool((buf[-GUARD:] == 0xA5).all())


@pytest.mark.parametrize("opacity", (0.3, 0.5, 0.7, 1.0))
def test_exhaustive_blend_image(opacity):
    """All 256 x 256 (image value, colour value) pairs in one launch, for the colour map alone and over a raw frame."""
    from mmsa.render import Renderer
    pred = np.repeat(np.arange(256, dtype=np.uint8)[None], 256, 0)[None]                      # pred[y, x] = x
    src = np.repeat(np.arange(256, dtype=np.uint8)[:, None, None], 256, 1).repeat(3, 2)[None]    # source value y in all three channels
    r = Renderer(PAL256, opacity=opacity)
    d_pred, d_src = torch.from_numpy(pred).to(DEV), torch.from_numpy(np.ascontiguousarray(src)).to(DEV)
    assert np.array_equal(r(d_pred).cpu().numpy(), RR.render_ref(pred, PAL256, opacity))
    assert np.array_equal(r(d_pred, d_src).cpu().numpy(), RR.render_ref(pred, PAL256, opacity, src))


@pytest.mark.parametrize("h,w", ((37, 53), (64, 128), (5, 3)))
def test_edge_paths(h, w):
    """pred is a strided view of a wider map, the source is larger than (h, w), the palette has 25 entries and the map holds 25..255 as well; both
    channel-reverse settings of the palette and of the source; nothing is written outside the picture."""
    from mmsa.render import Renderer
    g = np.random.default_rng(h * 1000 + w)
    B = 2
    wide = g.integers(0, 256, (B, h + 3, w + 7), dtype=np.uint8)
    wide[:, :, ::5] = g.integers(0, 25, wide[:, :, ::5].shape, dtype=np.uint8)
    wide[0, 0, 0], wide[1, h - 1, w - 1] = 255, 24
    pal = g.integers(0, 256, (25, 3))
    src = g.integers(0, 256, (B, h + 2, w + 5, 3), dtype=np.uint8)
    d_wide, d_src = torch.from_numpy(wide).to(DEV), torch.from_numpy(src).to(DEV)
    pred, d_pred = wide[:, :h, :w], d_wide[:, :h, :w]
    assert not d_pred.is_contiguous()
    for bgr in (True, False):
        r = Renderer(pal, opacity=0.3, bgr=bgr)
        out, buf = _guarded((B, h, w, 3))
        assert r(d_pred, out=out) is out
        assert np.array_equal(out.cpu().numpy(), RR.render_ref(pred, pal, 0.3, bgr=bgr)) and _guard_intact(buf)
        for rev in (False, True):
            out, buf = _guarded((B, h, w, 3))
            r(d_pred, d_src, img_shape=(h, w), out=out, source_reverse=rev)
            want = RR.render_ref(pred, pal, 0.3, src[..., ::-1] if rev else src, bgr=bgr)
            assert np.array_equal(out.cpu().numpy(), want) and _guard_intact(buf), (bgr, rev)


@pytest.mark.parametrize("variant,to_rgb", (("multimodal", (True, True)), ("muses", (True, False)), ("muses", (False, False))))
@pytest.mark.parametrize("h,w", ((37, 53), (64, 128)))
def test_tensor_form(variant, to_rgb, h, w):
    """The output of Preprocess on random uint8 frames, de-normalised as tensor2imgs does; the frame is larger than the map (the pad is cropped away)."""
    from mmsa.render import Renderer
    g = np.random.default_rng(h + w)
    B, Hs, Ws = 2, h + 3, w + 4
    pp = _pp(variant, to_rgb)
    rgb, aux = g.integers(0, 256, (B, Hs, Ws, 3), dtype=np.uint8), g.integers(0, 256, (B, Hs, Ws, 3), dtype=np.uint8)
    x = pp(torch.from_numpy(rgb).to(DEV), torch.from_numpy(aux).to(DEV))
    assert np.array_equal(x.cpu().numpy(), PR.normalize_ref(rgb, aux, LIDAR["mean"], LIDAR["std"], pp.to_rgb, pp.modalities_name, pp.norm_by_max, pp.variant))
    pred = g.integers(0, 30, (B, h, w), dtype=np.uint8)
    pal = g.integers(0, 256, (25, 3))
    r = Renderer(pal, opacity=0.7, preprocess=pp)
    out, buf = _guarded((B, h, w, 3))
    r(torch.from_numpy(pred).to(DEV), x, out=out)
    pic = RR.tensor2imgs_ref(x.cpu().numpy(), LIDAR["mean"], LIDAR["std"], pp.to_rgb[0], pp.div255[0])
    assert np.abs(pic.astype(int) - rgb.astype(int)).max() <= 1            # tensor2imgs restores the frame up to one level
    assert np.array_equal(out.cpu().numpy(), RR.render_ref(pred, pal, 0.7, pic)) and _guard_intact(buf)


def test_tensor_form_saturates():
    """Hand-set tensor values that de-normalise below 0 and above 255 saturate (the one deviation from the reference's C cast); NaN gives 0."""
    from mmsa.render import Renderer
    pp = _pp("muses")
    x = np.zeros((1, 6, 4, 8), dtype=np.float32)
    x[0, 0] = np.array([-50, -2.2, -2.1179, 0, 2.2489, 2.3, 1e30, np.nan], dtype=np.float32)
    x[0, 1] = np.array([-1e30, 3, 2.5, 2.43, 2.42, -2.03, -2.04, 0.5], dtype=np.float32)
    x[0, 2, 1:] = np.float32(7)
    pred = np.full((1, 4, 8), 255, dtype=np.uint8)
    r = Renderer([[9, 9, 9]], opacity=1.0, preprocess=pp)
    pic = RR.tensor2imgs_ref(x, LIDAR["mean"], LIDAR["std"], True, True)
    assert pic.min() == 0 and pic.max() == 255 and pic[0, 0, 7, 2] == 0
    half = Renderer([[9, 9, 9]], opacity=0.5, preprocess=pp)
    assert np.array_equal(half(torch.from_numpy(pred).to(DEV), torch.from_numpy(x).to(DEV)).cpu().numpy(), RR.render_ref(pred, [[9, 9, 9]], 0.5, pic))
    assert int(r(torch.from_numpy(pred).to(DEV), torch.from_numpy(x).to(DEV)).max()) == 0      # opacity 1.0: the source has no weight


def test_refusals():
    import mmsa.lib as lib
    from mmsa import ops
    from mmsa.render import Renderer
    pal = np.zeros((25, 3), dtype=np.int64)
    with pytest.raises(ValueError, match="1..256 entries, got 257"):
        Renderer(np.zeros((257, 3), dtype=np.int64))
    for bad in (0, 1.5):
        with pytest.raises(ValueError, match=r"must be in \(0, 1\]"):
            Renderer(pal, opacity=bad)
    r = Renderer(pal, preprocess=_pp("muses"))
    pred = torch.zeros(1, 8, 12, dtype=torch.uint8, device=DEV)
    with pytest.raises(RuntimeError, match="img_shape"):
        r(pred, img_shape=(8, 11))
    with pytest.raises(RuntimeError, match="smaller than the 8 x 12 map"):
        r(pred, torch.zeros(1, 8, 11, 3, dtype=torch.uint8, device=DEV))
    with pytest.raises(RuntimeError, match="smaller than the 8 x 12 map"):
        r(pred, torch.zeros(1, 6, 7, 12, device=DEV))
    with pytest.raises(RuntimeError, match="no CPU path"):
        r(pred.cpu())
    with pytest.raises(RuntimeError, match="no CPU path"):
        r(pred, torch.zeros(1, 8, 12, 3, dtype=torch.uint8))
    with pytest.raises(RuntimeError, match="preprocess="):
        Renderer(pal)(pred, torch.zeros(1, 6, 8, 12, device=DEV))
    # the entries refuse the same on their own, with a negative return and a message
    out = torch.full((1, 8, 12, 3), 7, dtype=torch.uint8, device=DEV)
    p = r.palette_on(DEV)
    src = torch.zeros(1, 8, 11, 3, dtype=torch.uint8, device=DEV)
    with pytest.raises(RuntimeError, match="1..256 entries, got 257"):
        lib.call("mmsa_render_u8", pred.data_ptr(), 96, 12, 1, 8, 12, p.data_ptr(), 257, 1, None, 0, 0, 0, 0.5, 0.5, out.data_ptr(), ops._stream())
    with pytest.raises(RuntimeError, match="smaller than the 8 x 12 map"):
        lib.call("mmsa_render_u8", pred.data_ptr(), 96, 12, 1, 8, 12, p.data_ptr(), 25, 1, src.data_ptr(), 8, 11, 0, 0.5, 0.5, out.data_ptr(), ops._stream())
    with pytest.raises(RuntimeError, match="null argument"):
        lib.call("mmsa_render_u8", None, 96, 12, 1, 8, 12, p.data_ptr(), 25, 1, None, 0, 0, 0, 0.5, 0.5, out.data_ptr(), ops._stream())
    with pytest.raises(RuntimeError, match=r"must be in \(0, 1\]"):
        lib.call("mmsa_render_u8", pred.data_ptr(), 96, 12, 1, 8, 12, p.data_ptr(), 25, 1, None, 0, 0, 0, 1.5, -0.5, out.data_ptr(), ops._stream())
    with pytest.raises(RuntimeError, match="null argument"):
        lib.call("mmsa_render_denorm_f32", pred.data_ptr(), 96, 12, 1, 8, 12, p.data_ptr(), 25, 1, None, 6, 8, 12, r._c_mean, r._c_std, 1, 1, 0.5, 0.5,
                 out.data_ptr(), ops._stream())
    torch.cuda.synchronize()
    assert bool((out == 7).all())                                          # a refused call launches nothing


@pytest.fixture(scope="module")
def models():
    import mmsa
    from oracle import ref_encoder as R
    from oracle import ref_head as RH
    from tests.configs import CONFIGS, HEAD_CONFIGS
    from tests.weights import seeded_state_dict
    cfg, hcfg = CONFIGS["tiny256"], HEAD_CONFIGS["head_tiny"]
    sd = seeded_state_dict(R.OracleEncoder(**cfg["kwargs"]), seed=cfg["seed"])
    hsd = seeded_state_dict(RH.OracleSegformerHead(**hcfg["kwargs"]), seed=hcfg["seed"])
    m = mmsa.build_backbone(dict(type="SAMAdapterbimodalMixModNewInTwinConvNEW", **cfg["kwargs"]))
    m.load_state_dict(sd)
    h = mmsa.build_head(dict(type="SegformerHead", **hcfg["kwargs"]))
    h.load_state_dict(hsd)
    return hcfg["kwargs"]["num_classes"], m, h


def _frames(g, shape):
    return g.integers(0, 256, shape, dtype=np.uint8), g.integers(0, 256, shape, dtype=np.uint8)


def _tensor_pic(pp, x):
    return RR.tensor2imgs_ref(x.cpu().numpy(), LIDAR["mean"], LIDAR["std"], pp.to_rgb[0], pp.div255[0])


def test_class_map_calls_with_render(models):
    """whole_class_map / slide_class_map with render= return the map they return without it and the picture Renderer paints from that map: over the
    raw frame with preprocess= on uint8 frames of the map's size, over the de-normalised tensor otherwise."""
    import mmsa.inference as inf
    from mmsa.render import Renderer
    C, m, h = models
    g = np.random.default_rng(5)
    pp = _pp("muses")
    pal = g.integers(0, 256, (C, 3))
    r = Renderer(pal, opacity=0.3, preprocess=pp)
    rgb, aux = _frames(g, (2, 256, 256, 3))
    pair = (torch.from_numpy(rgb).to(DEV), torch.from_numpy(aux).to(DEV))
    want = inf.whole_class_map(m, h, pair, preprocess=pp)
    got, pic = inf.whole_class_map(m, h, pair, preprocess=pp, render=r)
    assert torch.equal(got, want) and torch.equal(pic, r(want, pair[0]))
    assert np.array_equal(pic.cpu().numpy(), RR.render_ref(want.cpu().numpy(), pal, 0.3, rgb))
    x = pp(*pair)
    got, pic = inf.whole_class_map(m, h, x, render=r)                      # a normalised tensor: the `tensor` form
    assert torch.equal(got, want) and torch.equal(pic, r(want, x))
    assert np.array_equal(pic.cpu().numpy(), RR.render_ref(want.cpu().numpy(), pal, 0.3, _tensor_pic(pp, x)))
    with pytest.raises(RuntimeError, match="preprocess="):
        inf.whole_class_map(m, h, x, render=Renderer(pal))

    rgb, aux = _frames(g, (1, 256, 400, 3))                                # a frame of two windows
    pair = (torch.from_numpy(rgb).to(DEV), torch.from_numpy(aux).to(DEV))
    want, unc = inf.slide_class_map(m, h, pair, (256, 256), (170, 170), preprocess=pp)
    got, unc2, pic = inf.slide_class_map(m, h, pair, (256, 256), (170, 170), preprocess=pp, render=r)
    assert torch.equal(got, want) and int(unc.item()) == int(unc2.item()) == 0 and torch.equal(pic, r(want, pair[0]))
    assert np.array_equal(pic.cpu().numpy(), RR.render_ref(want.cpu().numpy(), pal, 0.3, rgb))
    x = pp(*pair)
    got, _, pic = inf.slide_class_map(m, h, x, (256, 256), (170, 170), render=r)
    assert torch.equal(got, want) and torch.equal(pic, r(want, x))
    # a raw frame that is not the map's size has no source in slide mode: refused by name, before any launch
    ppad = _pp("muses", pad_size=(256, 416))
    with pytest.raises(RuntimeError, match="no source for the picture"):
        inf.slide_class_map(m, h, pair, (256, 256), (170, 170), preprocess=ppad, render=r)


def test_slide_runner_with_render(models):
    """SlideRunner(render=): picture() is the restatement of that frame's map over the raw frame, run after run, from a static buffer."""
    import mmsa.inference as inf
    from mmsa.render import Renderer
    C, m, h = models
    g = np.random.default_rng(6)
    pp = _pp("muses")
    pal = g.integers(0, 256, (C, 3))
    r = Renderer(pal, opacity=0.5, preprocess=pp)
    rgb, aux = _frames(g, (1, 300, 420, 3))
    d_rgb, d_aux = torch.from_numpy(rgb).to(DEV), torch.from_numpy(aux).to(DEV)
    plain = inf.SlideRunner(m, h, (d_rgb, d_aux), (256, 256), (160, 160), chains=2, preprocess=pp)
    want = plain.run().outputs()[0].clone()
    with pytest.raises(RuntimeError, match="without render="):
        plain.run().picture()
    sr = inf.SlideRunner(m, h, (d_rgb, d_aux), (256, 256), (160, 160), chains=2, preprocess=pp, render=r)
    res = sr.run()
    cm, unc = res.outputs()
    pic = res.picture()
    torch.cuda.synchronize()
    assert torch.equal(cm, want) and int(unc.item()) == 0
    assert np.array_equal(pic.cpu().numpy(), RR.render_ref(want.cpu().numpy(), pal, 0.5, rgb))
    before = torch.cuda.memory_allocated()
    res = sr.run()
    pic2 = res.picture()
    torch.cuda.synchronize()
    assert torch.cuda.memory_allocated() <= before                         # the second run allocates nothing
    assert pic2.data_ptr() == pic.data_ptr() and np.array_equal(pic2.cpu().numpy(), RR.render_ref(want.cpu().numpy(), pal, 0.5, rgb))
    with pytest.raises(RuntimeError, match="return_map=False"):
        sr.run(return_map=False)
