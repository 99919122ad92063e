"""GPU tests of the device resize of mmsa.preprocess: raw HWC frames of one size -> resized (OpenCV bilinear), padded, normalised NCHW, whole and as
the windows of slide inference.  Every comparison is bit-exact (torch.equal on float32) against the numpy restatement tests/preprocess_resize_ref.py."""
import numpy as np
import pytest
import torch

from tests import preprocess_resize_ref as RR
from tests.configs import CONFIGS, HEAD_CONFIGS
from tests.weights import seeded_state_dict

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
LIDAR = dict(mean=[0.485, 0.456, 0.406, 1.4628459, 1.8271197, 0.07808967], std=[0.229, 0.224, 0.225, 7.55678107, 9.85001751, 0.67012253],
             modalities_name=["rgb", "lidar"], modalities_ch=[3, 3])
U8, F32 = np.uint8, np.float32


def _pp(scale, keep_ratio, variant="multimodal", to_rgb=(True, True), pad_size=None, pad_val=0, device_resize=True):
    from mmsa.preprocess import Preprocess
    return Preprocess(to_rgb=list(to_rgb), norm_by_max=True, variant=variant, pad_size=pad_size, pad_val=pad_val,
                      resize=dict(img_scale=scale, keep_ratio=keep_ratio), device_resize=device_resize, **LIDAR)


def _ref(pp, rgb, aux):
    return torch.from_numpy(RR.pipeline_ref(rgb, aux, pp.resize, LIDAR["mean"], LIDAR["std"], pp.to_rgb, pp.modalities_name, pp.norm_by_max, pp.variant,
                                            pad_size=pp.pad_size, pad_val=pp.pad_val[0]))


def _sources(g, shape, dtype):
    if dtype == U8:
        return g.integers(0, 256, shape, dtype=np.uint8)
    x = g.normal(0, 100, shape).astype(np.float32)
    x.reshape(-1)[::7] = g.integers(0, 256, x.reshape(-1)[::7].shape).astype(np.float32)
    return x


def _same(got, want, what):
    assert got.shape == want.shape and got.dtype == torch.float32, what
    assert torch.equal(got, want), f"{what}: {int((got != want).sum())} of {want.numel()} values differ, max {float((got - want).abs().max()):.3e}"


# (source h, w), img_scale (w, h), keep_ratio, pad_size, batch
CASES = [((1042, 1042), (1024, 1024), True, None, 2),          # DELIVER
         ((1080, 1920), (1024, 1024), True, None, 1),          # -> 576 x 1024: a source span beyond the staging buffer for float32 sources
         ((600, 800), (1024, 768), False, None, 1),            # upscale, keep_ratio=False
         ((37, 53), (41, 64), False, None, 3),                 # odd sizes, width not divisible by 4: the edge path everywhere
         ((200, 300), (517, 131), False, None, 1),
         ((600, 800), (640, 480), False, (512, 672), 2),       # resize, then pad
         ((301, 421), (2049, 77), False, None, 1)]             # three workgroups per row, the last with one column


@pytest.mark.parametrize("case", CASES, ids=lambda c: f"{c[0][0]}x{c[0][1]}->{c[1]}{'k' if c[2] else ''}{'p' if c[3] else ''}")
def test_uint8_pair_equals_the_fixed_point_restatement(case):
    (Hs, Ws), scale, keep, pad, B = case
    g = np.random.default_rng(Hs + Ws)
    rgb, aux = _sources(g, (B, Hs, Ws, 3), U8), _sources(g, (B, Hs, Ws, 3), U8)
    d_rgb, d_aux = torch.from_numpy(rgb).to(DEV), torch.from_numpy(aux).to(DEV)
    for variant, to_rgb in (("multimodal", (True, True)), ("muses", (True, False)), ("multimodal", (False, True)), ("muses", (False, False))):
        pp = _pp(scale, keep, variant, to_rgb, pad_size=pad)
        got = pp(d_rgb, d_aux).cpu()
        _same(got, _ref(pp, rgb, aux), f"{variant} to_rgb {to_rgb} B {B}")
        assert tuple(got.shape[2:]) == pp.canvas(Hs, Ws)
    if pad is not None:
        Hr, Wr = pp.resized(Hs, Ws)
        for c in range(6):
            a = np.float32(0) / np.float32(255) if pp.div255[c // 3] else np.float32(0)
            v = float((a - pp.mean[c]) * pp.sinv[c])
            assert bool((got[:, c, Hr:, :] == v).all()) and bool((got[:, c, :, Wr:] == v).all()), f"padding of channel {c}"
        nz = _pp(scale, keep, pad_size=pad, pad_val=7)
        _same(nz(d_rgb, d_aux).cpu(), _ref(nz, rgb, aux), "pad_val 7")


@pytest.mark.parametrize("case", CASES[:5], ids=lambda c: f"{c[0][0]}x{c[0][1]}->{c[1]}")
def test_float_and_mixed_pairs_equal_the_float32_restatement(case):
    """float32 + float32, and the mixed pairs: BOTH modalities on the float32 path, the uint8 one converted exactly."""
    (Hs, Ws), scale, keep, pad, B = case
    g = np.random.default_rng(Hs * 3 + Ws)
    for dts in ((F32, F32), (U8, F32), (F32, U8)):
        rgb, aux = _sources(g, (B, Hs, Ws, 3), dts[0]), _sources(g, (B, Hs, Ws, 3), dts[1])
        pp = _pp(scale, keep, "muses", (True, False), pad_size=pad)
        _same(pp(torch.from_numpy(rgb).to(DEV), torch.from_numpy(aux).to(DEV)).cpu(), _ref(pp, rgb, aux), f"{dts[0].__name__}/{dts[1].__name__}")


def _jobs(H, W, crop, stride, B):
    import mmsa.inference as inf
    return [(b, box) for box in inf.crop_boxes(H, W, crop, stride) for b in range(B)]


def test_crops_equal_slices_of_the_whole_output():
    g = np.random.default_rng(9)
    for (Hs, Ws), scale, keep, pad, crop, stride, B, dts in (((1042, 1042), (1024, 1024), True, None, (512, 512), (320, 320), 1, (U8, U8)),
                                                              ((1080, 1920), (1024, 1024), True, None, (512, 512), (64, 341), 1, (U8, U8)),     # odd x0
                                                              ((301, 421), (333, 290), False, (300, 340), (130, 150), (85, 95), 2, (U8, U8)),   # windows reach the padding
                                                              ((301, 421), (333, 290), False, None, (130, 150), (85, 95), 2, (U8, F32)),
                                                              ((203, 259), (400, 310), False, None, (256, 256), (54, 144), 1, (F32, F32))):
        rgb, aux = _sources(g, (B, Hs, Ws, 3), dts[0]), _sources(g, (B, Hs, Ws, 3), dts[1])
        d_rgb, d_aux = torch.from_numpy(rgb).to(DEV), torch.from_numpy(aux).to(DEV)
        pp = _pp(scale, keep, "muses", (True, False), pad_size=pad)
        H, W = pp.canvas(Hs, Ws)
        jobs = _jobs(H, W, crop, stride, B)
        assert 1 < len(jobs) <= 64
        whole = pp(d_rgb, d_aux)
        want = torch.stack([whole[b, :, y1:y2, x1:x2] for b, (y1, x1, y2, x2) in jobs], 0)
        got = pp.crops(d_rgb, d_aux, jobs, crop)
        assert got.shape == (len(jobs), 6) + tuple(crop) and torch.equal(got, want), f"{Hs}x{Ws} -> {H}x{W} crop {crop} stride {stride}"
        out = torch.full_like(got, float("nan"))
        assert pp.crops(d_rgb, d_aux, jobs, crop, out=out) is out and torch.equal(out, want)
    ref = _ref(pp, rgb, aux)
    assert torch.equal(got.cpu(), torch.stack([ref[b, :, y1:y2, x1:x2] for b, (y1, x1, y2, x2) in jobs], 0))


def test_equal_sizes_through_the_new_entries_equal_the_existing_launch():
    import ctypes
    import mmsa
    g = np.random.default_rng(21)
    Hs, Ws, B = 203, 259, 2
    for dts in ((U8, U8), (U8, F32), (F32, F32)):
        rgb = torch.from_numpy(_sources(g, (B, Hs, Ws, 3), dts[0])).to(DEV)
        aux = torch.from_numpy(_sources(g, (B, Hs, Ws, 3), dts[1])).to(DEV)
        pp = _pp((Ws, Hs), False, "muses", (True, False), pad_size=(224, 272))
        want = pp(rgb, aux)                                                          # identity resize: the existing entry
        for fixed in ((True, False) if dts == (U8, U8) else (False,)):
            tabs = pp.resize_tables(Hs, Ws, Hs, Ws, fixed, rgb.device)
            rs = (Hs, Ws) + tuple(t.data_ptr() for t in tabs) + (int(fixed),)
            got = torch.full_like(want, float("nan"))
            mmsa.lib.call("mmsa_preprocess_resize_nhwc", *pp._args(rgb, aux), got.data_ptr(), 224, 272, *rs, mmsa.ops._stream())
            assert torch.equal(got, want), f"{dts} fixed {fixed}"
            jobs = _jobs(224, 272, (128, 128), (96, 144), B)
            tab = (ctypes.c_int * (3 * len(jobs)))(*[int(v) for b, (y1, x1, _, _) in jobs for v in (b, y1, x1)])
            gc = torch.full((len(jobs), 6, 128, 128), float("nan"), device=DEV)
            mmsa.lib.call("mmsa_preprocess_resize_crops", *pp._args(rgb, aux), 224, 272, tab, len(jobs), gc.data_ptr(), 128, 128, *rs, mmsa.ops._stream())
            assert torch.equal(gc, pp.crops(rgb, aux, jobs, (128, 128)))


def test_second_call_of_a_geometry_is_graph_capturable():
    g = np.random.default_rng(11)
    shape = (1, 300, 420, 3)
    rgb, aux = torch.from_numpy(_sources(g, shape, U8)).to(DEV), torch.from_numpy(_sources(g, shape, U8)).to(DEV)
    pp = _pp((384, 288), False, "muses", (True, False))
    jobs = _jobs(288, 384, (256, 256), (32, 128), 1)
    out = torch.zeros(len(jobs), 6, 256, 256, device=DEV)
    whole = torch.zeros(1, 6, 288, 384, device=DEV)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        pp.crops(rgb, aux, jobs, (256, 256), out=out)                                # uploads the tables of this geometry
    torch.cuda.current_stream().wait_stream(s)
    assert len(pp._tables) == 1
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        pp.crops(rgb, aux, jobs, (256, 256), out=out)
        pp(rgb, aux, out=whole)
    assert len(pp._tables) == 1
    for rep in range(3):
        rgb.copy_(torch.from_numpy(_sources(g, shape, U8)).to(DEV))
        aux.copy_(torch.from_numpy(_sources(g, shape, U8)).to(DEV))
        out.zero_()
        whole.zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, pp.crops(rgb, aux, jobs, (256, 256))) and torch.equal(whole, pp(rgb, aux))
        _same(whole.cpu(), _ref(pp, rgb.cpu().numpy(), aux.cpu().numpy()), f"replay {rep}")
    # another geometry gets its own tables (the refusal to build them DURING a capture is tested without a device, tests/test_preprocess_resize_cpu.py)
    other = torch.zeros(1, 200, 300, 3, dtype=torch.uint8, device=DEV)
    pp(other, other)
    assert len(pp._tables) == 2


def test_refusals_on_device():
    pp = _pp((64, 48), False)
    u8 = torch.zeros(1, 40, 52, 3, dtype=torch.uint8, device=DEV)
    pp(u8, u8)
    for bad in (u8.to(torch.float16), u8.to(torch.int32), u8.to(torch.float64), u8.to(torch.int8)):
        with pytest.raises(RuntimeError, match="uint8 or float32"):
            pp(bad, u8)
        with pytest.raises(RuntimeError, match="uint8 or float32"):
            pp.crops(u8, bad, [(0, (0, 0, 8, 8))], (8, 8))
    with pytest.raises(NotImplementedError, match="INTER_AREA"):
        pp(torch.zeros(1, 96, 128, 3, dtype=torch.uint8, device=DEV), torch.zeros(1, 96, 128, 3, dtype=torch.uint8, device=DEV))
    with pytest.raises(NotImplementedError, match="only the identity"):
        _pp((64, 48), False, device_resize=False)(u8, u8)
    with pytest.raises(RuntimeError, match="outside"):                                # windows are checked against the RESIZED canvas (48 x 64)
        pp.crops(u8, u8, [(0, (20, 0, 52, 32))], (32, 32))
    pp.crops(u8, u8, [(0, (16, 32, 48, 64))], (32, 32))                               # beyond the 40 x 52 source, inside the canvas
    torch.cuda.synchronize()


@pytest.fixture(scope="module")
def models():
    import mmsa
    cfg, hcfg = CONFIGS["tiny256"], HEAD_CONFIGS["head_tiny"]
    m = mmsa.build_backbone(dict(type="SAMAdapterbimodalMixModNewInTwinConvNEW", **cfg["kwargs"]))
    m.load_state_dict(seeded_state_dict(m, seed=cfg["seed"]))
    h = mmsa.build_head(dict(type="SegformerHead", **hcfg["kwargs"]))
    h.load_state_dict(seeded_state_dict(h, seed=hcfg["seed"]))
    return m, h.to(DEV)


def test_whole_modes_from_resized_sources_equal_the_tensor_path(models):
    """266 x 266 sources resized to the model's 256 x 256 (the DELIVER arrangement at test size): whole_class_map and inference(mode 'whole_dim')
    on the raw pair equal the same call on the tensor pp(rgb, aux) returns, which equals the restatement."""
    import mmsa.inference as inf
    m, h = models
    g = np.random.default_rng(5)
    pp = _pp((256, 256), True, "multimodal", (True, True))
    shape = (2, 266, 266, 3)
    rgb, aux = _sources(g, shape, U8), _sources(g, shape, U8)
    pair = (torch.from_numpy(rgb).to(DEV), torch.from_numpy(aux).to(DEV))
    frame = pp(*pair)
    assert frame.shape == (2, 6, 256, 256)
    _same(frame.cpu(), _ref(pp, rgb, aux), "266 -> 256")
    assert torch.equal(inf.whole_class_map(m, h, pair, preprocess=pp), inf.whole_class_map(m, h, frame))
    cfg = dict(mode="whole_dim", dim=(256, 256))
    assert torch.equal(inf.inference(m, h, pair, cfg, preprocess=pp), inf.inference(m, h, frame, cfg))


def test_slide_runner_and_feeder_with_source_size_other_than_the_canvas(models):
    """FrameFeeder(shape = the SOURCE shape) + SlideRunner(preprocess=pp) on 330 x 462 frames resized to a 300 x 420 canvas returns the class map
    of slide_class_map on the same raw pair, and of the plain path on the resized, normalised tensor."""
    import mmsa.inference as inf
    from mmsa.preprocess import FrameFeeder
    m, h = models
    g = np.random.default_rng(77)
    pp = _pp((420, 300), False, "muses", (True, False))
    shape = (1, 330, 462, 3)
    rgb, aux = _sources(g, shape, U8), _sources(g, shape, U8)
    d_rgb, d_aux = torch.from_numpy(rgb).to(DEV), torch.from_numpy(aux).to(DEV)
    sr = inf.SlideRunner(m, h, (d_rgb, d_aux), (256, 256), (160, 160), chains=2, preprocess=pp)
    assert tuple(sr.out.shape) == (1, 300, 420)
    feeder = FrameFeeder(pp, shape[:3], slots=2)
    frames, maps = [], []
    for k in range(4):
        r, a = _sources(g, shape, U8), _sources(g, shape, U8)
        frames.append((r, a))
        maps.append(sr.run(frame=feeder.feed(r, a)).outputs()[0].clone())
    torch.cuda.synchronize()
    for k, (r, a) in enumerate(frames):
        pair = (torch.from_numpy(r).to(DEV), torch.from_numpy(a).to(DEV))
        want, unc = inf.slide_class_map(m, h, pair, (256, 256), (160, 160), max_batch=3, preprocess=pp)
        assert int(unc.item()) == 0 and torch.equal(maps[k], want), f"frame {k} through the feeder"
        plain, _ = inf.slide_class_map(m, h, _ref(pp, r, a).to(DEV), (256, 256), (160, 160), max_batch=3)
        assert torch.equal(want, plain)
    assert torch.equal(inf.argmax_map(inf.slide_inference(m, h, pair, (256, 256), (160, 160), preprocess=pp)), want)
    with pytest.raises(RuntimeError, match="shape, dtypes and device"):              # run(frame=) wants the SOURCE geometry of the runner's buffers
        sr.run(frame=(torch.zeros(1, 300, 420, 3, dtype=torch.uint8, device=DEV),) * 2)
    with pytest.raises(RuntimeError, match="expected"):
        feeder.feed(r[:, :300, :420], a[:, :300, :420])
