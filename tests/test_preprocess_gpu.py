"""GPU tests of mmsa.preprocess: raw HWC frames (uint8 / float32) -> normalised, padded NCHW, whole and as the windows of slide inference.
Every comparison is bit-exact (torch.equal) against the numpy float32 restatement of the reference's pipeline (tests/preprocess_ref.py)."""
import ctypes

import numpy as np
import pytest
import torch

from tests import preprocess_ref as PR
from tests.configs import CONFIGS, HEAD_CONFIGS
from tests.weights import seeded_state_dict

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
LIDAR = dict(mean=[0.485, 0.456, 0.406, 1.4628459, 1.8271197, 0.07808967], std=[0.229, 0.224, 0.225, 7.55678107, 9.85001751, 0.67012253],
             modalities_name=["rgb", "lidar"], modalities_ch=[3, 3])


def _pp(variant="muses", to_rgb=(True, False), norm_by_max=True, pad_size=None, pad_val=0, **kw):
    from mmsa.preprocess import Preprocess
    return Preprocess(to_rgb=list(to_rgb), norm_by_max=norm_by_max, variant=variant, pad_size=pad_size, pad_val=pad_val, **dict(LIDAR, **kw))


def _ref(pp, rgb, aux):
    return torch.from_numpy(PR.normalize_ref(rgb, aux, LIDAR["mean"], LIDAR["std"], pp.to_rgb, pp.modalities_name, pp.norm_by_max, pp.variant,
                                             pad_size=pp.pad_size, pad_val=pp.pad_val[0]))


def _sources(g, shape, dtype):
    """uint8: the decoder's bytes.  float32: non-integers, negatives and LiDAR-sized values (~1e2), a few exact bytes among them."""
    if dtype == np.uint8:
        return g.integers(0, 256, shape, dtype=np.uint8)
    x = g.normal(0, 100, shape).astype(np.float32)
    x.reshape(-1)[::7] = g.integers(0, 256, x.reshape(-1)[::7].shape).astype(np.float32)
    return x


@pytest.mark.parametrize("Hs,Ws,pad", [(37, 53, None), (600, 800, (800, 800)), (1080, 1920, None)])
def test_whole_frame_equals_the_float32_restatement(Hs, Ws, pad):
    """Both variants, all four to_rgb combinations, sources u8/u8, u8/f32, f32/f32, B = 1 and 3: 37 x 53 (odd: the edge path everywhere),
    600 x 800 padded to 800 x 800 (FMB: pad pixels are the NORMALISED pad value, not 0) and a 1080 x 1920 MUSES frame."""
    g = np.random.default_rng(Hs)
    for B in (1, 3):
        for dts in ((np.uint8, np.uint8), (np.uint8, np.float32), (np.float32, np.float32)):
            rgb, aux = _sources(g, (B, Hs, Ws, 3), dts[0]), _sources(g, (B, Hs, Ws, 3), dts[1])
            d_rgb, d_aux = torch.from_numpy(rgb).to(DEV), torch.from_numpy(aux).to(DEV)
            for variant in ("multimodal", "muses"):
                for to_rgb in ((False, False), (True, False), (False, True), (True, True)):
                    pp = _pp(variant, to_rgb, pad_size=pad)
                    got = pp(d_rgb, d_aux).cpu()
                    want = _ref(pp, rgb, aux)
                    what = f"{variant} to_rgb {to_rgb} {dts[0].__name__}/{dts[1].__name__} B {B}"
                    assert got.shape == want.shape and got.dtype == torch.float32, what
                    assert torch.equal(got, want), f"{what}: {int((got != want).sum())} of {want.numel()} values differ, max {float((got - want).abs().max()):.3e}"
                    if pad is not None:
                        for c in range(6):      # stated explicitly: a padded pixel is (pad_val [/ 255] - mean) * sinv, and that is not 0
                            a = np.float32(0) / np.float32(255) if pp.div255[c // 3] else np.float32(0)
                            v = float((a - pp.mean[c]) * pp.sinv[c])
                            assert v != 0.0 and bool((got[:, c, Hs:, :] == v).all()) and bool((got[:, c, :, Ws:] == v).all()), f"{what}: padding of channel {c}"
    # norm_by_max=False and a non-zero pad value per modality
    pp = _pp("multimodal", (True, True), norm_by_max=False, pad_size=(Hs + 3, Ws + 5), pad_val=7)
    assert torch.equal(pp(d_rgb, d_aux).cpu(), _ref(pp, rgb, aux))


def _jobs(H, W, crop, stride, B):
    import mmsa.inference as inf
    return [(b, box) for box in inf.crop_boxes(H, W, crop, stride) for b in range(B)]


def test_crops_equal_crop_batch_of_the_whole_frame():
    """pp.crops == mmsa_crop_batch_nchw(pp(...)) on the MUSES grid (1080 x 1920, crop 1024, stride 640: windows shifted inwards at the borders), on a
    grid with odd x0 (the unaligned path) and on a padded canvas whose windows reach into the padding."""
    import mmsa.inference as inf
    g = np.random.default_rng(3)
    for (Hs, Ws), crop, stride, B, pad, dts in (((1080, 1920), (1024, 1024), (640, 640), 1, None, (np.uint8, np.uint8)),
                                                ((1080, 1920), (1024, 1024), (640, 640), 1, None, (np.uint8, np.float32)),
                                                ((1080, 1920), (1024, 1024), (640, 640), 1, None, (np.float32, np.float32)),
                                                ((301, 421), (256, 256), (45, 55), 2, None, (np.uint8, np.float32)),      # x0 = 55, 110, 165 (border): odd
                                                ((203, 259), (130, 150), (73, 109), 2, None, (np.float32, np.uint8)),    # crop width no multiple of 4
                                                ((600, 800), (512, 512), (288, 288), 2, (800, 800), (np.uint8, np.uint8))):
        rgb, aux = _sources(g, (B, Hs, Ws, 3), dts[0]), _sources(g, (B, Hs, Ws, 3), dts[1])
        d_rgb, d_aux = torch.from_numpy(rgb).to(DEV), torch.from_numpy(aux).to(DEV)
        pp = _pp("muses", (True, False), pad_size=pad)
        H, W = pp.canvas(Hs, Ws)
        jobs = _jobs(H, W, crop, stride, B)
        if (Hs, Ws) == (1080, 1920):
            assert [(y, x) for _, (y, x, _, _) in jobs] == [(y, x) for y in (0, 56) for x in (0, 640, 896)]
        if (Hs, Ws) == (301, 421):
            assert any(x % 2 for _, (_, x, _, _) in jobs)
        assert len(jobs) <= 64
        got = pp.crops(d_rgb, d_aux, jobs, crop)
        want = inf._crops(pp(d_rgb, d_aux), jobs, crop)
        assert got.shape == (len(jobs), 6) + tuple(crop) and torch.equal(got, want), f"{Hs}x{Ws} crop {crop} stride {stride} {dts}"
        out = torch.full_like(got, float("nan"))
        assert pp.crops(d_rgb, d_aux, jobs, crop, out=out) is out and torch.equal(out, want)
    # and against the restatement directly (not only against this package's own whole-frame launch)
    ref = _ref(pp, rgb, aux)
    want = torch.stack([ref[b, :, y1:y2, x1:x2] for b, (y1, x1, y2, x2) in jobs], 0)
    assert torch.equal(got.cpu(), want)


def test_crops_are_graph_capturable():
    g = np.random.default_rng(11)
    rgb = torch.from_numpy(_sources(g, (1, 300, 420, 3), np.uint8)).to(DEV)
    aux = torch.from_numpy(_sources(g, (1, 300, 420, 3), np.float32)).to(DEV)
    pp = _pp()
    jobs = _jobs(300, 420, (256, 256), (160, 160), 1)
    out = torch.zeros(len(jobs), 6, 256, 256, device=DEV)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        pp.crops(rgb, aux, jobs, (256, 256), out=out)
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        pp.crops(rgb, aux, jobs, (256, 256), out=out)
    for rep in range(3):
        rgb.copy_(torch.from_numpy(_sources(g, (1, 300, 420, 3), np.uint8)).to(DEV))       # the graph reads the caller's buffers
        aux.copy_(torch.from_numpy(_sources(g, (1, 300, 420, 3), np.float32)).to(DEV))
        out.zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, pp.crops(rgb, aux, jobs, (256, 256)))


def test_refusals_on_device():
    import mmsa
    pp = _pp()
    u8 = torch.zeros(1, 40, 48, 3, dtype=torch.uint8, device=DEV)
    f32 = torch.zeros(1, 40, 48, 3, device=DEV)
    pp(u8, f32)
    with pytest.raises(RuntimeError, match="GPU tensor"):
        pp(u8.cpu(), f32)
    with pytest.raises(RuntimeError, match="GPU tensor"):
        pp(u8, f32.cpu())
    for bad in (u8.to(torch.float16), u8.to(torch.int32), u8.to(torch.float64)):
        with pytest.raises(RuntimeError, match="uint8 or float32"):
            pp(bad, f32)
    with pytest.raises(RuntimeError, match="contiguous"):
        pp(torch.zeros(1, 48, 40, 3, dtype=torch.uint8, device=DEV).transpose(1, 2), f32)
    with pytest.raises(RuntimeError, match="contiguous"):
        pp(u8, torch.zeros(1, 3, 40, 48, device=DEV).permute(0, 2, 3, 1))                      # a CHW tensor viewed as HWC
    for ch in (1, 4):
        with pytest.raises(RuntimeError, match="3 channels"):
            pp(u8, torch.zeros(1, 40, 48, ch, device=DEV))
    with pytest.raises(RuntimeError, match="3 channels"):
        pp(u8[0], f32[0])                                                                       # no batch axis
    with pytest.raises(RuntimeError, match="differ in shape"):
        pp(u8, torch.zeros(1, 40, 44, 3, device=DEV))
    with pytest.raises(RuntimeError, match="smaller"):                                          # H < Hs
        _pp(pad_size=(32, 48))(u8, f32)
    args = (u8.data_ptr(), 0, f32.data_ptr(), 1, 1, 40, 48, pp._c_mean, pp._c_sinv, pp._c_div, pp._c_swap, pp._c_pad)
    out = torch.zeros(1, 6, 40, 48, device=DEV)
    with pytest.raises(RuntimeError, match="smaller than"):                                     # the same refusal at the C boundary
        mmsa.lib.call("mmsa_preprocess_nhwc", *args, out.data_ptr(), 39, 48, mmsa.ops._stream())
    # windows: outside the padded canvas, more than 64
    padded = _pp(pad_size=(64, 64))
    padded.crops(u8, f32, [(0, (32, 32, 64, 64))], (32, 32))                                    # inside the PADDED canvas, beyond the source: fine
    with pytest.raises(RuntimeError, match="outside"):
        padded.crops(u8, f32, [(0, (33, 32, 65, 64))], (32, 32))
    with pytest.raises(RuntimeError, match="outside"):
        pp.crops(u8, f32, [(0, (16, 32, 48, 64))], (32, 32))                                    # without padding the canvas is the 40 x 48 source
    with pytest.raises(RuntimeError, match="outside"):
        pp.crops(u8, f32, [(1, (0, 0, 32, 32))], (32, 32))                                      # image index
    with pytest.raises(RuntimeError, match="at most 64"):
        pp.crops(u8, f32, [(0, (0, 0, 8, 8))] * 65, (8, 8))
    with pytest.raises(RuntimeError, match="`out`"):
        pp.crops(u8, f32, [(0, (0, 0, 8, 8))], (8, 8), out=torch.zeros(1, 6, 8, 9, device=DEV))
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


def _event_frames(g, shape):
    """uint8 RGB + a sparse uint8 auxiliary map (most pixels 0, like a projected LiDAR / event frame)."""
    rgb = g.integers(0, 256, shape, dtype=np.uint8)
    aux = (g.integers(0, 256, shape) * (g.random(shape) < 0.05)).astype(np.uint8)
    return rgb, aux


def test_slide_runner_on_raw_frames_equals_the_prenormalised_path(models):
    """SlideRunner(..., preprocess=pp) on raw uint8 frames == SlideRunner on the float frame the host pipeline would have uploaded, class map bit for
    bit, run after run; then through FrameFeeder over 6 frames while the caller overwrites its arrays right after feed()."""
    import mmsa.inference as inf
    from mmsa.preprocess import FrameFeeder
    m, h = models
    g = np.random.default_rng(77)
    pp = _pp("muses", (True, False))
    shape = (1, 300, 420, 3)
    rgb, aux = _event_frames(g, shape)
    d_rgb, d_aux = torch.from_numpy(rgb).to(DEV), torch.from_numpy(aux).to(DEV)
    frame = _ref(pp, rgb, aux).to(DEV)
    sr_raw = inf.SlideRunner(m, h, (d_rgb, d_aux), (256, 256), (160, 160), chains=2, preprocess=pp)
    sr_ref = inf.SlideRunner(m, h, frame, (256, 256), (160, 160), chains=2)
    assert torch.equal(sr_raw.crops, sr_ref.crops)
    for rep in range(3):
        if rep == 2:                       # new contents in the runners' static inputs: the two raw buffers / the float frame
            rgb, aux = _event_frames(g, shape)
            d_rgb.copy_(torch.from_numpy(rgb).to(DEV))
            d_aux.copy_(torch.from_numpy(aux).to(DEV))
            frame.copy_(_ref(pp, rgb, aux).to(DEV))
        cm, unc = sr_raw.run().outputs()
        got = cm.clone()
        want, unc2 = sr_ref.run().outputs()
        torch.cuda.synchronize()
        assert int(unc.item()) == 0 and int(unc2.item()) == 0 and torch.equal(got, want), f"run {rep}"
    # the plain functions take the same argument
    want = inf.argmax_map(inf.slide_inference(m, h, frame, (256, 256), (160, 160), max_batch=3))
    got = inf.argmax_map(inf.slide_inference(m, h, (d_rgb, d_aux), (256, 256), (160, 160), max_batch=3, preprocess=pp))
    assert torch.equal(got, want)
    assert torch.equal(inf.inference(m, h, (d_rgb, d_aux), dict(mode="slide", crop_size=(256, 256), stride=(160, 160)), preprocess=pp),
                       inf.inference(m, h, frame, dict(mode="slide", crop_size=(256, 256), stride=(160, 160))))
    cm_a, _ = inf.slide_class_map(m, h, (d_rgb, d_aux), (256, 256), (160, 160), max_batch=3, preprocess=pp)
    cm_b, _ = inf.slide_class_map(m, h, frame, (256, 256), (160, 160), max_batch=3)
    assert torch.equal(cm_a, cm_b)
    with pytest.raises(RuntimeError, match="pair"):
        inf.slide_class_map(m, h, frame, (256, 256), (160, 160), preprocess=pp)
    with pytest.raises(RuntimeError, match="only with preprocess"):
        sr_ref.run(frame=(d_rgb, d_aux))
    # FrameFeeder: host arrays in, overwritten by the caller as soon as feed() returns (no device-wide sync in between: outputs() waits for its own pass only)
    feeder = FrameFeeder(pp, shape[:3], slots=2)
    h_rgb, h_aux = np.empty(shape, np.uint8), np.empty(shape, np.uint8)
    frames, maps = [], []
    for k in range(6):
        r, a = _event_frames(g, shape)
        frames.append((r, a))
        h_rgb[:], h_aux[:] = r, a
        pair = feeder.feed(h_rgb, h_aux)
        h_rgb[:], h_aux[:] = 255 - r, 1                      # the caller's arrays are its own again
        maps.append(sr_raw.run(frame=pair).outputs()[0].clone())
    torch.cuda.synchronize()
    for k, (r, a) in enumerate(frames):
        frame.copy_(_ref(pp, r, a).to(DEV))
        want = sr_ref.run().outputs()[0]
        torch.cuda.synchronize()
        assert torch.equal(maps[k], want), f"frame {k} through the feeder"
    with pytest.raises(RuntimeError, match="expected"):
        feeder.feed(h_rgb[:, :100], h_aux[:, :100])
    with pytest.raises(RuntimeError, match="expected"):
        feeder.feed(h_rgb.astype(np.float32), h_aux)


def test_whole_class_map_on_raw_frames_equals_the_prenormalised_path(models):
    """whole_class_map(preprocess=pp) on raw frames (an FMB-like 192 x 256 frame padded to the model's 256 x 256, uint8 RGB + float32 auxiliary map) ==
    whole_class_map on the pre-normalised float frame, call after call and through FrameFeeder; the whole modes of `inference` likewise."""
    import mmsa.inference as inf
    from mmsa.preprocess import FrameFeeder
    m, h = models
    g = np.random.default_rng(5)
    pp = _pp("multimodal", (True, True), pad_size=(256, 256))
    shape = (2, 192, 256, 3)

    def make():
        return g.integers(0, 256, shape, dtype=np.uint8), (g.random(shape) * 255).astype(np.float32)

    feeder = FrameFeeder(pp, shape[:3], slots=2, dtypes=(torch.uint8, torch.float32))
    h_rgb, h_aux = np.empty(shape, np.uint8), np.empty(shape, np.float32)
    frames, maps = [], []
    for k in range(5):
        r, a = make()
        frames.append((r, a))
        h_rgb[:], h_aux[:] = r, a
        pair = feeder.feed(h_rgb, h_aux)
        h_rgb[:], h_aux[:] = 0, -1.0
        maps.append(inf.whole_class_map(m, h, pair, preprocess=pp))
    torch.cuda.synchronize()
    for k, (r, a) in enumerate(frames):
        frame = _ref(pp, r, a).to(DEV)
        assert torch.equal(maps[k], inf.whole_class_map(m, h, frame)), f"frame {k}"
        pair = (torch.from_numpy(r).to(DEV), torch.from_numpy(a).to(DEV))
        assert torch.equal(inf.whole_class_map(m, h, pair, preprocess=pp), maps[k])             # without the feeder, again
    for cfg in (dict(mode="whole"), dict(mode="whole_dim", dim=(256, 256)), dict(mode="whole_dim_cut", dim=(192, 256), cut_dim=(256, 192))):
        assert torch.equal(inf.inference(m, h, pair, cfg, rescale=cfg["mode"] != "whole_dim_cut", preprocess=pp),
                           inf.inference(m, h, frame, cfg, rescale=cfg["mode"] != "whole_dim_cut"))
