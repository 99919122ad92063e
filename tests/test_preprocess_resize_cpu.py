"""Host side of the device resize of mmsa.preprocess (no GPU): the opt-in, the geometry, the C boundary of the two new entries, the per-axis tables,
the refusals, and the numpy restatement the GPU tests compare against (tests/preprocess_resize_ref.py) held to DERIVED bounds of the exact bilinear
value computed independently in float64 (torch.nn.functional.interpolate, bilinear, align_corners=False: same sampling positions and edge rule)."""
import ctypes
import os

import numpy as np
import pytest
import torch

from tests import preprocess_ref as PR
from tests import preprocess_resize_ref as RR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_ENTRIES = ("mmsa_preprocess_resize_nhwc", "mmsa_preprocess_resize_crops")
GEOMETRIES = (((1042, 1042), (1024, 1024)), ((600, 800), (768, 1024)), ((1080, 1920), (576, 1024)), ((37, 53), (64, 41)), ((200, 300), (131, 517)),
              ((1042, 1042), (2084, 2084)))


def test_geometry_of_the_opt_in():
    """Fails on a tree without the feature (unknown keyword)."""
    from mmsa.preprocess import Preprocess
    cfgs = RR.load_cfgs()
    pp = Preprocess.from_pipeline(RR.pipeline_of(cfgs["deliver_rgb_lidar"]), resize="device")
    assert pp.device_resize and pp.resize == dict(img_scale=(1024, 1024), keep_ratio=True)
    assert pp.canvas(1042, 1042) == (1024, 1024) and pp.resized(1042, 1042) == (1024, 1024)
    assert pp.canvas(1024, 1024) == (1024, 1024)
    assert pp.canvas(1080, 1920) == (576, 1024)                                  # keep_ratio: the largest size inside (1024, 1024)
    # the same pipeline as the existing fixture writes it (values of tests/golden/preprocess_cfgs.json), and the default stays the identity only
    old = PR.load_cfgs()["deliver_rgb_lidar"]
    assert Preprocess.from_pipeline(PR.pipeline_of(old), resize="device").canvas(1042, 1042) == (1024, 1024)
    with pytest.raises(NotImplementedError, match="only the identity"):
        Preprocess.from_pipeline(PR.pipeline_of(old)).canvas(1042, 1042)
    # keep_ratio=False: (h, w) of the (w, h) scale; hand-built form
    kw = dict(mean=[0.5] * 6, std=[0.25] * 6, to_rgb=[True, False], modalities_name=["rgb", "lidar"], modalities_ch=[3, 3])
    fixed = Preprocess(resize=dict(img_scale=(640, 480), keep_ratio=False), device_resize=True, **kw)
    assert fixed.canvas(600, 800) == (480, 640) and fixed.canvas(37, 53) == (480, 640)
    with pytest.raises(NotImplementedError, match="only the identity"):
        Preprocess(resize=dict(img_scale=(640, 480), keep_ratio=False), **kw).canvas(600, 800)
    # resize, then pad
    rp = Preprocess.from_pipeline(RR.pipeline_of(cfgs["resize_then_pad"]), resize="device")
    assert rp.resized(600, 800) == (480, 640) and rp.canvas(600, 800) == (512, 672)
    small = Preprocess(resize=dict(img_scale=(640, 480), keep_ratio=False), device_resize=True, pad_size=(400, 640), **kw)
    with pytest.raises(RuntimeError, match="smaller than the 480 x 640 resized frame"):
        small.canvas(600, 800)
    # new_size of the restatement is the same function
    for (Hs, Ws), _ in GEOMETRIES:
        assert RR.new_size(Hs, Ws, (1024, 1024), True) == pp.resized(Hs, Ws) or (Hs, Ws) == (2048, 2048)


def test_refusals_of_the_opt_in():
    from mmsa.preprocess import Preprocess
    base = RR.pipeline_of(RR.load_cfgs()["deliver_rgb_lidar"])
    with pytest.raises(ValueError, match="resize="):
        Preprocess.from_pipeline(base, resize="host")
    rs = base[1]
    assert rs["type"] == "Resize_multimodal"
    with pytest.raises(NotImplementedError, match="ratio range"):
        Preprocess.from_pipeline([base[0], dict(rs, ratio_range=(0.5, 2.0))] + base[2:], resize="device")
    with pytest.raises(NotImplementedError, match="several scales"):
        Preprocess.from_pipeline([base[0], dict(rs, img_scale=[(1024, 1024), (512, 512)])] + base[2:], resize="device")
    with pytest.raises(NotImplementedError, match="after Pad_multimodal"):
        Preprocess.from_pipeline([base[0], dict(type="Pad_multimodal", size=(1100, 1100), pad_val=0), rs] + base[2:], resize="device")
    with pytest.raises(NotImplementedError, match="twice"):
        Preprocess.from_pipeline([base[0], rs, rs] + base[2:], resize="device")
    with pytest.raises(NotImplementedError, match="after Pad_multimodal / the normalisation"):
        Preprocess.from_pipeline(base + [rs], resize="device")
    # exactly 2 x on both axes is OpenCV's area average: refused by name, by the object and by the restatement
    pp = Preprocess.from_pipeline(base, resize="device")
    with pytest.raises(NotImplementedError, match="INTER_AREA"):
        pp.canvas(2048, 2048)
    with pytest.raises(NotImplementedError, match="INTER_AREA"):
        RR.resize_u8(np.zeros((8, 6, 3), np.uint8), 4, 3)
    with pytest.raises(NotImplementedError, match="INTER_AREA"):
        pp.canvas(2048, 1024)                                                    # keep_ratio: (1024, 512), 2 x on both axes as well
    half = Preprocess(mean=[0] * 6, std=[1] * 6, to_rgb=[False, False], modalities_name=["rgb", "lidar"], modalities_ch=[3, 3],
                      resize=dict(img_scale=(512, 1024), keep_ratio=False), device_resize=True)
    assert half.canvas(2048, 2048) == (1024, 512)                                # 2 x on ONE axis only stays bilinear
    # sources other than uint8 / float32, and CPU tensors, stay refused
    z = torch.zeros(1, 1042, 1042, 3, dtype=torch.uint8)
    with pytest.raises(RuntimeError, match="GPU tensor"):
        pp(z, z)
    with pytest.raises(RuntimeError, match="GPU tensor"):
        pp.crops(z, z, [(0, (0, 0, 4, 4))], (4, 4))
    import mmsa.preprocess as P
    assert set(P._DT) == {torch.uint8, torch.float32}                            # check() refuses every other dtype by name (GPU test)


def test_the_new_entries_are_declared_bound_and_exported():
    import mmsa
    from tests.test_host_cpu import _header_prototypes
    protos = _header_prototypes()
    for name in NEW_ENTRIES:
        assert name in mmsa.lib.SIGNATURES and hasattr(mmsa.lib.raw, name) and name in protos
        kinds = ["P" if t in (ctypes.c_void_p,) else "I" for t in mmsa.lib.SIGNATURES[name]]
        assert kinds == protos[name][1] and protos[name][0] == "I"
    assert mmsa.lib.ABI_VERSION == mmsa.lib.version() >= 105
    # the old entries keep their argument lists; the new ones are old + (Hr, Wr, four tables, fixed_point)
    for old, new in (("mmsa_preprocess_nhwc", NEW_ENTRIES[0]), ("mmsa_preprocess_crops", NEW_ENTRIES[1])):
        o, n = mmsa.lib.SIGNATURES[old], mmsa.lib.SIGNATURES[new]
        assert n[:len(o) - 1] == o[:-1] and len(n) == len(o) + 7 and n[-1] == o[-1]
    # host-side argument errors (nothing is launched)
    one = (ctypes.c_float * 6)(*[1.0] * 6)
    two_i, two_f = (ctypes.c_int * 2)(0, 0), (ctypes.c_float * 2)(0, 0)
    fake = ctypes.c_void_p(4096)
    tabs = (fake, fake, fake, fake)
    with pytest.raises(RuntimeError, match="smaller than the 12 x 16 resized frame"):
        mmsa.lib.call(NEW_ENTRIES[0], fake, 0, fake, 0, 1, 16, 16, one, one, two_i, two_i, two_f, fake, 8, 16, 12, 16, *tabs, 1, None)
    with pytest.raises(RuntimeError, match="two uint8 sources"):
        mmsa.lib.call(NEW_ENTRIES[0], fake, 0, fake, 1, 1, 16, 16, one, one, two_i, two_i, two_f, fake, 16, 16, 12, 16, *tabs, 1, None)
    with pytest.raises(RuntimeError, match="null table"):
        mmsa.lib.call(NEW_ENTRIES[0], fake, 0, fake, 0, 1, 16, 16, one, one, two_i, two_i, two_f, fake, 16, 16, 12, 16, fake, None, fake, fake, 1, None)
    with pytest.raises(RuntimeError, match="dtypes"):
        mmsa.lib.call(NEW_ENTRIES[1], fake, 2, fake, 0, 1, 16, 16, one, one, two_i, two_i, two_f, 16, 16, (ctypes.c_int * 3)(0, 0, 0), 1, fake, 8, 8, 12, 16, *tabs, 0, None)
    with pytest.raises(RuntimeError, match="outside"):
        mmsa.lib.call(NEW_ENTRIES[1], fake, 0, fake, 0, 1, 16, 16, one, one, two_i, two_i, two_f, 16, 16, (ctypes.c_int * 3)(0, 10, 0), 1, fake, 8, 8, 12, 16, *tabs, 1, None)


@pytest.mark.parametrize("n_src,n_dst", [(1042, 1024), (1920, 1024), (1080, 576), (37, 64), (53, 41), (300, 517), (1042, 2084), (5, 5), (1024, 1024), (2, 7), (1, 4)])
def test_axis_tables(n_src, n_dst):
    from mmsa.preprocess import resize_axis_table
    s, a = resize_axis_table(n_src, n_dst, True)
    s2, w = resize_axis_table(n_src, n_dst, False)
    assert s.dtype == np.int32 and a.dtype == np.int16 and w.dtype == np.float32 and a.shape == w.shape == (n_dst, 2) and np.array_equal(s, s2)
    assert s.min() >= 0 and s.max() <= n_src - 1 and (np.diff(s) >= 0).all()
    tot = a.astype(np.int32).sum(1)
    assert set(tot.tolist()) <= {2047, 2048, 2049} and a.min() >= 0
    assert (w >= 0).all() and (w <= 1).all()
    if n_src == n_dst:
        assert np.array_equal(s, np.arange(n_dst)) and (a == np.array([2048, 0])).all() and (w == np.array([1, 0], np.float32)).all()
    # the package's tables are the restatement's, bit for bit (two independent writings of the same published rule)
    rs, rf = RR.axis_taps(n_src, n_dst)
    assert np.array_equal(s, rs) and a.tobytes() == RR.fixed_coefs(rf).tobytes() and w.tobytes() == RR.float_coefs(rf).tobytes()
    # the last tap never reads beyond the source: where s is the last pixel its weight is (1, 0)
    last = s == n_src - 1
    assert (a[last] == np.array([2048, 0])).all()


def test_tables_are_cached_and_not_built_during_a_capture(monkeypatch):
    from mmsa.preprocess import Preprocess
    pp = Preprocess(mean=[0] * 6, std=[1] * 6, to_rgb=[False, False], modalities_name=["rgb", "lidar"], modalities_ch=[3, 3],
                    resize=dict(img_scale=(7, 5), keep_ratio=False), device_resize=True)
    tabs = pp.resize_tables(10, 10, 5, 7, True, "cpu")
    assert [tuple(t.shape) for t in tabs] == [(7,), (7, 2), (5,), (5, 2)] and [t.dtype for t in tabs] == [torch.int32, torch.int16, torch.int32, torch.int16]
    assert pp.resize_tables(10, 10, 5, 7, True, "cpu") is tabs and len(pp._tables) == 1          # same geometry: the same tensors, nothing is built
    assert [t.dtype for t in pp.resize_tables(10, 10, 5, 7, False, "cpu")] == [torch.int32, torch.float32, torch.int32, torch.float32]
    import mmsa.preprocess as P
    assert P._capturing(torch.device("cpu")) is False
    monkeypatch.setattr(P, "_capturing", lambda device: True)                                    # as inside torch.cuda.graph(...)
    assert pp.resize_tables(10, 10, 5, 7, True, "cpu") is tabs                                   # known geometry: fine inside a capture
    with pytest.raises(RuntimeError, match="run one call with this geometry before capturing"):
        pp.resize_tables(12, 10, 5, 7, True, "cpu")


def _exact(img, nh, nw):
    """float64 bilinear value at align_corners=False positions, [H, W, C] -> [nh, nw, C]."""
    t = torch.from_numpy(img.astype(np.float64)).permute(2, 0, 1)[None]
    return torch.nn.functional.interpolate(t, size=(nh, nw), mode="bilinear", align_corners=False)[0].permute(1, 2, 0).numpy()


def u8_bound(Hs, Ws):
    """Largest |fixed-point result - exact bilinear value| in grey levels, derived from the formula for S in [0, 255]:
      positions     f is rounded to float32 from a coordinate below n_src: |df| <= n_src * 2^-24 per axis; a bilinear value moves by at most
                    255 * |df| per axis                                                          -> 255 * (Hs + Ws) * 2^-24
      a0, a1        each within 1/2 of (1 - f) * 2048, f * 2048: |D / 2048 - row value| <= 255 * (1/4096 + 1/4096)        -> 255 / 2048
      D >> 4        drops less than 16 / 2048 of a grey level, weights sum to at most 2049 / 2048          -> (1 / 128) * (2049 / 2048)
      b0, b1        as a0, a1, on values of at most 255 * 2049 / 2048                                     -> (255 / 2048) * (2049 / 2048)
      two >> 16     b * (D >> 4) is in units of 1 / (2048 * 128); >> 16 leaves quarters: less than 1/4 each               -> 1/2
      (+ 2) >> 2    rounding to the nearest integer                                                                        -> 1/2
    = 1.257 + 255 * (Hs + Ws) * 2^-24 (1.289 for 1042 x 1042).  Derived, not measured."""
    return 255 * (Hs + Ws) * 2.0 ** -24 + 255 / 2048 + (1 / 128) * (2049 / 2048) + (255 / 2048) * (2049 / 2048) + 0.5 + 0.5


def test_uint8_restatement_within_the_derived_bound_of_the_exact_bilinear_value():
    g = np.random.default_rng(42)
    worst = 0.0
    for (Hs, Ws), (nh, nw) in GEOMETRIES:
        img = g.integers(0, 256, (Hs, Ws, 3), dtype=np.uint8)
        img[: Hs // 3, : Ws // 3] = (g.integers(0, 2, (Hs // 3, Ws // 3, 3)) * 255).astype(np.uint8)      # full-swing steps: the largest gradients
        got = RR.resize_u8(img, nh, nw)
        assert got.dtype == np.uint8 and got.shape == (nh, nw, 3)
        err = np.abs(got.astype(np.float64) - _exact(img, nh, nw)).max()
        print(f"uint8 {Hs}x{Ws} -> {nh}x{nw}: largest deviation {err:.3f} grey levels (bound {u8_bound(Hs, Ws):.3f})")
        assert err <= u8_bound(Hs, Ws), f"{Hs}x{Ws} -> {nh}x{nw}: {err:.3f} beyond the derived bound {u8_bound(Hs, Ws):.3f}"
        worst = max(worst, err)
    assert worst > 0.4, "a fixed-point result that is closer than rounding allows compares the wrong things"
    for n in ((37, 53), (1042, 1042)):                                           # equal sizes: the identity, exactly
        img = g.integers(0, 256, n + (3,), dtype=np.uint8)
        assert np.array_equal(RR.resize_u8(img, *n), img)
        assert np.array_equal(RR.resize_f32(img, *n), img.astype(np.float32))


def test_float32_restatement_within_the_derived_bound_of_the_float64_value():
    """Two comparisons.  (1) Against the float64 value at the restatement's OWN float32 positions: a value passes through at most 6 roundings of
    relative size u = 2^-24 (the coefficient 1 - f, a product, a sum, the row coefficient, a product, a sum), every intermediate is bounded by
    M = the largest |tap|, so |error| <= ((1 + u)^6 - 1) * M < 7 u M.  (2) Against torch's float64 interpolate, whose positions are exact: on top
    of (1) the float32 rounding of f (|df| <= n_src * u per axis) moves a bilinear value by at most |df| * (largest tap difference <= 2 M) per
    axis -> 7 u M + 2 (Hs + Ws) u M.  Derived, not measured."""
    g = np.random.default_rng(43)
    u = 2.0 ** -24
    for (Hs, Ws), (nh, nw) in GEOMETRIES:
        img = g.normal(0, 100, (Hs, Ws, 3)).astype(np.float32)
        got = RR.resize_f32(img, nh, nw).astype(np.float64)
        ys, fy = RR.axis_taps(Hs, nh)
        xs, fx = RR.axis_taps(Ws, nw)
        y1, x1 = np.minimum(ys + 1, Hs - 1), np.minimum(xs + 1, Ws - 1)
        S, fx64, fy64 = img.astype(np.float64), fx.astype(np.float64)[None, :, None], fy.astype(np.float64)[:, None, None]
        taps = [S[ys][:, xs], S[ys][:, x1], S[y1][:, xs], S[y1][:, x1]]
        own = (taps[0] * (1 - fx64) + taps[1] * fx64) * (1 - fy64) + (taps[2] * (1 - fx64) + taps[3] * fx64) * fy64
        M = np.max(np.abs(np.stack(taps)), 0)
        e1 = np.abs(got - own)
        assert (e1 <= 7 * u * M).all(), f"{Hs}x{Ws} -> {nh}x{nw}: {(e1 / (u * M + 1e-300)).max():.2f} u M at its own positions"
        e2, Mg = np.abs(got - _exact(img, nh, nw)), float(np.abs(img).max())      # (2) with M = the largest |pixel| of the frame: a moved position may change taps
        assert (e2 <= (7 + 2 * (Hs + Ws)) * u * Mg).all(), f"{Hs}x{Ws} -> {nh}x{nw}: {e2.max() / (u * Mg):.1f} u M against exact positions"
        print(f"float32 {Hs}x{Ws} -> {nh}x{nw}: {(e1 / (u * M + 1e-300)).max():.2f} u M at own positions, {e2.max() / (u * Mg):.1f} u M(frame) at exact positions")
    # a mixed pair runs BOTH modalities in float32, the uint8 one converted exactly
    rgb, aux = g.integers(0, 256, (1, 37, 53, 3), dtype=np.uint8), g.normal(0, 50, (1, 37, 53, 3)).astype(np.float32)
    r, a = RR.resize_pair(rgb, aux, 64, 41)
    assert r.dtype == a.dtype == np.float32 and np.array_equal(r, RR.resize_f32(rgb.astype(np.float32), 64, 41))
    r8, a8 = RR.resize_pair(rgb, rgb, 64, 41)
    assert r8.dtype == np.uint8 and not np.array_equal(r8.astype(np.float32), r), "fixed point and float32 are two functions"
    # the whole-pipeline helper composes resize -> pad -> normalise
    cfg = RR.load_cfgs()["resize_then_pad"]
    big = g.integers(0, 256, (1, 60, 80, 3), dtype=np.uint8)
    out = RR.pipeline_ref(big, big, dict(img_scale=(64, 48), keep_ratio=False), cfg["mean"], cfg["std"], cfg["to_rgb"], cfg["modalities_name"], True, "multimodal",
                          pad_size=(52, 68))
    want = PR.normalize_ref(RR.resize_u8(big, 48, 64), RR.resize_u8(big, 48, 64), cfg["mean"], cfg["std"], cfg["to_rgb"], cfg["modalities_name"], True, "multimodal",
                            pad_size=(52, 68))
    assert out.shape == (1, 6, 52, 68) and np.array_equal(out, want)
