"""Host side of mmsa.preprocess (no GPU): the parameters read from the reference's test pipelines, the refusals, the C boundary of the two new
entries, and the float32 restatement the GPU tests compare against (tests/preprocess_ref.py) held to a derived bound of the float64 formula."""
import os
import re

import numpy as np
import pytest
import torch

from tests import preprocess_ref as PR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_ENTRIES = ("mmsa_preprocess_nhwc", "mmsa_preprocess_crops")


@pytest.mark.parametrize("name", ["muses_rgb_lidar", "muses_rgb_event", "deliver_rgb_lidar", "fmb_rgb_therm"])
def test_from_pipeline_reads_the_reference_settings(name):
    from mmsa.preprocess import Preprocess
    cfg = PR.load_cfgs()[name]
    pp = Preprocess.from_pipeline(PR.pipeline_of(cfg))
    assert pp.variant == ("muses" if cfg["normalize"].endswith("_Muses") else "multimodal")
    assert pp.mean.dtype == np.float32 and pp.mean.tobytes() == np.array(cfg["mean"], dtype=np.float32).tobytes()
    want = np.float32(1) * (1 / np.float64(np.array(cfg["std"], dtype=np.float32))).astype(np.float32)
    assert pp.sinv.dtype == np.float32 and pp.sinv.tobytes() == want.tobytes(), "sinv must be float32(1 / float64(float32(std))) bit for bit"
    assert pp.to_rgb == cfg["to_rgb"] and pp.norm_by_max is True
    assert pp.div255 == ([True, False] if pp.variant == "muses" else [True, True])
    assert pp.pad_size == (None if cfg["pad_size"] is None else tuple(cfg["pad_size"])) and pp.pad_val == [0.0, 0.0]
    Hs, Ws = cfg["frame"]
    assert pp.canvas(Hs, Ws) == (tuple(cfg["pad_size"]) if cfg["pad_size"] else (Hs, Ws))
    # the launch arguments are those values
    assert list(pp._c_mean) == pp.mean.tolist() and list(pp._c_sinv) == pp.sinv.tolist()
    assert list(pp._c_div) == [int(v) for v in pp.div255] and list(pp._c_swap) == [int(v) for v in cfg["to_rgb"]]


def test_variants_differ_only_in_what_norm_by_max_divides():
    from mmsa.preprocess import Preprocess
    kw = dict(mean=[0] * 6, std=[1] * 6, to_rgb=[True, False], modalities_ch=[3, 3])
    assert Preprocess(modalities_name=["rgb", "lidar"], norm_by_max=True, variant="multimodal", **kw).div255 == [True, True]
    assert Preprocess(modalities_name=["rgb", "lidar"], norm_by_max=True, variant="muses", **kw).div255 == [True, False]
    assert Preprocess(modalities_name=["lidar", "rgb"], norm_by_max=True, variant="muses", **kw).div255 == [False, True]
    for v in ("multimodal", "muses"):
        assert Preprocess(modalities_name=["rgb", "lidar"], norm_by_max=False, variant=v, **kw).div255 == [False, False]


def test_refusals():
    from mmsa.preprocess import Preprocess
    cfgs = PR.load_cfgs()
    good = dict(mean=[0.5] * 6, std=[0.25] * 6, to_rgb=[True, False], modalities_name=["rgb", "lidar"], modalities_ch=[3, 3])
    Preprocess(**good)
    for bad in (dict(std=[0.25, 0, 0.25, 1, 1, 1]), dict(std=[0.25, float("inf"), 0.25, 1, 1, 1]), dict(std=[0.25, float("nan"), 0.25, 1, 1, 1]),
                dict(std=[1e-42] * 6),                                  # 1 / std overflows float32
                dict(modalities_ch=[3, 1]), dict(modalities_ch=[3, 3, 3], modalities_name=["rgb", "a", "b"]), dict(mean=[0.5] * 5),
                dict(variant="deliver"), dict(mean=[float("nan")] * 6)):
        with pytest.raises(ValueError):
            Preprocess(**dict(good, **bad))
    # pipeline steps without a device form are refused BY NAME
    base = PR.pipeline_of(cfgs["muses_rgb_lidar"])
    for extra, name in ((dict(type="RandomFlip", prob=0.5), "RandomFlip"), (dict(type="PhotoMetricDistortion_multimodal"), "PhotoMetricDistortion_multimodal"),
                        (dict(type="CropRect", box_crop=(0, 0, 10, 10)), "CropRect")):
        with pytest.raises(NotImplementedError, match=name):
            Preprocess.from_pipeline(base[:1] + [extra] + base[1:])
    msfa = base[-1]
    with pytest.raises(NotImplementedError, match="flip"):
        Preprocess.from_pipeline(base[:1] + [dict(msfa, flip=True)])
    with pytest.raises(NotImplementedError, match="scales"):
        Preprocess.from_pipeline(base[:1] + [dict(msfa, img_scale=[(1920, 1080), (960, 540)])])
    with pytest.raises(NotImplementedError, match="img_ratios"):
        Preprocess.from_pipeline(base[:1] + [dict(msfa, img_ratios=[0.5, 1.0])])
    with pytest.raises(NotImplementedError, match="Normalize"):
        Preprocess.from_pipeline(base[:1])
    with pytest.raises(NotImplementedError, match="after the normalisation"):       # the training order: pad AFTER normalising = zeros, another function
        Preprocess.from_pipeline(base + [dict(type="Pad_multimodal", size=(1024, 1024), pad_val=0)])
    with pytest.raises(NotImplementedError, match="size_divisor"):
        Preprocess.from_pipeline([dict(type="Pad_multimodal", size_divisor=32)] + base)
    with pytest.raises(NotImplementedError, match="ratio range"):
        Preprocess.from_pipeline(base[:1] + [dict(type="Resize_multimodal", img_scale=(1920, 1080), ratio_range=(0.5, 2.0))] + base[1:])
    # Resize_multimodal: accepted, and the identity is checked against the source size per call
    pp = Preprocess.from_pipeline(PR.pipeline_of(cfgs["deliver_rgb_lidar"]))
    assert pp.canvas(1024, 1024) == (1024, 1024)
    with pytest.raises(NotImplementedError, match="only the identity"):
        pp.canvas(1042, 1042)                                                        # DELIVER's native size: that resize is the OpenCV one
    with pytest.raises(NotImplementedError, match="only the identity"):
        pp.canvas(2048, 1024)
    assert pp.canvas(512, 1024) == (512, 1024)                                   # keep_ratio: already inside the scale, factor 1
    fixed = Preprocess.from_pipeline(base[:1] + [dict(type="Resize_multimodal", img_scale=(1920, 1080), keep_ratio=False)] + base[1:])
    assert fixed.canvas(1080, 1920) == (1080, 1920)
    with pytest.raises(NotImplementedError):
        fixed.canvas(1920, 1080)
    # padding only grows a frame
    fmb = Preprocess.from_pipeline(PR.pipeline_of(cfgs["fmb_rgb_therm"]))
    assert fmb.canvas(600, 800) == (800, 800)
    with pytest.raises(RuntimeError, match="smaller"):
        fmb.canvas(900, 800)
    # no CPU path
    z = torch.zeros(1, 8, 8, 3, dtype=torch.uint8)
    with pytest.raises(RuntimeError, match="GPU tensor"):
        fmb(z, z)
    with pytest.raises(RuntimeError, match="GPU tensor"):
        fmb.crops(z, z, [(0, (0, 0, 4, 4))], (4, 4))


def test_the_two_entries_are_declared_bound_and_exported():
    """Fails on a tree without the feature; tests/test_host_cpu.py's header / table comparison covers the argument kinds of the new rows."""
    import ctypes
    import mmsa
    from tests.test_host_cpu import _header_prototypes
    protos = _header_prototypes()
    for name in NEW_ENTRIES:
        assert name in mmsa.lib.SIGNATURES and hasattr(mmsa.lib.raw, name) and name in protos
        kinds = ["P" if t in (ctypes.c_void_p,) else "I" for t in mmsa.lib.SIGNATURES[name]]
        assert kinds == protos[name][1] and protos[name][0] == "I"
    assert mmsa.lib.ABI_VERSION == mmsa.lib.version() >= 104
    hdr = open(os.path.join(ROOT, "include", "mmsa.h")).read()
    assert re.search(r"enum \{ MMSA_PRE_U8 = 0, MMSA_PRE_F32 = 1 \}", hdr)
    assert mmsa.preprocess._DT == {torch.uint8: 0, torch.float32: 1}
    src = re.sub(r"//[^\n]*", "", open(os.path.join(ROOT, "multimodal-sam-adapter_amd", "csrc", "preprocess.hip")).read())      # code, without the comments
    assert src.count("/ 255") == 1 and src.count("__global__") == 1 and "pre_norm(" in src, "one device function holds the arithmetic of both entries"
    # host-side argument errors come back through mmsa_last_error() (no GPU needed: nothing is launched)
    one = (ctypes.c_float * 6)(*[1.0] * 6)
    two_i, two_f = (ctypes.c_int * 2)(0, 0), (ctypes.c_float * 2)(0, 0)
    fake = ctypes.c_void_p(4096)
    with pytest.raises(RuntimeError, match="smaller than"):
        mmsa.lib.call("mmsa_preprocess_nhwc", fake, 0, fake, 0, 1, 16, 16, one, one, two_i, two_i, two_f, fake, 8, 16, None)
    with pytest.raises(RuntimeError, match="dtypes"):
        mmsa.lib.call("mmsa_preprocess_nhwc", fake, 2, fake, 0, 1, 16, 16, one, one, two_i, two_i, two_f, fake, 16, 16, None)
    tab = (ctypes.c_int * 3)(0, 10, 0)
    with pytest.raises(RuntimeError, match="outside"):
        mmsa.lib.call("mmsa_preprocess_crops", fake, 0, fake, 0, 1, 16, 16, one, one, two_i, two_i, two_f, 16, 16, tab, 1, fake, 8, 8, None)
    with pytest.raises(RuntimeError, match="windows per call"):
        mmsa.lib.call("mmsa_preprocess_crops", fake, 0, fake, 0, 1, 16, 16, one, one, two_i, two_i, two_f, 16, 16, tab, 65, fake, 8, 8, None)


def _bound_check(x32, mean, std, div):
    """|restatement - float64 formula| <= 2^-23 * ((|a| + |a - m|) * |s| + |y|) per element, with a = x / 255 (or x), m = float32 mean, s = 1 / float32
    std, y = (a - m) * s, all in float64.  Derivation: the restatement rounds three times (a, a - m, the product; relative error <= 2^-24 each) and
    uses sinv = float32(s) (one more 2^-24): |dy| <= 2^-24 * (|a||s| + |a - m||s| + 2|y|) to first order, which the bound above doubles for the
    first two terms -- that slack covers the second-order terms.  Derived, not measured."""
    m32, s32 = np.float32(mean), PR.sinv_of([std])[0]
    a32 = x32 / np.float32(255) if div else x32
    got = (a32 - m32) * s32
    assert got.dtype == np.float32
    x = x32.astype(np.float64)
    a = x / 255.0 if div else x
    m, s = np.float64(m32), 1.0 / np.float64(np.float32(std))
    y = (a - m) * s
    bound = 2.0 ** -23 * ((np.abs(a) + np.abs(a - m)) * abs(s) + np.abs(y))
    err = np.abs(got.astype(np.float64) - y)
    assert (err <= bound).all(), f"mean {mean} std {std}: error {err.max():.3e} beyond the bound {bound[err.argmax()]:.3e}"
    return err.max(), np.abs(y).max()


def test_float32_restatement_within_the_derived_bound_of_the_float64_formula():
    cfgs = PR.load_cfgs()
    bytes32 = np.arange(256, dtype=np.float32)
    g = np.random.default_rng(7)
    floats = np.concatenate([g.normal(0, 100, 4096), g.uniform(-3, 260, 4096), [0.0, 1e-3, 254.5, 1e4]]).astype(np.float32)
    for name, cfg in cfgs.items():
        variant = "muses" if cfg["normalize"].endswith("_Muses") else "multimodal"
        div = PR.div255_of(variant, cfg["norm_by_max"], cfg["modalities_name"])
        worst = 0.0
        for c in range(6):
            for xs in (bytes32, floats):
                e, _ = _bound_check(xs, cfg["mean"][c], cfg["std"][c], div[c // 3])
                worst = max(worst, e)
        print(f"{name}: largest deviation from the float64 formula {worst:.2e}")
    # the whole-frame helper is the same arithmetic: channel order, reversal and padding
    cfg = cfgs["fmb_rgb_therm"]
    rgb = g.integers(0, 256, (2, 5, 7, 3), dtype=np.uint8)
    aux = g.normal(0, 50, (2, 5, 7, 3)).astype(np.float32)
    out = PR.normalize_ref(rgb, aux, cfg["mean"], cfg["std"], [True, False], cfg["modalities_name"], True, "multimodal", pad_size=(8, 9), pad_val=0)
    assert out.shape == (2, 6, 8, 9) and out.dtype == np.float32
    m32, s32 = np.array(cfg["mean"], dtype=np.float32), PR.sinv_of(cfg["std"])
    for c in range(3):
        assert np.array_equal(out[:, c, :5, :7], (rgb[..., 2 - c].astype(np.float32) / np.float32(255) - m32[c]) * s32[c])            # to_rgb reverses
        assert np.array_equal(out[:, 3 + c, :5, :7], (aux[..., c] / np.float32(255) - m32[3 + c]) * s32[3 + c])
        pad = (np.float32(0) / np.float32(255) - m32[c]) * s32[c]
        assert pad != 0 and (out[:, c, 5:, :] == pad).all() and (out[:, c, :, 7:] == pad).all(), "a padded pixel is the NORMALISED pad value"
    # 1 / 255 as a multiplication is another function (why the kernel divides)
    lidar = cfgs["muses_rgb_lidar"]
    diff = sum(int(((bytes32 / np.float32(255) - np.float32(lidar["mean"][c])) * PR.sinv_of(lidar["std"])[c]
                    != (bytes32 * np.float32(1 / 255.0) - np.float32(lidar["mean"][c])) * PR.sinv_of(lidar["std"])[c]).sum()) for c in range(6))
    assert diff > 0
