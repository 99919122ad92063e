"""The arithmetic of the rendered picture, without a GPU: the numpy restatement (tests/render_ref.py) against integer and rational arithmetic, the
de-normalise round trip, and the library boundary."""
from fractions import Fraction

import numpy as np
import pytest

from tests import preprocess_ref as PR
from tests import render_ref as RR

# RGB statistics typed in from the configs (configs/DELIVER/..._RGBLIDAR.py: Normalize_multimodal; configs/MUSES/..._RGBLIDAR.py: Normalize_multimodal_Muses)
DELIVER = dict(mean=[0.485, 0.456, 0.406, 0, 0, 0], std=[0.229, 0.224, 0.225, 1, 1, 1], to_rgb=[True, True], norm_by_max=True, variant="multimodal",
               names=["rgb", "lidar"])
MUSES = dict(mean=[0.485, 0.456, 0.406, 1.4628459, 1.8271197, 0.07808967], std=[0.229, 0.224, 0.225, 7.55678107, 9.85001751, 0.67012253],
             to_rgb=[True, False], norm_by_max=True, variant="muses", names=["rgb", "lidar"])


def _pairs(opacity):
    """The restatement over all 256 x 256 (image value, colour value) pairs: [256, 256], row = image value, column = colour value."""
    img = np.repeat(np.arange(256, dtype=np.uint8)[:, None, None], 256, 1).repeat(3, 2)
    seg = np.repeat(np.arange(256, dtype=np.uint8)[None], 256, 0)
    pal = np.repeat(np.arange(256)[:, None], 3, 1)
    out = RR.show_result_ref(img, seg, pal, opacity)
    assert np.array_equal(out[..., 0], out[..., 1]) and np.array_equal(out[..., 0], out[..., 2])
    return out[..., 0].astype(np.int64)


@pytest.mark.parametrize("num,den", ((1, 2), (1, 4), (1, 1)))
def test_dyadic_opacities_are_the_integer_identity(num, den):
    """With opacity 0.5, 0.25 and 1.0 every float64 step is exact: the picture is (img * (den - num) + colour * num) // den."""
    i, c = np.meshgrid(np.arange(256), np.arange(256), indexing="ij")
    assert np.array_equal(_pairs(num / den), (i * (den - num) + c * num) // den)


def _three_roundings(opacity):
    op, om = Fraction(opacity), Fraction(1 - opacity)          # the doubles the reference multiplies by, exactly
    out = np.empty((256, 256), dtype=np.int64)
    for i in range(256):
        a = Fraction(float(i * om))                            # float(): the correctly rounded double of the exact product
        for c in range(256):
            out[i, c] = int(float(a + Fraction(float(c * op))))
    return out


@pytest.mark.parametrize("opacity", (0.3, 0.7))
def test_non_dyadic_opacities_round_three_times(opacity):
    """The restatement equals rational arithmetic with the two products and the sum each rounded to double, on all pairs."""
    assert np.array_equal(_pairs(opacity), _three_roundings(opacity))


def test_the_pairs_tell_a_contracted_blend_from_the_right_one():
    """At opacity 0.3 some pairs have an integer exact result (img * 7 + colour * 3 divisible by 10) that the three roundings land just below: the
    truncation takes them one level down.  A float32, fused or exact blend gives the upper value there, so the exhaustive image of the GPU test can
    tell them apart.  Of the 6556 pairs with an integer exact result, 1271 land below it (measured with numpy; the property the test needs is
    that there is at least one)."""
    i, c = np.meshgrid(np.arange(256), np.arange(256), indexing="ij")
    exact = (i * 7 + c * 3) // 10
    got = _pairs(0.3)
    differ = got != exact
    print("pairs at opacity 0.3 below the exact floor:", int(differ.sum()))
    assert differ.any()
    assert np.array_equal(got[differ], exact[differ] - 1) and ((i * 7 + c * 3)[differ] % 10 == 0).all()
    assert int(differ.sum()) == 1271 and int(((i * 7 + c * 3) % 10 == 0).sum()) == 6556


@pytest.mark.parametrize("cfg,lost", ((DELIVER, (66, 36, 42)), (MUSES, (66, 36, 42))), ids=("deliver", "muses"))
def test_denormalise_round_trip(cfg, lost):
    """tensor2imgs of the normalised tensor against the raw frame, all 256 values per channel: within one level, and the number of values that lose a
    level (the documented difference between the `raw` and the `tensor` source): 66 / 36 / 42 of 256 for the tensor's planes 0 / 1 / 2 with the ImageNet
    statistics in 0..1 form."""
    v = np.arange(256, dtype=np.uint8)
    rgb = np.repeat(v[None, None, :, None], 3, 3)              # [1, 1, 256, 3]: value v in every channel
    x = PR.normalize_ref(rgb, rgb, cfg["mean"], cfg["std"], cfg["to_rgb"], cfg["names"], cfg["norm_by_max"], cfg["variant"])
    pic = RR.tensor2imgs_ref(x, cfg["mean"], cfg["std"], cfg["to_rgb"][0], norm_by_max=cfg["norm_by_max"])
    d = pic[0, 0].astype(np.int64) - rgb[0, 0].astype(np.int64)        # [256, 3] in the frame's channel order
    assert np.abs(d).max() <= 1
    assert d.max() <= 0                                                # truncation never gains a level here
    planes = d[:, ::-1] if cfg["to_rgb"][0] else d                     # per tensor plane (mean / std order)
    print("values losing a level per plane:", (planes == -1).sum(0))
    assert tuple(int(n) for n in (planes == -1).sum(0)) == lost


def test_saturation_and_missing_palette_entries():
    assert RR.to_u8(np.array([-3.5, -0.5, 0.0, 0.99, 254.99, 255.0, 255.9, 256.0, 1e9, np.nan], dtype=np.float32)).tolist() == [0, 0, 0, 0, 254, 255, 255, 255, 255, 0]
    seg = np.array([[0, 1, 2, 255]], dtype=np.uint8)
    out = RR.show_result_ref(np.full((1, 4, 3), 100, np.uint8), seg, [[10, 20, 30], [40, 50, 60]], 0.5)
    assert out.tolist() == [[[65, 60, 55], [80, 75, 70], [50, 50, 50], [50, 50, 50]]]      # BGR; classes 2 and 255 have no entry: colour 0


def test_boundary():
    import mmsa
    assert mmsa.lib.version() == mmsa.lib.ABI_VERSION >= 107
    for name in ("mmsa_render_u8", "mmsa_render_denorm_f32"):
        assert name in mmsa.lib.SIGNATURES and hasattr(mmsa.lib.raw, name)
    assert mmsa.Renderer is mmsa.render.Renderer
    with pytest.raises(ValueError, match="1..256 entries, got 257"):
        mmsa.Renderer(np.zeros((257, 3), dtype=np.int64))
    with pytest.raises(ValueError, match="palette is required"):
        mmsa.Renderer(None)
    for bad in (0, 1.5):
        with pytest.raises(ValueError, match=r"must be in \(0, 1\]"):
            mmsa.Renderer([[0, 0, 0]], opacity=bad)
    r = mmsa.Renderer([[1, 2, 3]], opacity=0.3)
    assert r.one_minus == 1 - 0.3 and int(r.packed[0]) == 1 | 2 << 8 | 3 << 16
