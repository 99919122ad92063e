"""The guided vote filter without a GPU: the restatement (tests/vote_filter_ref.py) against the brute-force version and, with unit weights, against the majority
filter's restatement; the range table against exact rounding; the weight quantisation against integer arithmetic; every argument refusal that needs no device,
the C entry's checks on the host, header / ctypes table / version; and the property the filter is built for, on the restatement alone."""
import ctypes
import inspect
import math
import os
import re
from decimal import Decimal, getcontext
from fractions import Fraction

import numpy as np
import pytest
import torch

from tests import majority_ref as MR
from tests import vote_filter_ref as VR

import mmsa.evaluate as E  # noqa: E402  (what this file is about)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY = "mmsa_vote_filter_u8"


def _equal(got, want, what):
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), what


# ---- 1. the restatement against brute force

def test_the_restatement_equals_brute_force_on_small_maps():
    rng = np.random.default_rng(11)
    changed = zero_total = 0
    for trial in range(96):
        H, W = (int(v) for v in rng.integers(1, 11, size=2))
        m = MR.noise(H, W, 500 + trial, (2, 3, 25)[trial % 3], 0.15, 0.1)
        r = int(rng.integers(1, 4))
        role = MR.roles(**MR.CONFIGS[("any", "C25")[trial % 2]])
        where, half = MR.MODES[trial % 4]
        G = (1, 3, 0)[(trial // 4) % 3]
        guide = VR.guide_of(m[None], G, (2, 1), trial)[0] if G else None
        lut = None if not G else (VR.range_table(8.0, G), VR.cut_table(G, 12))[(trial // 12) % 2]      # the second one has zeros
        wq = VR.wq_of(VR.weights_of((H, W), trial)) if (trial // 2) % 2 else None
        got = VR.vote(m, role, r, where == "all", half, guide, lut, wq)
        _equal(got, VR.brute(m, role, r, where == "all", half, guide, lut, wq), (trial, m.tolist(), r, where, half, G))
        changed += int((got[0] != m).any())
        vt = VR.sums(m, role, r, guide, lut, wq)
        zero_total += int(((vt.total == 0) & (MR.box(role[m] == MR.VOTER, r) > 0)).any())
    assert changed > 40 and zero_total > 5, (changed, zero_total)      # and T = 0 with voters in the window is met


def test_bands_equal_the_whole():
    m = MR.patchy(90, 70, 3)
    role = MR.roles(**MR.CONFIGS["C25"])
    guide, wq = VR.guide_of(m[None], 3, (0, 0), 1)[0], VR.wq_of(VR.weights_of(m.shape, 2))
    whole = VR.sums(m, role, 4, guide, VR.range_table(8.0, 3), wq)
    bands = VR.sums(m, role, 4, guide, VR.range_table(8.0, 3), wq, cells=20 * 70 * 27)
    for a, b in zip(whole, bands):
        assert np.array_equal(a, b)


# ---- 2. unit weights: the majority filter

def test_unit_weights_equal_the_majority_restatement():
    names = [c.name for c in MR.CASES if MR.maps_of(c.name)[0].size <= 3 * 200 and c.radius <= VR.MAX_RADIUS]
    assert len(names) >= 12
    for name in names:
        role, r, maps = MR.role_of(name), MR.CASE[name].radius, MR.maps_of(name)
        guide = VR.guide_of(maps, 3, (1, 2), 5)
        for b, m in enumerate(maps):
            plain, ones = VR.sums(m, role, r), VR.sums(m, role, r, guide[b], np.ones(766, dtype=np.uint16))
            for where, half in MR.MODES:
                want = (MR.want_of(name, where, half)[0][b], MR.want_of(name, where, half)[1][b])
                for vt in (plain, ones):
                    got = VR.apply(m, role, vt, where == "all", half)
                    assert got[1].dtype == np.uint32
                    _equal(got, want, (name, b, where, half))


# ---- 3. the range table

def test_the_range_table():
    getcontext().prec = 60
    for sigma, ch in ((8.0, 3), (8.0, 1), (0.5, 1), (3.25, 3), (100.0, 1), (1000.0, 3), (2, 1)):
        t = E.vote_range_table(sigma, ch)
        assert t.dtype == np.uint16 and t.shape == (255 * ch + 1,) and t[0] == 256 and (np.diff(t.astype(np.int64)) <= 0).all() and t.max() <= VR.MAX_WEIGHT
        assert np.array_equal(t, VR.range_table(float(sigma), ch))
        s = Fraction(float(sigma))
        for d in (0, 1, 2, 5, 9, 17, 40, 100, 255 * ch):
            x = Fraction(-d * d) / (2 * s * s)
            exact = Decimal(256) * (Decimal(x.numerator) / Decimal(x.denominator)).exp() + Decimal("0.5")
            if abs(exact - exact.to_integral_value()) > Decimal("1e-9"):      # float64 cannot decide a value this close to a step; none of these is
                assert int(t[d]) == math.floor(exact), (sigma, d)
    assert E.vote_range_table(8.0).shape == (766,) and list(inspect.signature(E.vote_range_table).parameters) == ["sigma", "channels"]
    for bad in (0, -1.0, float("nan"), float("inf"), None, "8", True):
        with pytest.raises(ValueError, match="sigma = "):
            E.vote_range_table(bad)
    for bad in (0, 2, 4, 1.0, None):
        with pytest.raises(ValueError, match="channels = "):
            E.vote_range_table(8.0, bad)


# ---- 4. the weight quantisation

def test_the_weight_quantisation_against_integer_arithmetic():
    f32 = np.float32
    edges = np.arange(0, 257, dtype=np.float32) / f32(256)
    ws = np.concatenate([edges, np.nextafter(edges, f32(-1)), np.nextafter(edges, f32(2)), VR.SPECIAL_WEIGHTS,
                         np.array([1e-45, 1.1754942e-38, 1.1754944e-38, 3.4e38, -3.4e38, 0.00390624, 0.9999999], dtype=np.float32)])
    got = VR.wq_of(ws)
    for w, q in zip(ws.tolist(), got.tolist()):
        if w != w or w <= 0:
            want = 0
        elif w >= 1:
            want = 255
        else:
            want = min(255, int(Fraction(w) * 256))      # exact: w is the float32's own value
        assert q == want, (w, q, want)
    assert got[:257].tolist() == list(range(256)) + [255]                                     # k / 256 itself gives k
    assert got[258:514].tolist() == list(range(255)) + [255]                                  # one ulp below k / 256 gives k - 1 (k = 1 .. 256)
    assert got[257] == 0 and got[514:771].tolist() == list(range(256)) + [255]                # one ulp above gives k


# ---- 5. refusals that need no device

def test_python_refusals():
    import mmsa
    m = torch.zeros(2, 6, 8, dtype=torch.uint8)
    g3, g1 = torch.zeros(2, 7, 9, 3, dtype=torch.uint8), torch.zeros(2, 6, 8, dtype=torch.uint8)
    for bad in (0, 17, 32, -1, 2.0, None, True, "1"):
        with pytest.raises(ValueError, match="radius = .*an int in 1..16"):
            mmsa.vote_filter(m, bad)
    with pytest.raises(ValueError, match="hole = "):
        mmsa.vote_filter(m, hole=300)
    with pytest.raises(ValueError, match="inert = "):
        mmsa.vote_filter(m, inert="254")
    with pytest.raises(ValueError, match=r"hole and inert share the bytes \[254\]"):
        mmsa.vote_filter(m, hole=[254, 255], inert=254)
    with pytest.raises(ValueError, match=r"hole holds the bytes \[3\], which are among the 5 classes"):
        mmsa.vote_filter(m, num_classes=5, hole=[3, 255])
    with pytest.raises(ValueError, match="num_classes = "):
        mmsa.vote_filter(m, num_classes=257)
    with pytest.raises(ValueError, match='where = "holes" and hole is empty'):
        mmsa.vote_filter(m, where="holes")
    with pytest.raises(ValueError, match="where = "):
        mmsa.vote_filter(m, hole=255, where="some")
    with pytest.raises(ValueError, match="half = "):
        mmsa.vote_filter(m, half=1)
    # the guide and its table
    for kw in (dict(sigma=8.0), dict(range_weights=np.ones(766)), dict(sigma=8.0, range_weights=np.ones(766))):
        with pytest.raises(ValueError, match="without guide= neither is taken"):
            mmsa.vote_filter(m, **kw)
    for kw in (dict(), dict(sigma=8.0, range_weights=np.ones(766, dtype=np.uint16))):
        with pytest.raises(ValueError, match="a guide takes sigma= .* or range_weights= .*exactly one of them"):
            mmsa.vote_filter(m, guide=g3, **kw)
    for bad in (0, -2.0, float("nan"), "8", True):
        with pytest.raises(ValueError, match="sigma = "):
            mmsa.vote_filter(m, guide=g3, sigma=bad)
    with pytest.raises(RuntimeError, match="guide must be a tensor"):
        mmsa.vote_filter(m, guide=g3.numpy(), sigma=8.0)
    with pytest.raises(RuntimeError, match="guide is torch.float32; the raw uint8 frame"):
        mmsa.vote_filter(m, guide=g3.float(), sigma=8.0)
    for bad in (torch.zeros(2, 7, 9, 2, dtype=torch.uint8), torch.zeros(2, 7, 9, 4, dtype=torch.uint8), torch.zeros(7, 9, dtype=torch.uint8),
                torch.zeros(2, 7, 18, 3, dtype=torch.uint8)[:, :, ::2]):
        with pytest.raises(RuntimeError, match=r"guide must be a contiguous \[B, Hg, Wg, 3\], \[B, Hg, Wg, 1\] or \[B, Hg, Wg\] tensor"):
            mmsa.vote_filter(m, guide=bad, sigma=8.0)
    for bad in (torch.zeros(1, 7, 9, 3, dtype=torch.uint8), torch.zeros(2, 5, 9, 3, dtype=torch.uint8), torch.zeros(2, 6, 7, dtype=torch.uint8)):
        with pytest.raises(RuntimeError, match=r"guide has shape .*the map is \[B, H, W\] = \(2, 6, 8\)"):
            mmsa.vote_filter(m, guide=bad, sigma=8.0)
    for bad, msg in ((np.ones(256), "range_weights has 256 entries; a guide of 3 channels has L1 differences 0..765, so 766 are expected"),
                     (np.ones((2, 383)), "range_weights must be a one-dimensional array of 766 integers in 0..4096"),
                     ("table", "range_weights must be a one-dimensional array"),
                     (np.full(766, 0.5), "range_weights holds values that are not integers"),
                     (np.full(766, np.nan), "range_weights holds values that are not integers"),
                     (np.full(766, 4097), "range_weights holds values outside 0..4096"),
                     (np.full(766, -1), "range_weights holds values outside 0..4096")):
        with pytest.raises(ValueError, match=re.escape(msg)):
            mmsa.vote_filter(m, guide=g3, range_weights=bad)
    with pytest.raises(ValueError, match="range_weights has 766 entries; a guide of 1 channel has L1 differences 0..255, so 256 are expected"):
        mmsa.vote_filter(m, guide=g1, range_weights=np.ones(766))
    # the weights
    with pytest.raises(RuntimeError, match="weights is torch.float64; a float32 confidence map"):
        mmsa.vote_filter(m, weights=torch.zeros(2, 6, 8, dtype=torch.float64))
    with pytest.raises(RuntimeError, match=r"weights has shape \(2, 6, 9\)"):
        mmsa.vote_filter(m, weights=torch.zeros(2, 6, 9))
    with pytest.raises(RuntimeError, match="weights must be a tensor"):
        mmsa.vote_filter(m, weights=np.zeros((2, 6, 8), dtype=np.float32))
    # the map and the outputs
    with pytest.raises(RuntimeError, match="map is torch.int32"):
        mmsa.vote_filter(m.int())
    with pytest.raises(RuntimeError, match=r"map must be a contiguous \[B, H, W\] tensor"):
        mmsa.vote_filter(m[0])
    with pytest.raises(RuntimeError, match="an empty map"):
        mmsa.vote_filter(torch.zeros(1, 0, 8, dtype=torch.uint8))
    with pytest.raises(RuntimeError, match="out is torch.int32"):
        mmsa.vote_filter(m, out=m.int())
    with pytest.raises(RuntimeError, match=r"out has shape \(2, 6, 9\)"):
        mmsa.vote_filter(m, out=torch.zeros(2, 6, 9, dtype=torch.uint8))
    with pytest.raises(RuntimeError, match="out is the map; a stencil cannot run in place"):
        mmsa.vote_filter(m, out=m)
    with pytest.raises(RuntimeError, match="support is torch.uint16; a uint32 sum map"):
        mmsa.vote_filter(m, support=torch.zeros(2, 6, 8, dtype=torch.uint16))
    with pytest.raises(RuntimeError, match=r"support has shape \(2, 8, 6\)"):
        mmsa.vote_filter(m, support=torch.zeros(2, 8, 6, dtype=torch.uint32))
    with pytest.raises(RuntimeError, match="map must be a GPU tensor"):
        mmsa.vote_filter(m, 2, guide=g3, sigma=8.0, weights=torch.zeros(2, 6, 8), num_classes=25, hole=254, where="holes", half=True, out=torch.zeros_like(m),
                         support=torch.zeros(2, 6, 8, dtype=torch.uint32))


# ---- 6. the C entry on the host

def test_the_entry_refuses_bad_arguments_on_the_host():
    """Before any launch, so no GPU is needed: every pointer is a fake."""
    import mmsa
    raw = mmsa.lib.raw
    a, b, c, d, e, f, w = (ctypes.c_void_p(256 * k) for k in range(1, 8))
    ERR_ARG = -1

    def call(src=a, B=1, H=4, W=4, role=b, radius=2, all_=1, half=0, guide=e, Hg=4, Wg=4, G=3, lut=f, weight=w, out=c, support=d):
        rc = raw.mmsa_vote_filter_u8(src, B, H, W, role, radius, all_, half, guide, Hg, Wg, G, lut, weight, out, support, None)
        return (rc, mmsa.lib.last_error()) if rc else (0, "")

    for kw in (dict(src=None), dict(role=None), dict(out=None)):
        rc, msg = call(**kw)
        assert rc == ERR_ARG and "vote_filter_u8: src, role and out are required" in msg, msg
    for kw in (dict(guide=None), dict(lut=None)):
        rc, msg = call(**kw)
        assert rc == ERR_ARG and "vote_filter_u8: guide and range_lut come together; one of them is null" in msg, msg
    rc, msg = call(out=a)
    assert rc == ERR_ARG and "vote_filter_u8: out is src; a stencil cannot run in place" in msg, msg
    for kw in (dict(support=a), dict(support=c)):
        rc, msg = call(**kw)
        assert rc == ERR_ARG and "vote_filter_u8: support is a plane of its own, neither src nor out" in msg, msg
    for kw in (dict(out=e), dict(out=w), dict(support=e), dict(support=w)):
        rc, msg = call(**kw)
        assert rc == ERR_ARG and "vote_filter_u8: out and support are planes of their own, neither the guide nor the weights" in msg, msg
    for kw in (dict(B=0), dict(H=0), dict(W=-1), dict(H=1 << 16, W=1 << 15, Hg=1 << 16, Wg=1 << 15)):
        rc, msg = call(**kw)
        assert rc == ERR_ARG and "vote_filter_u8: bad map size" in msg, msg
    for r in (0, 17, 32, -1):
        rc, msg = call(radius=r)
        assert rc == ERR_ARG and f"vote_filter_u8: radius = {r}; 1..16 are supported" in msg, msg
    for v in (-1, 2):
        rc, msg = call(all_=v)
        assert rc == ERR_ARG and f"vote_filter_u8: all = {v}; 0 " in msg, msg
        rc, msg = call(half=v)
        assert rc == ERR_ARG and f"vote_filter_u8: half = {v}; 0 or 1" in msg, msg
    for G in (0, 2, 4, -1):
        rc, msg = call(G=G)
        assert rc == ERR_ARG and f"vote_filter_u8: G = {G}; a guide of 1 or 3 channels is supported" in msg, msg
    for kw in (dict(Hg=3), dict(Wg=3), dict(Hg=0, Wg=0)):
        rc, msg = call(**kw)
        assert rc == ERR_ARG and "vote_filter_u8: the guide is " in msg and "the map 4 x 4; the map is the guide's top-left corner" in msg, msg
    rc, msg = call(Hg=1 << 16, Wg=1 << 15)
    assert rc == ERR_ARG and "vote_filter_u8: bad guide size" in msg, msg
    rc, msg = call(B=1 << 30, H=65, W=65, Hg=65, Wg=65)
    assert rc == ERR_ARG and "vote_filter_u8: 1073741824 maps of 65 x 65 are more workgroups than a launch holds" in msg, msg
    # without a guide G, Hg and Wg are not looked at, and the next check is reached
    rc, msg = call(guide=None, lut=None, G=7, Hg=0, Wg=0, radius=0)
    assert rc == ERR_ARG and "vote_filter_u8: radius = 0" in msg, msg


# ---- 7. - 9. header, ctypes table, export, version

def test_the_entry_is_declared_bound_exported_and_versioned():
    import mmsa
    from tests.test_host_cpu import _header_prototypes
    hdr = open(os.path.join(ROOT, "include", "mmsa.h")).read()
    ver = open(os.path.join(ROOT, "include", "mmsa_version.h")).read()
    assert mmsa.lib.version() == mmsa.lib.ABI_VERSION == int(re.search(r"#define MMSA_ABI_VERSION (\d+)", ver).group(1)) == 114
    sig = mmsa.lib.SIGNATURES
    assert re.search(r"\bint " + ENTRY + r"\(", hdr) and ENTRY in sig and hasattr(mmsa.lib.raw, ENTRY) and ENTRY in ver
    kinds = {ctypes.c_void_p: "P", ctypes.c_int: "I"}
    assert _header_prototypes()[ENTRY] == ("I", [kinds[t] for t in sig[ENTRY]]) and len(sig[ENTRY]) == 17
    assert "vote_filter" in mmsa.__all__ and mmsa.vote_filter is E.vote_filter and E.MAX_VOTE_RADIUS == VR.MAX_RADIUS == 16 and E.MAX_RANGE_WEIGHT == VR.MAX_WEIGHT
    for word in ("S_best", "the smallest v", "2 S_best(p) > T(p)", "clipped at the image border", "1 137 438 720 < 2^31", "uint32 [B, H, W]"):
        assert word in hdr, word
    src = open(os.path.join(ROOT, "multimodal-sam-adapter_amd", "csrc", "vote.hip")).read()
    assert "1 137 438 720 < 2^31" in src and '#include "conf_bin.h"' in src and "static_assert" in src
    p = inspect.signature(mmsa.vote_filter).parameters
    assert list(p) == ["map", "radius", "guide", "sigma", "range_weights", "weights", "num_classes", "hole", "inert", "where", "half", "out", "support"]
    assert [p[k].default for k in list(p)[1:]] == [2, None, None, None, None, None, (), None, "all", False, None, None]
    assert all(p[k].kind is inspect.Parameter.KEYWORD_ONLY for k in list(p)[2:])
    for use in ("mmsa.vote_filter(pred, 8, guide=rgb, sigma=8, num_classes=C)", "guide=aux, sigma=6, weights=conf", 'hole=254, where="holes"',
                "mmsa.suppress_small(pred, 64, num_classes=C, fill=254)"):
        assert use in mmsa.vote_filter.__doc__, use
    assert list(inspect.signature(mmsa.majority_filter).parameters) == ["map", "radius", "num_classes", "hole", "inert", "where", "half", "out", "support"]


# ---- 10. what the filter is for

def scene(seed):
    """[96, 130], 25 classes: `truth` a 24-px block map cut at (5, 7); the guide its colours with noise of -6 .. 6; `pred` the same block map cut at (8, 10) --
    every contour displaced by 3 px in both axes -- with 5 % random classes, 3 % of the hole byte 250 and 1 % of the inert byte 254."""
    rng = np.random.default_rng(seed)
    H, W, C = 96, 130, 25
    big = np.kron(rng.integers(0, C, size=(5, 6)), np.ones((24, 24), dtype=np.int64)).astype(np.uint8)
    truth, pred = big[5:5 + H, 7:7 + W].copy(), big[8:8 + H, 10:10 + W].copy()
    palette = rng.integers(0, 256, size=(C, 3))
    guide = np.clip(palette[truth] + rng.integers(-6, 7, size=(H, W, 3)), 0, 255).astype(np.uint8)
    u = rng.random((H, W))
    spots = rng.integers(0, C, size=(H, W)).astype(np.uint8)
    pred[u < 0.05] = spots[u < 0.05]
    pred[(u >= 0.05) & (u < 0.08)] = 250
    pred[(u >= 0.08) & (u < 0.09)] = 254
    weights = (np.where(pred == truth, 0.9, 0.3) * rng.random((H, W))).astype(np.float32)
    return truth, pred, guide, weights


def scene_errors(seed):
    """The share of the counted pixels (those that are not inert) that differ from the truth: (majority r 8, guided 3-channel r 8, guided 1-channel r 8,
    majority r 2, weights alone r 2)."""
    truth, pred, guide, weights = scene(seed)
    role = MR.roles(**MR.CONFIGS["C25"])
    counted = pred != 254

    def err(out):
        return float((out != truth)[counted].mean())

    return (err(MR.majority(pred, role, 8)[0]), err(VR.vote(pred, role, 8, guide=guide, lut=VR.range_table(8.0, 3))[0]),
            err(VR.vote(pred, role, 8, guide=guide[..., 0], lut=VR.range_table(8.0, 1))[0]), err(MR.majority(pred, role, 2)[0]),
            err(VR.vote(pred, role, 2, wq=VR.wq_of(weights))[0]))


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_the_guided_filter_puts_displaced_contours_back(seed):
    """Conditions on the reference definition.  Measured (majority r 8, guided 3-channel r 8, guided 1-channel r 8, majority r 2, weights alone r 2):
    seed 1: 0.2141, 0.0001, 0.0142, 0.2158, 0.1485;  seed 2: 0.2227, 0.0016, 0.0227, 0.2247, 0.1548;  seed 3: 0.2187, 0.0000, 0.0088, 0.2230, 0.1530.
    The 1-channel guide is channel 0 of the 3-channel one: two classes whose colours lie close in that channel are what is left of its error."""
    maj8, g3, g1, maj2, w2 = scene_errors(seed)
    print(f"seed {seed}: majority r8 {maj8:.4f}, 3-channel guide {g3:.4f}, 1-channel guide {g1:.4f}, majority r2 {maj2:.4f}, weights alone r2 {w2:.4f}")
    assert maj8 > 0.1
    assert g3 <= maj8 / 10, (g3, maj8)
    assert g1 <= maj8 / 5, (g1, maj8)
    assert w2 < maj2, (w2, maj2)
