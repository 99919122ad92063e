"""The nearest-label fill without a GPU: the restatement (tests/fill_nearest_ref.py) against a brute-force search and against scipy's exact transform, the tie
rules on hand-made maps with the result written out, what the restatement predicts for every input of tests/test_fill_nearest_gpu.py, every argument refusal
that needs no device, the C entry's checks on the host, and header / ctypes table / version."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest
import torch

from tests import fill_nearest_ref as FR

import mmsa.evaluate as E  # noqa: E402  (what this file is about)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY = "mmsa_fill_nearest_u8"
h, i = FR.HOLES[1], FR.INERT[0]


# ---- 1. the restatement

def test_the_restatement_equals_brute_force_on_random_small_maps():
    rng = np.random.default_rng(3)
    n = 0
    for trial in range(300):
        H, W = (int(v) for v in rng.integers(1, 14, size=2))
        m = FR.noise(H, W, 100 + trial, (0.1, 0.5, 0.9)[trial % 3], inert_share=0.2)
        cap = int(rng.integers(1, 7))
        got, want = FR.fill(m, FR.HOLES, FR.INERT, cap), FR.brute(m, FR.HOLES, FR.INERT, cap)
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), (trial, m.tolist(), cap)
        n += int((want[1] > 0).any())
    assert n > 250                                                                   # the maps do have holes


def test_the_roles_agree_with_the_package():
    assert np.array_equal(FR.roles(FR.HOLES, FR.INERT), E.fill_roles(FR.HOLES, FR.INERT)) and np.array_equal(FR.roles(255), E.fill_roles())
    assert FR.FAR == E.FILL_FAR == 65535 and (E.FILL_SOURCE, E.FILL_HOLE, E.FILL_INERT) == (0, 1, 2)
    r = E.fill_roles(hole=[7, 9], inert=np.uint8(3))
    assert r.dtype == np.uint8 and r.shape == (256,) and r[7] == r[9] == 1 and r[3] == 2 and r.sum() == 4


def _sources_by_value(m):
    """{value: squared exact distance to the nearest source of that value}, and the same over all sources, by scipy."""
    ndi = pytest.importorskip("scipy.ndimage")
    src = FR.roles(FR.HOLES, FR.INERT)[m] == 0
    sq = lambda mask: np.rint(ndi.distance_transform_edt(~mask) ** 2).astype(np.int64)      # noqa: E731
    return sq(src), {int(v): sq(src & (m == v)) for v in np.unique(m[src])}


def test_the_distances_equal_scipy_and_every_filled_value_is_a_source_at_that_distance():
    """Independent of the tie-break: d2 is the rounded square of scipy's exact transform wherever that is at most cap^2 and FAR elsewhere, and the value a hole
    took is the value of SOME source at exactly that distance."""
    pytest.importorskip("scipy.ndimage")
    seen = 0
    for c in FR.CASES:
        if c.name.startswith("stack") and max(FR.maps_of(c.name).shape[1:]) > 140:      # the large stacks: the noise maps only
            pick = [k for k, n in enumerate(FR.STACK) if n.startswith("noise")]
        else:
            pick = range(FR.maps_of(c.name).shape[0])
        out, d2 = FR.want_of(c.name)
        for b in pick:
            m = FR.maps_of(c.name)[b]
            holes = np.isin(m, FR.HOLES)
            if not holes.any() or holes.all():
                continue
            every, by_value = _sources_by_value(m)
            want = np.where(holes, np.where(every <= c.cap ** 2, every, FR.FAR), 0)
            assert np.array_equal(d2[b], want), (c.name, b)
            filled = holes & (d2[b] != FR.FAR)
            assert np.array_equal(out[b][~filled], m[~filled]), (c.name, b)
            for v in np.unique(out[b][filled]):
                at = filled & (out[b] == v)
                assert int(v) in by_value and np.array_equal(by_value[int(v)][at], d2[b][at].astype(np.int64)), (c.name, b, int(v))
            seen += 1
    assert seen > 100


# ---- 2. the tie rules, by hand

def _fill(m, cap, hole=FR.HOLES, inert=FR.INERT):
    m = np.asarray(m, dtype=np.uint8)
    got, brute = FR.fill(m, hole, inert, cap), FR.brute(m, hole, inert, cap)
    assert np.array_equal(got[0], brute[0]) and np.array_equal(got[1], brute[1])
    return got[0].tolist(), got[1].tolist()


def test_ties_by_hand():
    # four differently valued sources at up / down / left / right of a hole: the upper one; a corner between two: the upper one, or else the left one
    out, d2 = _fill(FR.CROSS, 1)
    assert out == FR.CROSS_FILLED.tolist() == [[1, 1, 1], [3, 1, 4], [3, 2, 4]] and d2 == [[1, 0, 1], [0, 1, 0], [1, 0, 1]]
    # left against right: left
    assert _fill([[3, h, 4]], 5) == ([[3, 3, 4]], [[0, 1, 0]])
    assert _fill([[3, h, h, h, 4]], 5) == ([[3, 3, 3, 4, 4]], [[0, 1, 4, 1, 0]])
    # up against down: up
    assert _fill([[3], [h], [4]], 5) == ([[3], [3], [4]], [[0], [1], [0]])
    # up-right against down-left at the same d2 = 2: up-right, the smaller qy; the inert bytes stay and offer nothing
    assert _fill(FR.DIAG, 2) == ([[i, i, 5], [i, 5, i], [6, i, i]], [[0, 0, 0], [0, 2, 0], [0, 0, 0]])
    assert _fill(FR.DIAG[::-1], 2)[0] == [[6, i, i], [i, 6, i], [i, i, 5]]            # mirrored: down-right against up-left: up-left
    assert _fill(FR.DIAG, 1) == (FR.DIAG.tolist(), [[0, 0, 0], [0, FR.FAR, 0], [0, 0, 0]])      # d2 = 2 > cap^2 = 1: the hole stays
    # a nearer source below beats a farther one above, and inert pixels in between block nothing
    assert _fill([[3], [i], [i], [h], [i], [4]], 5)[0] == [[3], [i], [i], [4], [i], [4]]
    # the other hole byte fills as well, and a hole never offers its byte
    assert _fill([[FR.HOLES[0], h, 9]], 2) == ([[9, 9, 9]], [[4, 1, 0]])


def test_the_cap_by_hand():
    # along a row at cap 3: distance 3 fills, distance 4 does not
    assert _fill([[7, h, h, h, h]], 3) == ([[7, 7, 7, 7, h]], [[0, 1, 4, 9, FR.FAR]])
    # d2 == cap^2 = 25 fills -- (0, 5), (5, 0), (3, 4), (4, 3) -- and cap^2 + 1 = 26 -- (1, 5), (5, 1) -- does not
    m = np.full((6, 6), h, dtype=np.uint8)
    m[0, 0] = 7
    out, d2 = FR.fill(m, FR.HOLES, FR.INERT, 5)
    y, x = np.mgrid[0:6, 0:6]
    d = y * y + x * x
    assert np.array_equal(out == 7, d <= 25) and np.array_equal(d2, np.where(d <= 25, d, FR.FAR)) and d2[3, 4] == d2[0, 5] == 25 and d2[1, 5] == d2[5, 1] == FR.FAR
    assert np.array_equal(FR.brute(m, FR.HOLES, FR.INERT, 5)[0], out)
    # no hole: a copy, d2 all 0; all holes: unchanged, d2 all FAR
    m = FR.noise(5, 9, 1, 0.0)
    assert np.array_equal(FR.fill(m, FR.HOLES, FR.INERT, 9)[0], m) and not FR.fill(m, FR.HOLES, FR.INERT, 9)[1].any()
    m = np.full((5, 9), h, dtype=np.uint8)
    assert np.array_equal(FR.fill(m, FR.HOLES, FR.INERT, 9)[0], m) and (FR.fill(m, FR.HOLES, FR.INERT, 9)[1] == FR.FAR).all()


# ---- 3. what the restatement predicts for the inputs of the GPU file

# holes, filled, left: seeded noise over 25 classes, `sparse` of tests/fill_nearest_ref.py
PREDICTED = {"partial 67x131 1% cap 4": (8711, 2588, 6123), "full 67x131 1% cap 255": (8711, 8711, 0), "partial 300x520 0.05% cap 32": (155919, 115593, 40326)}


def _numbers(name, b=None):
    m, (out, d2) = FR.maps_of(name), FR.want_of(name)
    if b is not None:
        m, out, d2 = m[b], out[b], d2[b]
    holes = np.isin(m, FR.HOLES)
    filled, left = holes & (d2 != FR.FAR), holes & (d2 == FR.FAR)
    assert np.array_equal(out[~filled], m[~filled]) and not np.isin(out[filled], FR.HOLES + FR.INERT).any() and not d2[~holes].any(), name
    assert (d2[filled] >= 1).all() and (d2[filled] <= FR.CASE[name].cap ** 2).all(), name
    return int(holes.sum()), int(filled.sum()), int(left.sum())


def test_the_predicted_numbers_of_every_gpu_case():
    for c in FR.CASES:
        holes, filled, left = _numbers(c.name)
        assert holes == filled + left, c.name
        if c.name in PREDICTED:
            assert (holes, filled, left) == PREDICTED[c.name], (c.name, holes, filled, left)
        if c.name.startswith("partial"):
            assert filled > 0 and left > 0, c.name      # a kernel that fills nothing, or ignores the cap, cannot pass
    assert sum(c.name.startswith("partial") for c in FR.CASES) == 2
    for H, W in FR.SHAPES:
        for cap in (3, 255):
            name = f"stack {H}x{W} cap {cap}"
            per = {n: _numbers(name, b) for b, n in enumerate(FR.STACK)}
            assert per["no hole"] == (0, 0, 0) and per["all holes"] == (H * W, 0, H * W), name
            for n in ("corner source", "centre source"):
                assert per[n][0] == H * W - 1, name
                if max(H, W) > 8 and cap == 3:
                    assert per[n][1] > 0 and per[n][2] > 0, (name, n)      # the disc's edge lies inside the map
            if H * W > 1:
                assert per["noise 50%"][1] > 0 and per["cross tiled"][1] > 0, name
    # 300 x 520 at cap 255: the corner source reaches 255 pixels along its row and its column and no further
    d2 = FR.want_of("stack 300x520 cap 255")[1][FR.STACK.index("corner source")]
    assert d2[299, 255] == 255 ** 2 and d2[299, 256] == FR.FAR and d2[299 - 255, 0] == 255 ** 2 and d2[299 - 256, 0] == FR.FAR
    # the scan cases: a row of 513 filled from one end as far as the cap reaches
    for x in (0, 512):
        d2 = FR.want_of(f"scan 1x513 source at x = {x}")[1][0, 0]
        assert np.array_equal(d2, np.where(np.abs(np.arange(513) - x) <= 255, (np.arange(513) - x) ** 2, FR.FAR))


# ---- 4. refusals that need no device

def test_python_refusals():
    import mmsa
    m = torch.zeros(1, 6, 8, dtype=torch.uint8)
    for bad in ((), [], [3, 300], -1, 256, "255", None, 2.0, True):
        with pytest.raises(ValueError, match="hole"):
            mmsa.fill_nearest(m, hole=bad)
    for bad in (300, [1, -2], "254", 1.5):
        with pytest.raises(ValueError, match="inert = "):
            mmsa.fill_nearest(m, inert=bad)
    with pytest.raises(ValueError, match=r"hole and inert share the bytes \[254\]"):
        mmsa.fill_nearest(m, hole=[254, 255], inert=254)
    for bad in (0, 256, -3, 2.0, None, True):
        with pytest.raises(ValueError, match="cap = .*1..255 pixels"):
            mmsa.fill_nearest(m, cap=bad)
    with pytest.raises(RuntimeError, match="map is torch.int32"):
        mmsa.fill_nearest(m.int())
    with pytest.raises(RuntimeError, match=r"map must be a contiguous \[B, H, W\] tensor"):
        mmsa.fill_nearest(m[0])
    with pytest.raises(RuntimeError, match="map must be a tensor"):
        mmsa.fill_nearest(m.numpy())
    with pytest.raises(RuntimeError, match="an empty map"):
        mmsa.fill_nearest(torch.zeros(1, 0, 8, dtype=torch.uint8))
    with pytest.raises(RuntimeError, match="out is torch.int32"):
        mmsa.fill_nearest(m, out=m.int())
    with pytest.raises(RuntimeError, match=r"out has shape \(1, 6, 9\)"):
        mmsa.fill_nearest(m, out=torch.zeros(1, 6, 9, dtype=torch.uint8))
    with pytest.raises(RuntimeError, match="d2 is torch.int16; a uint16 distance map"):
        mmsa.fill_nearest(m, d2=torch.zeros(1, 6, 8, dtype=torch.int16))
    with pytest.raises(RuntimeError, match=r"d2 has shape \(1, 8, 6\)"):
        mmsa.fill_nearest(m, d2=torch.zeros(1, 8, 6, dtype=torch.uint16))
    for bad in (torch.zeros(47, dtype=torch.uint16), torch.zeros(48, dtype=torch.int32), torch.zeros(2, 48, dtype=torch.uint16)[:, ::2], np.zeros(48, dtype=np.uint16)):
        with pytest.raises(RuntimeError, match="scratch must be a contiguous uint16 tensor of at least 48 elements"):
            mmsa.fill_nearest(m, scratch=bad)
    plane = torch.zeros(1, 6, 8, dtype=torch.uint16)
    with pytest.raises(RuntimeError, match="scratch and d2 are two planes"):
        mmsa.fill_nearest(m, d2=plane, scratch=plane)
    with pytest.raises(RuntimeError, match="map must be a GPU tensor"):
        mmsa.fill_nearest(m, d2=plane, scratch=torch.zeros(64, dtype=torch.uint16), out=m)
    # nearest= of the calls that paint
    for fill in (0, 4):
        with pytest.raises(ValueError, match=f"suppress_small: fill = {fill} with nearest=: the byte is one of the 5 classes"):
            mmsa.suppress_small(m, 4, num_classes=5, fill=fill, nearest=8)
        with pytest.raises(ValueError, match=f"select_segments: fill = {fill} with nearest=: the byte is one of the 5 classes"):
            mmsa.select_segments(m, mmsa.SegmentTable(num_classes=5), None, fill=fill, nearest=8)
    for bad in (0, 256, 1.5, True):
        with pytest.raises(ValueError, match="suppress_small: cap = "):
            mmsa.suppress_small(m, 4, num_classes=5, nearest=bad)
        with pytest.raises(ValueError, match="select_segments: cap = "):
            mmsa.select_segments(m, mmsa.SegmentTable(num_classes=5), None, nearest=bad)
    with pytest.raises(RuntimeError, match="pred must be a GPU tensor"):
        mmsa.suppress_small(m, 4, num_classes=5, fill=5, nearest=8)      # the first byte that is no class: accepted
    for fn in (mmsa.suppress_small, mmsa.select_segments):
        assert inspect.signature(fn).parameters["nearest"].default is None and "fill=254" in fn.__doc__ and "held it before the call" in fn.__doc__
    p = inspect.signature(mmsa.fill_nearest).parameters
    assert list(p) == ["map", "hole", "inert", "cap", "out", "d2", "scratch"] and (p["hole"].default, p["inert"].default, p["cap"].default) == (255, (), 32)
    assert list(inspect.signature(mmsa.abstain).parameters) == ["pred", "conf", "bins", "min_bin", "out", "threshold"] and "fill_nearest" in mmsa.abstain.__doc__


def test_the_entry_refuses_bad_arguments_on_the_host():
    """Before any launch, so no GPU is needed: every pointer is a fake."""
    import mmsa
    raw = mmsa.lib.raw
    a, b, c, d, e = (ctypes.c_void_p(256 * k) for k in range(1, 6))
    ERR_ARG = -1

    def call(src=a, B=1, H=4, W=4, role=b, none_byte=255, cap=8, scratch=c, out=d, d2=e):
        rc = raw.mmsa_fill_nearest_u8(src, B, H, W, role, none_byte, cap, scratch, out, d2, None)
        return (rc, mmsa.lib.last_error()) if rc else (0, "")

    for kw in (dict(src=None), dict(role=None), dict(scratch=None), dict(out=None)):
        rc, msg = call(**kw)
        assert rc == ERR_ARG and "fill_nearest_u8: src, role, scratch and out are required" in msg, msg
    for kw in (dict(scratch=e), dict(scratch=a), dict(scratch=d), dict(d2=d), dict(d2=a)):
        rc, msg = call(**kw)
        assert rc == ERR_ARG and "fill_nearest_u8: scratch and d2 are two planes, and neither is src or out" in msg, msg
    for kw in (dict(B=0), dict(H=0), dict(W=-1), dict(H=1 << 16, W=1 << 15)):
        rc, msg = call(**kw)
        assert rc == ERR_ARG and "fill_nearest_u8: bad map size" in msg, msg
    for cap in (0, 256, -1):
        rc, msg = call(cap=cap)
        assert rc == ERR_ARG and f"fill_nearest_u8: cap = {cap}; 1..255 are supported" in msg, msg
    for nb in (-1, 256):
        rc, msg = call(none_byte=nb)
        assert rc == ERR_ARG and f"fill_nearest_u8: none_byte = {nb}" in msg, msg
    rc, msg = call(B=1 << 30, H=4, W=4)
    assert rc == ERR_ARG and "fill_nearest_u8: 1073741824 maps of 4 x 4 are more workgroups than a launch holds" in msg, msg


def test_the_entry_is_declared_bound_exported_and_versioned():
    import mmsa
    from tests.test_host_cpu import _header_prototypes
    hdr = open(os.path.join(ROOT, "include", "mmsa.h")).read()
    ver = open(os.path.join(ROOT, "include", "mmsa_version.h")).read()
    assert mmsa.lib.version() == mmsa.lib.ABI_VERSION == int(re.search(r"#define MMSA_ABI_VERSION (\d+)", ver).group(1)) == 114
    sig = mmsa.lib.SIGNATURES
    assert re.search(r"\bint " + ENTRY + r"\(", hdr) and ENTRY in sig and hasattr(mmsa.lib.raw, ENTRY) and ENTRY in ver
    kinds = {ctypes.c_void_p: "P", ctypes.c_int: "I"}
    assert _header_prototypes()[ENTRY] == ("I", [kinds[t] for t in sig[ENTRY]])
    assert "fill_nearest" in mmsa.__all__ and mmsa.fill_nearest is E.fill_nearest
