"""The majority filter without a GPU: the restatement (tests/majority_ref.py) against the brute-force version and against scipy's convolution, hand-made maps
with the result written out, the condition that the shared GPU cases hide nothing, every argument refusal that needs no device, the C entry's checks on the
host, and header / ctypes table / version."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest
import torch

from tests import majority_ref as MR

import mmsa.evaluate as E  # noqa: E402  (what this file is about)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY = "mmsa_majority_filter_u8"
h, i = MR.HOLES[1], MR.INERT[0]
ANY = MR.roles(**MR.CONFIGS["any"])
SMALL = [c.name for c in MR.CASES if MR.maps_of(c.name)[0].size <= 3 * 200]      # every degenerate shape, 3 x 200 at radius 8 and the 63 / 64 / 65 columns


# ---- 1. the restatement

def _equal(got, want, what):
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), what


def test_the_restatement_equals_brute_force_on_every_small_case():
    n = 0
    for name in SMALL:
        role, r = MR.role_of(name), MR.CASE[name].radius
        for b, m in enumerate(MR.maps_of(name)):
            for where, half in MR.MODES:
                want = MR.brute(m, role, r, where == "all", half)
                _equal((MR.want_of(name, where, half)[0][b], MR.want_of(name, where, half)[1][b]), want, (name, b, where, half))
                n += 1
    assert n >= 13 * len(MR.STACK) * 4


def test_the_restatement_equals_brute_force_on_random_small_maps():
    rng = np.random.default_rng(4)
    changed = 0
    for trial in range(120):
        H, W = (int(v) for v in rng.integers(1, 12, size=2))
        m = MR.noise(H, W, 300 + trial, (2, 3, 25)[trial % 3], 0.15, 0.1)
        r = int(rng.integers(1, 5))
        role = MR.roles(**MR.CONFIGS[("any", "C25")[trial % 2]])
        where, half = MR.MODES[trial % 4]
        got = MR.majority(m, role, r, where == "all", half)
        _equal(got, MR.brute(m, role, r, where == "all", half), (trial, m.tolist(), r, where, half))
        changed += int((got[0] != m).any())
    assert changed > 80


def test_the_counts_equal_scipy_convolution():
    """An independent route to n_v, T and n_best: per value the indicator convolved with a box of ones, zero padded."""
    ndi = pytest.importorskip("scipy.ndimage")
    seen = 0
    for name in ("stack 9x65 radius 3 C25", "stack 3x200 radius 8 any", "stack 67x131 radius 2 any", "stack 67x131 radius 17 C25", "three of 70x90 radius 3"):
        role, r = MR.role_of(name), MR.CASE[name].radius
        ones = np.ones((2 * r + 1, 2 * r + 1), dtype=np.int64)
        for m, vt in zip(MR.maps_of(name), MR.votes_of(name)):
            voter = role[m] == 0
            counts = {v: ndi.convolve((voter & (m == v)).astype(np.int64), ones, mode="constant", cval=0) for v in np.unique(m[voter]).tolist()}
            if not counts:
                assert not vt.total.any()
                continue
            vals = np.array(sorted(counts))
            n = np.stack([counts[v] for v in vals.tolist()])
            assert np.array_equal(n.sum(axis=0), vt.total) and np.array_equal(n.max(axis=0), vt.best)
            assert np.array_equal(vals[n.argmax(axis=0)][vt.best > 0], vt.value[vt.best > 0])               # argmax: the first of equals, the smallest v
            assert np.array_equal((n == n.max(axis=0)).sum(axis=0)[vt.best > 0], vt.tied[vt.best > 0])
            for v in vals.tolist():
                at = voter & (m == v)
                assert np.array_equal(counts[v][at], vt.own[at])
            seen += 1
    assert seen >= 25


def test_the_roles_agree_with_the_package():
    for cfg in MR.CONFIGS.values():
        assert np.array_equal(MR.roles(**cfg), E.majority_roles(**cfg))
    assert np.array_equal(E.majority_roles(), np.zeros(256, dtype=np.uint8))                             # no list, no class count: every byte votes
    r = E.majority_roles(5, hole=[7, 9], inert=np.uint8(3))
    assert r.dtype == np.uint8 and r.shape == (256,) and not r[[0, 1, 2, 4]].any() and r[7] == r[9] == 1 and r[3] == 2 and (r[5:7] == 2).all() and (r[10:] == 2).all()
    assert (E.MAJORITY_VOTER, E.MAJORITY_HOLE, E.MAJORITY_INERT) == (MR.VOTER, MR.HOLE, MR.INERT_ROLE) == (0, 1, 2) and E.MAX_MAJORITY_RADIUS == 32


# ---- 2. by hand

def _run(m, r, where="all", half=False, role=ANY):
    m = np.asarray(m, dtype=np.uint8)
    got = MR.majority(m, role, r, where == "all", half)
    _equal(got, MR.brute(m, role, r, where == "all", half), "brute")
    return got[0].tolist(), got[1].tolist()


def test_a_checkerboard_stays():
    """Two values alternating: in every window the own value is among the tied (or ahead), so nothing changes."""
    m = (np.add.outer(np.arange(4), np.arange(6)) % 2 + 3).astype(np.uint8)
    out, support = _run(m, 1)
    assert out == m.tolist() and support == [[2, 3, 3, 3, 3, 2], [3, 5, 5, 5, 5, 3], [3, 5, 5, 5, 5, 3], [2, 3, 3, 3, 3, 2]]
    assert _run(m, 1, half=True)[0] == m.tolist()


def test_a_three_way_tie_at_a_hole_goes_to_the_smallest_value():
    m = [[9, 9, 4], [4, h, 6], [6, i, i]]                                                              # the hole sees 9, 9, 4, 4, 6, 6
    assert _run(m, 1, "holes") == ([[9, 9, 4], [4, 4, 6], [6, i, i]], [[0, 0, 0], [0, 2, 0], [0, 0, 0]])
    # where="all": the voters are targets too.  (0, 1) sees 9, 9, 4, 4, 6 and keeps its 9, which is among the tied; (1, 0) sees 9, 9, 4, 6: no tie, 9
    assert _run(m, 1) == ([[9, 9, 4], [9, 4, 6], [6, i, i]], [[2, 2, 1], [2, 2, 1], [1, 0, 0]])
    # a voter that is NOT among the tied takes the smallest of them: the 7 sees 5, 5, 8, 8 and itself once
    assert _run([[5, 5, 7, 8, 8]], 2) == ([[5, 5, 5, 8, 8]], [[2, 2, 2, 2, 2]])


def test_exactly_half_stays_under_half():
    # the hole's window: 2 x value 4, 1 x 6, 1 x 9: 2 * 2 = 4 = T
    m = [[4, 4, 6], [i, h, 9], [i, i, i]]
    assert _run(m, 1, "holes", half=True) == (m, [[0, 0, 0], [0, 2, 0], [0, 0, 0]])                     # stays, and support tells the count all the same
    assert _run(m, 1, "holes")[0] == [[4, 4, 6], [i, 4, 9], [i, i, i]]
    m[2][2] = 4                                                                                         # 3 of 5: more than half
    assert _run(m, 1, "holes", half=True) == ([[4, 4, 6], [i, 4, 9], [i, i, 4]], [[0, 0, 0], [0, 3, 0], [0, 0, 0]])


def test_the_core_of_a_wide_hole_block_stays():
    m = np.full((7, 7), 2, dtype=np.uint8)
    m[1:6, 1:6] = h                                                                                     # 5 x 5 holes, radius 1: the 3 x 3 core sees holes only
    out, support = MR.majority(m, ANY, 1, False, False)
    want = np.full((7, 7), 2, dtype=np.uint8)
    want[2:5, 2:5] = h
    assert np.array_equal(out, want) and not support[2:5, 2:5].any() and support[1, 1] == 5 and support[1, 3] == 3 and not support[0].any()
    _equal((out, support), MR.brute(m, ANY, 1, False, False), "brute")


def test_degenerate_shapes():
    assert _run([[5]], 1) == ([[5]], [[1]]) and _run([[5]], 32, half=True) == ([[5]], [[1]])
    assert _run([[h]], 3) == ([[h]], [[0]]) and _run([[i]], 3) == ([[i]], [[0]])
    # 3 x 200 at radius 8: the image is thinner than the halo; a one-value map counts its clipped windows
    out, support = MR.majority(np.full((3, 200), 7, dtype=np.uint8), ANY, 8)
    x = np.arange(200)
    assert (out == 7).all() and np.array_equal(support, np.tile(3 * (np.minimum(x + 8, 199) - np.maximum(x - 8, 0) + 1), (3, 1)))
    m = MR.noise(3, 200, 1, 3)
    _equal(MR.majority(m, ANY, 8), MR.brute(m, ANY, 8), "3 x 200")


def test_inert_pixels_vote_nothing_and_stay():
    m = [[i, i, i], [3, 5, 3], [i, 3, i]]
    assert _run(m, 1) == ([[i, i, i], [3, 3, 3], [i, 3, i]], [[0, 0, 0], [2, 3, 2], [0, 3, 0]])
    # with a class count every byte from C on that is no hole is inert: 200 stays and does not vote, 255 is a hole and takes the vote
    role = MR.roles(**MR.CONFIGS["C25"])
    assert _run([[200, 200, 200], [200, 255, 1], [200, 200, 200]], 1, role=role)[0] == [[200, 200, 200], [200, 1, 1], [200, 200, 200]]


# ---- 3. the shared GPU cases hide nothing

def test_the_gpu_cases_hide_nothing():
    seen = dict(own_tie=0, smallest_tie=0, exact_half=0, voteless_hole=0, seam_left=0, seam_right=0)
    edges = np.zeros(8, dtype=np.int64)                       # changed pixels: first / last row, first / last column, the four corners
    for c in MR.CASES:
        role, maps = MR.role_of(c.name), MR.maps_of(c.name)
        out = MR.want_of(c.name)[0]
        names = MR.STACK if c.name.startswith("stack") else ("patchy", "noise 25") if c.name.startswith("two") else ("patchy", "noise 3", "noise 25")
        for b, (m, vt) in enumerate(zip(maps, MR.votes_of(c.name))):
            voter, hole = role[m] == MR.VOTER, role[m] == MR.HOLE
            ch = out[b] != m
            seen["own_tie"] += int((voter & (vt.own == vt.best) & (vt.tied >= 2)).sum())
            seen["smallest_tie"] += int((ch & (vt.tied >= 2)).sum())
            seen["exact_half"] += int(((voter | hole) & (vt.total > 0) & (2 * vt.best == vt.total)).sum())
            seen["voteless_hole"] += int((hole & (vt.total == 0)).sum())
            if m.shape[1] > 64:
                seen["seam_left"] += int(ch[:, 63].sum())
                seen["seam_right"] += int(ch[:, 64].sum())
            edges += [ch[0].sum(), ch[-1].sum(), ch[:, 0].sum(), ch[:, -1].sum(), ch[0, 0], ch[0, -1], ch[-1, 0], ch[-1, -1]]
            noisy = names[b] in MR.NOISY and not (names[b] == "noise 200" and c.config == "C25")      # most of that map is inert then
            if noisy and c.radius <= 3 and m.size >= 500:
                assert ch.sum() * 100 >= m.size, (c.name, names[b], int(ch.sum()), m.size)
                # the half rule and the holes-only mode act as well, each on what it is meant for
                assert (MR.want_of(c.name, "holes")[0][b] != m).any(), (c.name, names[b])
                if names[b] in ("noise 3", "patchy") and c.radius <= 2 and m.size >= 5000:
                    some = MR.want_of(c.name, "all", True)[0][b] != m
                    assert some.any() and (some != ch).any(), (c.name, names[b])
    assert all(v > 0 for v in seen.values()), seen
    assert (edges > 0).all(), edges.tolist()


def test_the_figures_of_the_reference_case():
    """25-value noise at 67 x 131, radius 1: what the restatement gives, so that a change to it or to the generator shows."""
    name = "stack 67x131 radius 1 any"
    m, vt, out = MR.maps_of(name)[0], MR.votes_of(name)[0], MR.want_of(name)[0][0]
    voter = MR.role_of(name)[m] == 0
    own_tie = int((voter & (vt.own == vt.best) & (vt.tied >= 2)).sum())
    changed = int((out != m).sum())
    assert own_tie > 2000 and changed > 3000 and own_tie + changed <= m.size, (own_tie, changed)
    holes = MR.want_of(name, "holes")[0][0]
    assert (holes != m).sum() == np.isin(m, MR.HOLES).sum() > 100 and np.array_equal(holes[voter], m[voter])      # every hole of a noise map has a voter near


# ---- 4. refusals that need no device

def test_python_refusals():
    import mmsa
    m = torch.zeros(1, 6, 8, dtype=torch.uint8)
    for bad in (0, 33, -1, 2.0, None, True, "1"):
        with pytest.raises(ValueError, match="radius = .*an int in 1..32"):
            mmsa.majority_filter(m, bad)
    for bad in ([3, 300], -1, 256, "255", None, 2.0, True):
        with pytest.raises(ValueError, match="hole = "):
            mmsa.majority_filter(m, hole=bad)
    for bad in (300, [1, -2], "254", 1.5):
        with pytest.raises(ValueError, match="inert = "):
            mmsa.majority_filter(m, inert=bad)
    with pytest.raises(ValueError, match=r"hole and inert share the bytes \[254\]"):
        mmsa.majority_filter(m, hole=[254, 255], inert=254)
    with pytest.raises(ValueError, match=r"hole holds the bytes \[3\], which are among the 5 classes"):
        mmsa.majority_filter(m, num_classes=5, hole=[3, 255])
    for bad in (0, 257, 2.5, True, "25"):
        with pytest.raises(ValueError, match="num_classes = "):
            mmsa.majority_filter(m, num_classes=bad)
    with pytest.raises(ValueError, match='where = "holes" and hole is empty'):
        mmsa.majority_filter(m, where="holes")
    for bad in ("some", None, 1, "ALL"):
        with pytest.raises(ValueError, match="where = "):
            mmsa.majority_filter(m, hole=255, where=bad)
    for bad in (1, None, "yes"):
        with pytest.raises(ValueError, match="half = "):
            mmsa.majority_filter(m, half=bad)
    with pytest.raises(RuntimeError, match="map is torch.int32"):
        mmsa.majority_filter(m.int())
    with pytest.raises(RuntimeError, match=r"map must be a contiguous \[B, H, W\] tensor"):
        mmsa.majority_filter(m[0])
    with pytest.raises(RuntimeError, match="map must be a tensor"):
        mmsa.majority_filter(m.numpy())
    with pytest.raises(RuntimeError, match="an empty map"):
        mmsa.majority_filter(torch.zeros(1, 0, 8, dtype=torch.uint8))
    with pytest.raises(RuntimeError, match="out is torch.int32"):
        mmsa.majority_filter(m, out=m.int())
    with pytest.raises(RuntimeError, match=r"out has shape \(1, 6, 9\)"):
        mmsa.majority_filter(m, out=torch.zeros(1, 6, 9, dtype=torch.uint8))
    with pytest.raises(RuntimeError, match="out is the map; a stencil cannot run in place"):
        mmsa.majority_filter(m, out=m)
    with pytest.raises(RuntimeError, match="support is torch.int16; a uint16 count map"):
        mmsa.majority_filter(m, support=torch.zeros(1, 6, 8, dtype=torch.int16))
    with pytest.raises(RuntimeError, match=r"support has shape \(1, 8, 6\)"):
        mmsa.majority_filter(m, support=torch.zeros(1, 8, 6, dtype=torch.uint16))
    with pytest.raises(RuntimeError, match="map must be a GPU tensor"):
        mmsa.majority_filter(m, 2, num_classes=25, hole=254, where="holes", half=True, out=torch.zeros_like(m), support=torch.zeros(1, 6, 8, dtype=torch.uint16))
    p = inspect.signature(mmsa.majority_filter).parameters
    assert list(p) == ["map", "radius", "num_classes", "hole", "inert", "where", "half", "out", "support"]
    assert [p[k].default for k in list(p)[1:]] == [1, None, (), None, "all", False, None, None]
    assert all(p[k].kind is inspect.Parameter.KEYWORD_ONLY for k in list(p)[2:])
    for use in ("mmsa.majority_filter(pred, 2, num_classes=C)", "half=True", 'hole=254, where="holes"'):
        assert use in mmsa.majority_filter.__doc__
    # the neighbours keep their signatures
    assert list(inspect.signature(mmsa.suppress_small).parameters) == ["pred", "min_area", "num_classes", "connectivity", "fill", "out", "root", "area", "nearest"]
    assert list(inspect.signature(mmsa.select_segments).parameters) == ["pred", "table", "keep", "fill", "out", "nearest"]


def test_the_entry_refuses_bad_arguments_on_the_host():
    """Before any launch, so no GPU is needed: every pointer is a fake."""
    import mmsa
    raw = mmsa.lib.raw
    a, b, c, d = (ctypes.c_void_p(256 * k) for k in range(1, 5))
    ERR_ARG = -1

    def call(src=a, B=1, H=4, W=4, role=b, radius=2, all_=1, half=0, out=c, support=d):
        rc = raw.mmsa_majority_filter_u8(src, B, H, W, role, radius, all_, half, out, support, None)
        return (rc, mmsa.lib.last_error()) if rc else (0, "")

    for kw in (dict(src=None), dict(role=None), dict(out=None)):
        rc, msg = call(**kw)
        assert rc == ERR_ARG and "majority_filter_u8: src, role and out are required" in msg, msg
    rc, msg = call(out=a)
    assert rc == ERR_ARG and "majority_filter_u8: out is src; a stencil cannot run in place" in msg, msg
    for kw in (dict(support=a), dict(support=c)):
        rc, msg = call(**kw)
        assert rc == ERR_ARG and "majority_filter_u8: support is a plane of its own, neither src nor out" in msg, msg
    for kw in (dict(B=0), dict(H=0), dict(W=-1), dict(H=1 << 16, W=1 << 15)):
        rc, msg = call(**kw)
        assert rc == ERR_ARG and "majority_filter_u8: bad map size" in msg, msg
    for r in (0, 33, -1):
        rc, msg = call(radius=r)
        assert rc == ERR_ARG and f"majority_filter_u8: radius = {r}; 1..32 are supported" in msg, msg
    for v in (-1, 2):
        rc, msg = call(all_=v)
        assert rc == ERR_ARG and f"majority_filter_u8: all = {v}; 0 " in msg, msg
        rc, msg = call(half=v)
        assert rc == ERR_ARG and f"majority_filter_u8: half = {v}; 0 or 1" in msg, msg
    rc, msg = call(B=1 << 30, H=65, W=65)
    assert rc == ERR_ARG and "majority_filter_u8: 1073741824 maps of 65 x 65 are more workgroups than a launch holds" in msg, msg


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
    assert "majority_filter" in mmsa.__all__ and mmsa.majority_filter is E.majority_filter
    for word in ("n_best", "the smallest v", "2 n_best(p) > T(p)", "clipped at the image border", "65^2 = 4225"):
        assert word in hdr, word
