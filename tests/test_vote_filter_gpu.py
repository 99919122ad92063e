"""The guided vote filter on the GPU (csrc/vote.hip): `out` and `support` of mmsa.vote_filter against the numpy restatement of tests/vote_filter_ref.py, byte for
byte, into buffers pre-filled with a canary -- degenerate axes, an image thinner than the halo, 63 / 64 / 65 columns, the row counts around the tile height,
several tiles at every radius class, a batch, the seven maps of majority_ref.stack in all four modes, crossed with 1 and 3 guide channels, a padded guide
frame, weights and two range tables -- and slot groups, the largest sums, windows without a vote, special weights, and identities on device results."""
import numpy as np
import pytest
import torch

from tests import majority_ref as MR
from tests import vote_filter_ref as VR

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CANARY_U8, CANARY_U16, CANARY_U32 = 0xA5, 0xBEEF, 0xDEADBEEF


def _dev(a):
    return None if a is None else torch.from_numpy(np.array(a)).to(DEV)      # a copy: the cached cases are read-only


def _host(t):
    return t.cpu().numpy()


def _canary(shape, dtype):
    return _dev(np.full(shape, {np.uint8: CANARY_U8, np.uint16: CANARY_U16, np.uint32: CANARY_U32}[dtype], dtype=dtype))


def _same(got, want, what):
    bad = np.argwhere(got != want)
    assert got.shape == want.shape and bad.size == 0, (what, len(bad), bad[:5].tolist(), got[tuple(bad[0])], want[tuple(bad[0])])


def _run(maps, radius, want, what, **kw):
    """One call into canary-filled out and support -> both equal `want`."""
    import mmsa
    out, support = _canary(maps.shape, np.uint8), _canary(maps.shape, np.uint32)
    got = mmsa.vote_filter(_dev(maps) if isinstance(maps, np.ndarray) else maps, radius, out=out, support=support, **kw)
    assert got is out, what
    _same(_host(out), want[0], (what, "out"))
    _same(_host(support), want[1], (what, "support"))
    return out, support


def _keywords(name, guide, weights):
    c = VR.CASE[name]
    kw = dict(MR.CONFIGS[c.config], guide=guide, weights=weights)
    if c.table == "sigma":
        kw["sigma"] = 8.0
    elif c.table == "cut":
        kw["range_weights"] = VR.cut_table(c.G)
    return kw


@pytest.mark.parametrize("name", [c.name for c in VR.CASES])
def test_every_case_equals_the_restatement(name):
    c = VR.CASE[name]
    maps, guide, weights = VR.inputs_of(name)
    src, g, w = _dev(maps), _dev(guide), _dev(weights)
    for where, half in MR.MODES:
        _run(src, c.radius, VR.want_of(name, where, half), (name, where, half), where=where, half=half, **_keywords(name, g, w))
    assert np.array_equal(_host(src), maps) and (g is None or np.array_equal(_host(g), guide)), name                 # the inputs are read only
    assert w is None or np.array_equal(_host(w).view(np.uint32), weights.view(np.uint32)), name


def test_the_cases_hide_nothing():
    """The shared cases change pixels, differ from the plain majority filter, and meet ties and voteless windows."""
    differ = tie = voteless = 0
    for c in VR.CASES:
        maps = VR.inputs_of(c.name)[0]
        out = VR.want_of(c.name)[0]
        plain = MR.majority_batch(maps, VR.role_of(c.name), c.radius)[0]
        differ += int((out != plain).sum())
        for m, vt in zip(maps, VR.sums_of(c.name)):
            tie += int((vt.tied >= 2).sum())
            voteless += int(((vt.total == 0) & (MR.box(VR.role_of(c.name)[m] == MR.VOTER, c.radius) > 0)).sum())
    assert differ > 10000 and tie > 1000 and voteless > 100, (differ, tie, voteless)


def test_slot_groups():
    """More than 32 values in a tile: 200-value noise with every byte a voter (six or seven walks per tile), and exactly 32 and 33 values in one tile."""
    role = MR.roles(**MR.CONFIGS["any"])
    m = MR.noise(40, 100, 5, 200)[None]
    guide, w = VR.guide_of(m, 3, (0, 0), 9), VR.weights_of(m.shape, 10)
    assert len(np.unique(m[0][:8 + 2, :64 + 2])) > 5 * 32                          # the first 8-row tile with its halo at radius 2: six or seven walks
    for r in (2, 16):
        want = VR.vote_batch(m, role, r, guide=guide, lut=VR.range_table(8.0, 3), wq=VR.wq_of(w))
        _run(m, r, want, ("noise 200", r), guide=_dev(guide), sigma=8.0, weights=_dev(w), **MR.CONFIGS["any"])
    rng = np.random.default_rng(3)
    for n in (32, 33):
        m = rng.integers(0, n, size=(1, 8, 64)).astype(np.uint8) * 3 + 1         # one tile of 8 rows; values 1, 4, 7, ...
        m[0, 0, :n] = np.arange(n) * 3 + 1
        assert len(np.unique(m)) == n
        w = VR.weights_of(m.shape, n)
        want = VR.vote_batch(m, role, 2, wq=VR.wq_of(w))
        _run(m, 2, want, ("values", n), weights=_dev(w))
        _run(m, 2, VR.vote_batch(m, role, 2, half=True, wq=VR.wq_of(w)), ("values, half", n), weights=_dev(w), half=True)


def test_the_largest_sums_do_not_overflow():
    r, H, W = 16, 40, 70
    m = np.full((1, H, W), 9, dtype=np.uint8)
    guide = np.full((1, H, W, 3), 77, dtype=np.uint8)
    out, support = _canary(m.shape, np.uint8), _canary(m.shape, np.uint32)
    import mmsa
    mmsa.vote_filter(_dev(m), r, guide=_dev(guide), range_weights=np.full(766, 4096), weights=_dev(np.ones(m.shape, dtype=np.float32)), out=out, support=support)
    s = _host(support)[0].astype(np.int64)
    y, x = np.arange(H)[:, None], np.arange(W)[None, :]
    taps = (np.minimum(y + r, H - 1) - np.maximum(y - r, 0) + 1) * (np.minimum(x + r, W - 1) - np.maximum(x - r, 0) + 1)
    _same(s, taps * 4096 * 255, "support")
    assert s[20, 35] == 1089 * 4096 * 255 == 1137438720 and s[0, 0] == s[-1, -1] == 17 * 17 * 4096 * 255 and np.array_equal(_host(out), m)


def test_windows_without_a_vote_stay():
    import mmsa
    m = MR.patchy(50, 90, 4)[None]
    role = MR.roles(**MR.CONFIGS["C25"])
    y, x = np.arange(50)[:, None], np.arange(90)[None, :]
    guide = ((y * 7 + x * 3) % 251).astype(np.uint8)[None]                          # every pixel differs from all others of a 5 x 5 window
    lut = np.zeros(256, dtype=np.uint16)
    lut[0] = 300
    w = VR.weights_of(m.shape, 6)
    wq = VR.wq_of(w)
    out, support = _run(m, 2, VR.vote_batch(m, role, 2, guide=guide, lut=lut, wq=wq), "table zero but at 0", guide=_dev(guide), range_weights=lut,
                        weights=_dev(w), **MR.CONFIGS["C25"])
    voter = role[m] == MR.VOTER
    assert np.array_equal(_host(out), m) and np.array_equal(_host(support)[voter], (300 * wq[voter]).astype(np.uint32)) and not _host(support)[~voter].any()
    nan = np.full(m.shape, np.nan, dtype=np.float32)
    out, support = _canary(m.shape, np.uint8), _canary(m.shape, np.uint32)
    mmsa.vote_filter(_dev(m), 3, weights=_dev(nan), out=out, support=support, **MR.CONFIGS["C25"])
    assert np.array_equal(_host(out), m) and not _host(support).any()


def test_special_weights():
    """Every special value as the weight of the one voter of a window: the support is its quantised weight."""
    f32 = np.float32
    edges = np.arange(0, 257, dtype=np.float32) / f32(256)
    ws = np.concatenate([edges, np.nextafter(edges, f32(-1)), np.nextafter(edges, f32(2)), VR.SPECIAL_WEIGHTS, np.array([1e-45, 1.1754942e-38, 3.4e38], dtype=f32)])
    n = len(ws)
    m = np.full((1, 3, 3 * n), 255, dtype=np.uint8)                                 # holes, and one voter in the middle of every 3 x 3 cell
    m[0, 1, 1::3] = 4
    w = np.zeros(m.shape, dtype=np.float32)
    w[0, 1, 1::3] = ws
    want = VR.vote_batch(m, MR.roles(None, 255), 1, wq=VR.wq_of(w))
    _, support = _run(m, 1, want, "special weights", weights=_dev(w), hole=255)
    assert np.array_equal(_host(support)[0, 0, 1::3], VR.wq_of(ws).astype(np.uint32))
    assert np.array_equal(want[0][0, 0, 1::3], np.where(VR.wq_of(ws) > 0, 4, 255))


@pytest.mark.parametrize("radius", [1, 3, 8, 16])
def test_unit_weights_are_the_majority_filter(radius):
    import mmsa
    maps = MR.stack(67, 131, radius)
    src = _dev(maps)
    guide = _dev(VR.guide_of(maps, 3, (2, 5), radius))
    for cfg in ("C25", "any"):
        for where, half in MR.MODES[:2] if cfg == "any" else MR.MODES:
            kw = dict(where=where, half=half, **MR.CONFIGS[cfg])
            s16 = _canary(maps.shape, np.uint16)
            want = _host(mmsa.majority_filter(src, radius, support=s16, **kw)), _host(s16).astype(np.uint32)
            _run(src, radius, want, ("plain", cfg, where, half), **kw)
            _run(src, radius, want, ("a table of ones", cfg, where, half), guide=guide, range_weights=np.ones(766, dtype=np.int64), **kw)


def test_every_image_of_a_batch_equals_its_own_single_image_result():
    import mmsa
    name = "three of 70x90 radius 3"
    maps, guide, weights = VR.inputs_of(name)
    kw = dict(sigma=8.0, **MR.CONFIGS["C25"])
    both = mmsa.vote_filter(_dev(maps), 3, guide=_dev(guide), weights=_dev(weights), **kw)
    for b in range(3):
        one = mmsa.vote_filter(_dev(maps[b:b + 1]), 3, guide=_dev(guide[b:b + 1]), weights=_dev(weights[b:b + 1]), **kw)
        _same(_host(one)[0], _host(both)[b], ("image", b))
        _same(_host(one)[0], VR.want_of(name)[0][b], ("image against the restatement", b))


def test_a_new_out_and_the_same_bytes_on_every_run():
    import mmsa
    name, = [c.name for c in VR.CASES if c.name.startswith("stack 130x200 radius 8 ")]
    maps, guide, weights = VR.inputs_of(name)
    src, g, w = _dev(maps), _dev(guide), _dev(weights)
    first = mmsa.vote_filter(src, 8, **_keywords(name, g, w))
    assert first.dtype == torch.uint8 and first.device.type == "cuda"
    _same(_host(first), VR.want_of(name)[0], "support=None")
    for _ in range(2):
        assert _host(mmsa.vote_filter(src, 8, **_keywords(name, g, w))).tobytes() == _host(first).tobytes()


def test_a_captured_graph_replayed_on_changed_input_equals_the_eager_result():
    import mmsa
    role = MR.roles(**MR.CONFIGS["any"])
    a, b = MR.stack(67, 131, 2), MR.stack(67, 131, 3)                               # two inputs of one shape
    ga, gb = VR.guide_of(a, 3, (5, 3), 1), VR.guide_of(b, 3, (5, 3), 2)
    wa, wb = VR.weights_of(a.shape, 3), VR.weights_of(b.shape, 4)
    src, guide, w = _dev(a), _dev(ga), _dev(wa)
    out, support = _canary(a.shape, np.uint8), _canary(a.shape, np.uint32)
    kw = dict(guide=guide, sigma=8.0, weights=w, where="all", half=True, out=out, support=support, **MR.CONFIGS["any"])
    mmsa.vote_filter(src, 2, **kw)                                                   # the tables go up before the capture
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        before = torch.cuda.memory_allocated()                                       # read inside: entering a capture allocates on its own
        assert mmsa.vote_filter(src, 2, **kw) is out                                 # nothing allocated, nothing uploaded
        assert torch.cuda.memory_allocated() == before
    src.copy_(_dev(b))
    guide.copy_(_dev(gb))
    w.copy_(_dev(wb))
    out.fill_(CANARY_U8)
    graph.replay()
    torch.cuda.synchronize()
    want = VR.vote_batch(b, role, 2, True, True, gb, VR.range_table(8.0, 3), VR.wq_of(wb))
    _same(_host(out), want[0], "replay: out")
    _same(_host(support), want[1], "replay: support")
    eager = mmsa.vote_filter(_dev(b), 2, guide=_dev(gb), sigma=8.0, weights=_dev(wb), where="all", half=True, **MR.CONFIGS["any"])
    _same(_host(eager), _host(out), "replay against eager")


def test_aliases_are_refused_on_the_device():
    import mmsa
    m = _dev(MR.stack(9, 64, 1))
    with pytest.raises(RuntimeError, match="out is the map; a stencil cannot run in place"):
        mmsa.vote_filter(m, out=m.view(m.shape))
    plane = torch.zeros(m.numel(), dtype=torch.uint32, device=DEV)
    out = plane.view(torch.uint8)[:m.numel()].view(m.shape)
    with pytest.raises(RuntimeError, match="support aliases a map"):
        mmsa.vote_filter(m, out=out, support=plane.view(m.shape))
    with pytest.raises(RuntimeError, match="support aliases a map"):
        mmsa.vote_filter(plane.view(torch.uint8)[:m.numel()].view(m.shape), support=plane.view(m.shape))
    g = torch.zeros(7, 9, 64, dtype=torch.uint8, device=DEV)
    w = torch.zeros(7, 9, 64, dtype=torch.float32, device=DEV)
    with pytest.raises(RuntimeError, match="out or support aliases the guide or the weights"):
        mmsa.vote_filter(m, guide=g, sigma=8.0, out=g)
    with pytest.raises(RuntimeError, match="out or support aliases the guide or the weights"):
        mmsa.vote_filter(m, weights=w, support=w.view(torch.uint32))
    with pytest.raises(RuntimeError, match="guide is on cpu"):
        mmsa.vote_filter(m, guide=torch.zeros(7, 9, 64, dtype=torch.uint8), sigma=8.0)
