"""The majority filter on the GPU (csrc/majority.hip): `out` and `support` of mmsa.majority_filter against the numpy restatement of tests/majority_ref.py, byte
for byte, into buffers pre-filled with a canary -- degenerate axes, an image thinner than the halo, 63 / 64 / 65 columns, the row counts around the three tile
heights, several tiles on both sides of either tile-height switch, many ragged tiles in a batch, noise over 3, 25 and 200 values, the patchy map with two hole
bytes and an inert byte, a one-value map, an all-hole map, a solid hole block, both targets with and without the half rule -- and identities on device results."""
import numpy as np
import pytest
import torch

from tests import majority_ref as MR

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CANARY_U8, CANARY_U16 = 0xA5, 0xBEEF


def _dev(a):
    return torch.from_numpy(np.array(a)).to(DEV)      # a copy: the cached cases are read-only


def _host(t):
    return t.cpu().numpy()


def _canary(shape, dtype):
    return _dev(np.full(shape, CANARY_U8 if dtype == np.uint8 else CANARY_U16, dtype=dtype))


def _same(got, want, what):
    bad = np.argwhere(got != want)
    assert got.shape == want.shape and bad.size == 0, (what, len(bad), bad[:5].tolist(), got[tuple(bad[0])], want[tuple(bad[0])])


def _run(src, maps, radius, config, where, half, want, what):
    """One call into canary-filled out and support -> both equal `want`."""
    import mmsa
    out, support = _canary(maps.shape, np.uint8), _canary(maps.shape, np.uint16)
    got = mmsa.majority_filter(src, radius, where=where, half=half, out=out, support=support, **MR.CONFIGS[config])
    assert got is out, what
    _same(_host(out), want[0], (what, where, half, "out"))
    _same(_host(support), want[1], (what, where, half, "support"))
    return out, support


@pytest.mark.parametrize("name", [c.name for c in MR.CASES])
def test_every_case_equals_the_restatement(name):
    c, maps = MR.CASE[name], MR.maps_of(name)
    src = _dev(maps)
    for where, half in MR.MODES:
        _run(src, maps, c.radius, c.config, where, half, MR.want_of(name, where, half), name)
    assert np.array_equal(_host(src), maps), name       # the map itself is read only


def test_every_image_of_a_batch_equals_its_own_single_image_result():
    import mmsa
    name = "three of 70x90 radius 3"
    maps = MR.maps_of(name)
    both = mmsa.majority_filter(_dev(maps), 3, **MR.CONFIGS["C25"])
    for b in range(3):
        one = mmsa.majority_filter(_dev(maps[b:b + 1]), 3, **MR.CONFIGS["C25"])
        _same(_host(one)[0], _host(both)[b], ("image", b))
        _same(_host(one)[0], MR.want_of(name)[0][b], ("image against the restatement", b))


def test_no_support_and_a_new_out():
    import mmsa
    name = "stack 67x131 radius 2 any"
    out = mmsa.majority_filter(_dev(MR.maps_of(name)), 2, **MR.CONFIGS["any"])
    assert out.dtype == torch.uint8 and out.device.type == "cuda"
    _same(_host(out), MR.want_of(name)[0], "support=None")


def test_holes_only_without_a_hole_byte_is_the_input():
    import mmsa
    m = MR.noise(67, 131, 9, 25, 0.0, 0.02)                                         # 25-value noise and the inert byte; 250 is the hole byte, and absent
    for r in (1, 9, 17):
        out, support = _canary(m[None].shape, np.uint8), _canary(m[None].shape, np.uint16)
        mmsa.majority_filter(_dev(m[None]), r, num_classes=25, hole=250, where="holes", out=out, support=support)
        assert np.array_equal(_host(out)[0], m) and not _host(support).any()


def test_a_one_value_map_gives_itself_and_counts_its_windows():
    import mmsa
    for r, (H, W) in ((2, (70, 131)), (9, (40, 70)), (17, (70, 70))):
        m = np.full((1, H, W), 11, dtype=np.uint8)
        out, support = _canary(m.shape, np.uint8), _canary(m.shape, np.uint16)
        mmsa.majority_filter(_dev(m), r, out=out, support=support)
        s = _host(support)[0]
        assert np.array_equal(_host(out), m) and (s[r:H - r, r:W - r] == (2 * r + 1) ** 2).all()
        assert s[0, 0] == s[0, -1] == s[-1, 0] == s[-1, -1] == (r + 1) ** 2 and s.max() == (2 * r + 1) ** 2
        y, x = np.arange(H)[:, None], np.arange(W)[None, :]
        want = (np.minimum(y + r, H - 1) - np.maximum(y - r, 0) + 1) * (np.minimum(x + r, W - 1) - np.maximum(x - r, 0) + 1)
        _same(s.astype(np.int64), want, ("support", r))


def test_out_is_the_input_wherever_support_is_zero_or_the_pixel_is_inert():
    import mmsa
    name = "stack 130x200 radius 3 C25"
    maps, role = MR.maps_of(name), MR.role_of(name)
    for where, half in MR.MODES:
        out, support = _canary(maps.shape, np.uint8), _canary(maps.shape, np.uint16)
        mmsa.majority_filter(_dev(maps), 3, where=where, half=half, out=out, support=support, **MR.CONFIGS["C25"])
        o, s = _host(out), _host(support)
        stay = (s == 0) | (role[maps] == MR.INERT_ROLE)
        assert stay.any() and (~stay).any() and np.array_equal(o[stay], maps[stay]), (where, half)
        assert not s[role[maps] == MR.INERT_ROLE].any() and (role[o[o != maps]] == MR.VOTER).all()      # a pixel changes to a voter's value only


def test_the_same_bytes_on_every_run():
    import mmsa
    m = _dev(MR.maps_of("two of 600x900 radius 2"))
    first = _host(mmsa.majority_filter(m, 2, **MR.CONFIGS["C25"])).tobytes()
    for _ in range(2):
        assert _host(mmsa.majority_filter(m, 2, **MR.CONFIGS["C25"])).tobytes() == first


def test_a_captured_graph_replayed_on_changed_input_equals_the_eager_result():
    import mmsa
    a, b = MR.maps_of("stack 67x131 radius 2 any"), MR.maps_of("stack 67x131 radius 3 any")      # two inputs of one shape
    src = _dev(a)
    out, support = _canary(a.shape, np.uint8), _canary(a.shape, np.uint16)
    kw = dict(where="all", half=True, out=out, support=support, **MR.CONFIGS["any"])
    mmsa.majority_filter(src, 2, **kw)                                               # the role table goes up before the capture
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        assert mmsa.majority_filter(src, 2, **kw) is out                             # nothing allocated, nothing uploaded
    src.copy_(_dev(b))
    out.fill_(CANARY_U8)
    graph.replay()
    torch.cuda.synchronize()
    want = MR.majority_batch(b, MR.roles(**MR.CONFIGS["any"]), 2, True, True)
    _same(_host(out), want[0], "replay: out")
    _same(_host(support), want[1], "replay: support")
    eager = mmsa.majority_filter(_dev(b), 2, where="all", half=True, **MR.CONFIGS["any"])
    _same(_host(eager), _host(out), "replay against eager")


def test_aliases_are_refused_on_the_device():
    import mmsa
    m = _dev(MR.maps_of("stack 9x64 radius 1 C25"))
    with pytest.raises(RuntimeError, match="out is the map; a stencil cannot run in place"):
        mmsa.majority_filter(m, out=m.view(m.shape))
    plane = torch.zeros(m.numel(), dtype=torch.uint16, device=DEV)
    out = plane.view(torch.uint8)[:m.numel()].view(m.shape)
    with pytest.raises(RuntimeError, match="support aliases a map"):
        mmsa.majority_filter(m, out=out, support=plane.view(m.shape))
