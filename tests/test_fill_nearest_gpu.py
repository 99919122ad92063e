"""The nearest-label fill on the GPU (csrc/fill.hip): `out` and `d2` of mmsa.fill_nearest against the numpy restatement of tests/fill_nearest_ref.py, byte for
byte, into buffers pre-filled with a canary -- degenerate axes, every alignment class of the 64-column tile, a lane's piece of 1, 2 and 3 pixels, the group of
four rows, row distances beyond 255, maps without holes and of holes alone, the disc's edge around one source, the scan across lanes and waves, the tie
patterns, noise with inert bytes, a batch, in place, a caller's scratch, no d2, and nearest= of suppress_small / select_segments."""
import numpy as np
import pytest
import torch

from tests import components_ref as CR
from tests import fill_nearest_ref as FR

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


def _run(maps, cap, what, hole=FR.HOLES, inert=FR.INERT, want=None, **kw):
    """One call into canary-filled out and d2 -> both equal the restatement."""
    import mmsa
    src = _dev(maps)
    out = _canary(maps.shape, np.uint8)
    d2 = _canary(maps.shape, np.uint16)
    got = mmsa.fill_nearest(src, hole=hole, inert=inert, cap=cap, out=out, d2=d2, **kw)
    assert got is out and np.array_equal(_host(src), maps), what       # the map itself is read only
    want = FR.fill_batch(maps, hole, inert, cap) if want is None else want
    _same(_host(out), want[0], (what, "out"))
    _same(_host(d2), want[1], (what, "d2"))
    return out, d2


@pytest.mark.parametrize("name", [c.name for c in FR.CASES])
def test_every_case_equals_the_restatement(name):
    _run(FR.maps_of(name), FR.CASE[name].cap, name, want=FR.want_of(name))


@pytest.mark.parametrize("W,x", [(256, 0), (256, 255), (512, 0), (512, 511)])
def test_a_row_with_one_source_at_an_end_of_the_scan(W, x):
    """The scan over the lanes of a row (csrc/row_scan.h) with ONE marked index in the whole row, every other row without any: the source in the first piece
    of the first wave and in the last piece of the last wave (one pixel per lane at 256 columns, two at 512); image 1 has it at the other end."""
    maps = np.stack([FR.one_source(5, W, 2, x), FR.one_source(5, W, 0, W - 1 - x, value=3)])
    for cap in (3, 255):
        _run(maps, cap, (W, x, cap))


def test_no_hole_copies_and_all_holes_stay():
    for H, W in ((1, 1), (5, 70), (67, 131)):
        out, d2 = _run(FR.maps_of(f"stack {H}x{W} cap 255"), 255, (H, W), want=FR.want_of(f"stack {H}x{W} cap 255"))
        m = FR.maps_of(f"stack {H}x{W} cap 255")
        assert np.array_equal(_host(out)[:2], m[:2]) and not _host(d2)[0].any() and (_host(d2)[1] == FR.FAR).all()


def test_one_hole_byte_and_no_inert_byte():
    """The defaults: hole = 255 alone; 250 and 254 are then classes like any other, and sources."""
    m = FR.maps_of("stack 67x131 cap 20")
    _run(m, 20, "defaults", hole=255, inert=())
    _run(m, 7, "a list of one, an inert list", hole=[250], inert=[255, 254])


def test_in_place():
    import mmsa
    name = "stack 67x131 cap 20"
    m = _dev(FR.maps_of(name))
    d2 = _canary(tuple(m.shape), np.uint16)
    assert mmsa.fill_nearest(m, hole=FR.HOLES, inert=FR.INERT, cap=20, out=m, d2=d2) is m
    _same(_host(m), FR.want_of(name)[0], "in place: out")
    _same(_host(d2), FR.want_of(name)[1], "in place: d2")


def test_a_callers_scratch_larger_than_needed_and_no_d2():
    import mmsa
    name = "batch of two"
    m, want = FR.maps_of(name), FR.want_of(name)
    scratch = _canary((m.size + 1000,), np.uint16)
    _run(m, FR.CASE[name].cap, "scratch=", want=want, scratch=scratch)
    assert (_host(scratch)[m.size:] == CANARY_U16).all(), "the plane ends at B * H * W"
    out = mmsa.fill_nearest(_dev(m), hole=FR.HOLES, inert=FR.INERT, cap=FR.CASE[name].cap, scratch=scratch)      # d2=None, a new out
    assert out.dtype == torch.uint8 and out.device.type == "cuda"
    _same(_host(out), want[0], "d2=None")
    with pytest.raises(RuntimeError, match="scratch and d2 are two planes"):
        mmsa.fill_nearest(_dev(m), d2=scratch[:m.size].view(m.shape), scratch=scratch)


def test_the_same_bytes_on_every_run():
    import mmsa
    m = _dev(FR.maps_of("partial 300x520 0.05% cap 32"))
    first = _host(mmsa.fill_nearest(m, hole=FR.HOLES, inert=FR.INERT, cap=32)).tobytes()
    for _ in range(3):
        assert _host(mmsa.fill_nearest(m, hole=FR.HOLES, inert=FR.INERT, cap=32)).tobytes() == first


def _class_maps():
    rng = np.random.default_rng(77)
    m = np.stack([CR.blocky(rng, 67, 131, 5, 3, 9), rng.integers(0, 5, size=(67, 131)).astype(np.uint8)])
    m[0, 20:24, 30:60] = 255          # an ignored region that was there before
    m[rng.random(m.shape) < 0.02] = 9      # and specks of a byte beyond the classes
    return m


def test_suppress_small_nearest_is_the_composition():
    import mmsa
    m, C = _class_maps(), 5
    d = _dev(m)
    plain = mmsa.suppress_small(d, 6, num_classes=C, fill=254)
    assert _host(mmsa.suppress_small(d, 6, num_classes=C, fill=254, nearest=None)).tobytes() == _host(plain).tobytes()
    assert _host(plain).tobytes() == CR.suppress(m, C, 6, 8, fill=254).tobytes() and (_host(plain) == 254).any()
    for cap in (2, 32):
        got = mmsa.suppress_small(d, 6, num_classes=C, fill=254, nearest=cap)
        want = FR.fill_batch(_host(plain), 254, (), cap)[0]
        _same(_host(got), want, ("suppress_small", cap))
        assert (want != _host(plain)).any() and (want == 255).any()                  # holes were filled, and the 255 of before was kept (a source)
    inplace = d.clone()
    assert mmsa.suppress_small(inplace, 6, num_classes=C, fill=254, out=inplace, nearest=32) is inplace and _host(inplace).tobytes() == _host(got).tobytes()
    # fill=255: the ignored region of before is filled as well
    got = _host(mmsa.suppress_small(d, 6, num_classes=C, nearest=32))
    _same(got, FR.fill_batch(CR.suppress(m, C, 6, 8, fill=255), 255, (), 32)[0], "fill=255")
    assert not (got[0, 20:24, 30:60] == 255).any()


def test_select_segments_nearest_is_the_composition():
    import mmsa
    m, C = _class_maps(), 5
    d = _dev(m)
    st = mmsa.segment_table(d, num_classes=C, void=True)
    keep = st.keep(min_area=6)
    plain = mmsa.select_segments(d, st, keep, fill=200)
    assert _host(mmsa.select_segments(d, st, keep, fill=200, nearest=None)).tobytes() == _host(plain).tobytes() and (_host(plain) == 200).any()
    for cap in (2, 32):
        got = mmsa.select_segments(d, st, keep, fill=200, nearest=cap)
        want = FR.fill_batch(_host(plain), 200, (), cap)[0]
        _same(_host(got), want, ("select_segments", cap))
        assert (want != _host(plain)).any()
    inplace = d.clone()
    assert mmsa.select_segments(inplace, st, keep, fill=200, out=inplace, nearest=32) is inplace and _host(inplace).tobytes() == _host(got).tobytes()
