"""Run-length tables without a GPU: the numpy restatement of tests/run_length_ref.py held to independent statements, the host helpers (runs of one value,
the uncompressed COCO RLE, its area and box) against the masks and the records of the segment table, hand-made cases, the refusals, the exports, and -- for
every input of tests/test_run_length_gpu.py -- the predicted run count against the capacity its test uses."""
import os
import re

import numpy as np
import pytest

from tests import run_length_ref as RR
from tests import segment_table_ref as SR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- 1. the restatement against independent statements

@pytest.mark.parametrize("order", RR.ORDERS)
@pytest.mark.parametrize("kind,H,W", [("one", 67, 131), ("noise", 31, 63), ("noise25", 31, 63), ("blocky", 67, 131), ("vstripes", 65, 63), ("hstripes", 63, 65),
                                      ("seams", 67, 131), ("ids", 67, 131), ("one", 1, 1), ("seams", 1, 131), ("seams", 67, 1)])
def test_restatement_rebuilds_the_map(kind, H, W, order):
    m = RR.image(kind, H, W)
    flat = RR.flat_of(m, order)
    starts, lengths, values = RR.runs(m, order)
    assert starts[0] == 0 and (lengths > 0).all() and lengths.sum() == H * W and np.array_equal(starts[1:], np.cumsum(lengths)[:-1])
    assert np.array_equal(np.repeat(values, lengths), flat)                    # the runs rebuild the map
    assert (values[1:] != values[:-1]).all()                                   # neighbouring runs differ: none could be merged
    assert len(starts) == RR.count_of(kind, H, W, order)
    count, s, v = RR.table([m], order, len(starts) + 2)
    assert count.tolist() == [len(starts)] and np.array_equal(s[0, :-2], starts) and (s[0, -2:] == -7).all() and (v[0, -2:] == -7).all()
    assert np.array_equal(RR.decode(m, order, len(starts), -5), m)


def test_the_maps_are_what_their_names_say():
    for H, W in RR.SHAPES:
        for order in RR.ORDERS:
            assert RR.count_of("one", H, W, order) == 1                        # one run, continuing over every line end
            assert RR.count_of("noise", H, W, order) == H * W                  # every pixel is a run
    H, W = 67, 131
    nv, nh = -(-W // 2), -(-H // 2)      # stripes two pixels wide, of the values 0..4 in turn: a line whose last stripe has the first one's value runs on
    assert (nv - 1) % 5 == 0 and (nh - 1) % 5 != 0
    assert RR.count_of("vstripes", H, W, "row") == H * nv - (H - 1) == 4356 and RR.count_of("vstripes", H, W, "column") == nv == 66
    assert RR.count_of("hstripes", H, W, "column") == W * nh == 4454 and RR.count_of("hstripes", H, W, "row") == nh == 34
    for H, W in RR.MANY + RR.EDGES:                                            # line ends that continue into the next line, and line ends that do not
        m = RR.image("seams", H, W)
        row, col = m[:-1, -1] == m[1:, 0], m[-1, :-1] == m[0, 1:]
        assert row[0::2].all() and not row[1::2].any() and col[0::2].all() and not col[1::2].any()
    ids = RR.image("ids", 67, 131)
    assert ids.dtype == np.int32 and (ids == -1).any() and ids.max() > 1 << 16


# ---- 2. the host helpers against the masks and the records of the segment table

@pytest.mark.parametrize("kind,H,W", [("blocky", 67, 131), ("special", 67, 131), ("blobs", 31, 63), ("one", 5, 9)])
def test_coco_rle_of_every_id_of_a_segment_table(kind, H, W):
    import mmsa
    n, ids, rec = SR.table(np.minimum(SR.image(kind, H, W), SR.C), SR.image_roots(kind, H, W))
    runs = RR.runs(ids, "column")
    assert n > 0
    for k in range(n):
        rle = mmsa.coco_rle_of(*runs, k, H, W)
        assert rle["size"] == [H, W] and all(isinstance(c, int) for c in rle["counts"]) and sum(rle["counts"]) == H * W
        assert all(c > 0 for c in rle["counts"][1:])                           # only the leading count may be 0
        assert np.array_equal(RR.rle_mask(rle), ids == k)
        assert mmsa.rle_area_of(rle) == rec[k, SR.AREA]
        assert mmsa.rle_bbox_of(rle) == [rec[k, SR.X0], rec[k, SR.Y0], rec[k, SR.X1] - rec[k, SR.X0] + 1, rec[k, SR.Y1] - rec[k, SR.Y0] + 1]
        s, l = mmsa.runs_of_value(*runs, k)
        assert l.sum() == rec[k, SR.AREA] and s[0] == np.flatnonzero(ids.T.ravel() == k)[0] and (np.diff(s) > l[:-1]).all()      # ascending, never adjacent
    if (ids == -1).any():
        assert np.array_equal(RR.rle_mask(mmsa.coco_rle_of(*runs, -1, H, W)), ids == -1)
    assert mmsa.coco_rle_of(*runs, n + 5, H, W) == {"size": [H, W], "counts": [H * W]} and mmsa.rle_bbox_of({"size": [H, W], "counts": [H * W]}) == [0, 0, 0, 0]


def test_hand_made_masks():
    import mmsa
    H, W = 3, 4                          # column-major index = x * 3 + y
    m = np.array([[1, 0, 0, 2],
                  [1, 0, 2, 2],
                  [0, 2, 2, 2]])
    runs = RR.runs(m, "column")
    assert runs[0].tolist() == [0, 2, 5, 6, 7] and runs[1].tolist() == [2, 3, 1, 1, 5] and runs[2].tolist() == [1, 0, 2, 0, 2]
    one = mmsa.coco_rle_of(*runs, 1, H, W)                                     # a mask that starts at index 0: a leading 0
    assert one == {"size": [3, 4], "counts": [0, 2, 10]} and mmsa.rle_area_of(one) == 2 and mmsa.rle_bbox_of(one) == [0, 0, 1, 2]
    two = mmsa.coco_rle_of(*runs, 2, H, W)                                     # a mask that ends at H * W: no trailing entry; its last run crosses column ends
    assert two == {"size": [3, 4], "counts": [5, 1, 1, 5]} and mmsa.rle_area_of(two) == 6 and mmsa.rle_bbox_of(two) == [1, 0, 3, 3]
    zero = mmsa.coco_rle_of(*runs, 0, H, W)                                    # the run 2..4 crosses the end of column 0
    assert zero == {"size": [3, 4], "counts": [2, 3, 1, 1, 5]} and mmsa.rle_bbox_of(zero) == [0, 0, 3, 3] and np.array_equal(RR.rle_mask(zero), m == 0)
    s, l = mmsa.runs_of_value(*runs, 2)
    assert s.tolist() == [5, 7] and l.tolist() == [1, 5]
    full = mmsa.coco_rle_of(*RR.runs(np.ones((3, 4), dtype=np.uint8), "column"), 1, 3, 4)
    assert full == {"size": [3, 4], "counts": [0, 12]} and mmsa.rle_bbox_of(full) == [0, 0, 4, 3]
    assert mmsa.rle_bbox_of({"size": [3, 4], "counts": [4, 1, 7]}) == [1, 1, 1, 1] and mmsa.rle_area_of({"size": [3, 4], "counts": [12]}) == 0


# ---- 3. refusals and exports

class _Words:
    """The device words a RunTable reads on the host, without a device."""

    def __init__(self, a):
        self.a = np.asarray(a)

    def __getitem__(self, k):
        return _Words(self.a[k])

    def __gt__(self, v):
        return _Words(self.a > v)

    def any(self):
        return _Words(self.a.any())

    def item(self):
        return self.a.item()

    def cpu(self):
        return self

    def numpy(self):
        return self.a


def test_refusals():
    import mmsa
    from mmsa.evaluate import RunTable, SegmentTable
    m = RR.image("seams", 5, 7)
    with pytest.raises(ValueError, match="COCO's RLE is the column-major mask.*order='column'.*order='row'"):
        mmsa.coco_rle_of(*RR.runs(m, "row"), 1, 5, 7, order="row")
    with pytest.raises(ValueError, match="the runs do not cover the 5 x 8 = 40 pixels"):
        mmsa.coco_rle_of(*RR.runs(m, "column"), 1, 5, 8)
    with pytest.raises(ValueError, match="three integer arrays of one length"):
        mmsa.runs_of_value(np.zeros(2, dtype=np.int64), np.ones(3, dtype=np.int64), np.zeros(2, dtype=np.int64), 0)
    for order in RR.ORDERS:                                                    # host() on an overflowed table is never silent
        count, starts, values = RR.table([m, m], order, 4)
        rt = RunTable(_Words(count), _Words(starts), _Words(values), order, (2, 5, 7), 4)
        assert rt.overflow() is True and count[0] > 4
        with pytest.raises(RuntimeError, match=rf"image 1 has {count[1]} runs and the table 4 rows: the last {count[1] - 4} were dropped.*capacity="):
            rt.host(1)
        count, starts, values = RR.table([m, m], order, 35)
        rt = RunTable(_Words(count), _Words(starts), _Words(values), order, (2, 5, 7), 35)
        got = rt.host(0)
        assert rt.overflow() is False and all(np.array_equal(a, b) and a.dtype == np.int64 for a, b in zip(got, RR.runs(m, order)))
        with pytest.raises(ValueError, match="b = 2; an image index 0..1"):
            rt.host(2)
    with pytest.raises(ValueError, match="mmsa.RunTable: order = 'diagonal'"):
        RunTable(None, None, None, "diagonal", (1, 2, 2), 4)
    for bad in (0, -3, 2.5, "9", True, 1 << 31):
        with pytest.raises(ValueError, match="capacity = .*a positive number of runs per image"):
            RunTable(None, None, None, "row", (1, 2, 2), bad)
        with pytest.raises(ValueError, match="mmsa.SegmentTable: capacity = .*a positive number of runs per image"):
            SegmentTable(num_classes=5, runs="column", run_capacity=bad)
    with pytest.raises(ValueError, match="mmsa.SegmentTable: order = 'both'"):
        SegmentTable(num_classes=5, runs="both")
    for runs in (None, "row"):                                                 # masks need the column-major runs: refused before anything is read
        with pytest.raises(ValueError, match=rf"segments_info\(masks=True\) reads the column-major runs of ids.*runs='column' \(this one has runs={runs!r}\)"):
            SegmentTable(num_classes=5, runs=runs).segments_info(0, masks=True)
    st = SegmentTable(num_classes=5, runs="column", run_capacity=77)
    assert st.run_order == "column" and st.runs is None and SegmentTable(num_classes=5).run_order is None
    with pytest.raises(RuntimeError, match="nothing was filled yet"):
        st.segments_info(0, masks=True)
    with pytest.raises(RuntimeError, match="map must be a uint8 .* or int32 .* tensor, got ndarray"):
        mmsa.run_lengths(np.zeros((1, 4, 4), dtype=np.uint8))
    with pytest.raises(ValueError, match="order = 'F'"):
        mmsa.run_lengths(None, order="F")
    with pytest.raises(RuntimeError, match="table= takes an mmsa.evaluate.RunTable, got int"):
        mmsa.run_lengths(None, table=3)
    with pytest.raises(RuntimeError, match="table takes an mmsa.evaluate.RunTable, got NoneType"):
        mmsa.run_decode(None)


def test_exports_and_constants():
    import mmsa
    from mmsa import evaluate as E
    for name in ("RunTable", "run_lengths", "run_decode", "runs_of_value", "coco_rle_of", "rle_area_of", "rle_bbox_of"):
        assert getattr(mmsa, name) is getattr(E, name) and name in mmsa.__all__
    hdr, ver = (open(os.path.join(ROOT, "include", f)).read() for f in ("mmsa.h", "mmsa_version.h"))
    for name in ("mmsa_run_lengths_u8", "mmsa_run_lengths_i32", "mmsa_run_lengths_block", "mmsa_run_decode_i32"):
        assert f"int {name}(" in hdr and name in ver and name in mmsa.lib.SIGNATURES and hasattr(mmsa.lib.raw, name)
    assert mmsa.lib.SIGNATURES["mmsa_run_lengths_u8"] == mmsa.lib.SIGNATURES["mmsa_run_lengths_i32"] and len(mmsa.lib.SIGNATURES["mmsa_run_lengths_u8"]) == 11
    assert len(mmsa.lib.SIGNATURES["mmsa_run_decode_i32"]) == 11 and mmsa.lib.version() == 114
    block = mmsa.lib.raw.mmsa_run_lengths_block
    assert [block(k) for k in range(5)] == [E.RUNS_BLOCK, E.RUNS_TILE, E.SCAN_LANES, E.SCAN_TRIP, -1] == [RR.BLOCK, RR.TILE, RR.SCAN_LANES, RR.SCAN_TRIP, -1]
    assert E.default_run_capacity(31, 63) == 4096 == RR.default_capacity(31, 63) and E.default_run_capacity(1080, 1920) == 259200 == RR.default_capacity(1080, 1920)
    for H, W in RR.SHAPES + [RR.LARGE]:
        assert E.run_units(H, W) == RR.units(H, W) >= 1 and E.run_scratch_words(3, H, W, "row") == 3 * RR.units(H, W)
        assert E.run_scratch_words(3, H, W, "column") == 3 * RR.units(H, W) + 3 * H * W      # the transposed int32 map behind the unit counts
        assert E.run_scratch_words(3, H, W, "column", 1) == 3 * RR.units(H, W) + -(-3 * H * W // 4)
    # The column order is the row order of the transposed map (the form with one scan unit per column of a 64-row tile lost to it by more than the spread,
    # profiles/run_length.txt), so in either order the scan units are blocks: the large map has more of them than the scan workgroup has lanes and than one
    # trip of the scan takes, and the two middle shapes have several blocks and several ragged transpose tiles in each axis.
    assert RR.units(*RR.LARGE) > RR.SCAN_TRIP > RR.SCAN_LANES
    for H, W in RR.MANY:
        assert RR.units(H, W) > 1 and H > RR.TILE and W > RR.TILE and H % RR.TILE and W % RR.TILE


def test_argument_limits_are_refused_before_any_launch():
    """The library's own refusals: every one returns MMSA_ERR_ARG with a message and launches nothing, so they need no device."""
    import mmsa
    raw, p = mmsa.lib.raw, 4096          # a non-null pointer that is never followed
    ok = dict(B=1, H=4, W=4, order=1, capacity=8)
    for change, words in ((dict(order=2), "order = 2"), (dict(order=-1), "order = -1"), (dict(capacity=0), "capacity = 0"), (dict(B=65536), "bad map size"),
                          (dict(H=0), "bad map size"), (dict(H=1 << 16, W=1 << 15), "bad map size"), (dict(B=3, capacity=1 << 30), "B \\* capacity below 2\\^31")):
        a = dict(ok, **change)
        for name in ("mmsa_run_lengths_u8", "mmsa_run_lengths_i32"):
            assert getattr(raw, name)(p, a["B"], a["H"], a["W"], a["order"], a["capacity"], p + 64, p + 128, p + 192, p + 256, None) == -1
            assert re.search(words, mmsa.lib.last_error()), (name, change, mmsa.lib.last_error())
        assert raw.mmsa_run_decode_i32(p, p + 64, p + 128, a["B"], a["H"], a["W"], a["order"], a["capacity"], -1, p + 192, None) == -1
        assert re.search(words, mmsa.lib.last_error()), (change, mmsa.lib.last_error())
    for k in range(5):                   # a null pointer in every place
        ptrs = [p + 64 * i for i in range(5)]
        ptrs[k] = None
        assert raw.mmsa_run_lengths_u8(ptrs[0], 1, 4, 4, 0, 8, ptrs[1], ptrs[2], ptrs[3], ptrs[4], None) == -1 and "are required" in mmsa.lib.last_error()
    for k in range(4):
        ptrs = [p + 64 * i for i in range(4)]
        ptrs[k] = None
        assert raw.mmsa_run_decode_i32(ptrs[0], ptrs[1], ptrs[2], 1, 4, 4, 0, 8, -1, ptrs[3], None) == -1 and "are required" in mmsa.lib.last_error()


# ---- 4. the inputs of the GPU tests, predicted

def test_every_gpu_input_has_the_overflow_its_test_expects():
    over = []
    for kind, H, W, capacity, overflows in RR.CASES:
        for order, expected in zip(RR.ORDERS, overflows):
            n, cap = RR.count_of(kind, H, W, order), RR.capacity_of(kind, H, W, capacity, order)
            assert 1 <= n <= H * W and cap >= 1 and (n > cap) == expected, (kind, H, W, capacity, order, n, cap)
        over += [(kind, capacity)] * any(overflows)
    assert over == [("noise", "count-1"), ("noise", 1), ("seams", "count-1"), ("seams", 1), ("noise", None)]


def test_reference_counts_of_the_shared_maps():
    """Run counts pinned from these seeds, (row, column)."""
    want = {("blocky", 67, 131): (335, 393), ("blocky", 130, 200): (883, 2826), ("seams", 67, 131): (5894, 5905), ("ids", 67, 131): (464, 886),
            ("noise25", 31, 63): (1869, 1859)}
    got = {k: (RR.count_of(*k, "row"), RR.count_of(*k, "column")) for k in want}
    assert got == want
