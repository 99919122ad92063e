"""Run-length tables on the GPU (csrc/runs.hip): count, starts and values against the numpy restatement of tests/run_length_ref.py, byte for byte.  Everything
is integers: every comparison is equality.  The shapes are the smallest at which each mechanism can fail: one pixel, one row, one column, one below, at and
one above the row block and the column tile in each axis, more scan units than the scan workgroup has lanes and than one trip of the scan takes; the maps are
one run, every pixel a run, blocks, the stripes that are the worst case of one order and the best of the other, line ends that continue and line ends that do
not, and ids with -1.  Every input is listed in run_length_ref.CASES, where tests/test_run_length_cpu.py predicts its run count."""
import numpy as np
import pytest
import torch

from tests import run_length_ref as RR
from tests import segment_table_ref as SR

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CANARY = -7


def _dev(a):
    return torch.from_numpy(np.array(a)).to(DEV)      # a copy: the cached cases are read-only


def _host(t):
    return t.cpu().numpy()


def _case(kind, H, W, capacity="HW", overflows=(False, False)):
    """The image of a listed case: an input that is not in the list has no prediction in the CPU file."""
    assert (kind, H, W, capacity, overflows) in RR.CASES, (kind, H, W, capacity)
    return RR.image(kind, H, W)


def _table(B, H, W, order, capacity):
    """A table whose rows hold the canary: what the launch does not write stays."""
    import mmsa
    t = mmsa.RunTable.empty(B, H, W, order, capacity, DEV)
    t.count.fill_(CANARY), t.starts.fill_(CANARY), t.values.fill_(CANARY)
    return t


def _run(maps, order, capacity, dtype=None):
    import mmsa
    m = np.stack(maps)
    B, H, W = m.shape
    t = _table(B, H, W, order, capacity)
    got = mmsa.run_lengths(_dev(m if dtype is None else m.astype(dtype)), table=t)
    assert got is t and t.shape == (B, H, W) and t.order == order and t.capacity == capacity
    return t


def _same(t, maps, what=None):
    """count, and starts / values with the canary behind the rows that were written."""
    count, starts, values = RR.table(maps, t.order, t.capacity, CANARY)
    assert np.array_equal(_host(t.count), count), what
    assert np.array_equal(_host(t.starts), starts), what
    assert np.array_equal(_host(t.values), values), what


# ---- 1. the table equals the restatement

@pytest.mark.parametrize("order", RR.ORDERS)
@pytest.mark.parametrize("H,W", RR.SHAPES)
def test_every_map_at_every_shape(H, W, order):
    import mmsa
    assert mmsa.lib.raw.mmsa_run_lengths_block(0) == RR.BLOCK and mmsa.lib.raw.mmsa_run_lengths_block(1) == RR.TILE      # the edges are the library's own
    for kind in RR.KINDS:
        m = _case(kind, H, W)
        t = _run([m], order, H * W)
        _same(t, [m], kind)
        n = int(t.count[0])
        assert n == RR.count_of(kind, H, W, order) and (kind != "one" or n == 1) and (kind != "noise" or n == H * W)
        i32 = _run([m], order, H * W, np.int32)                                # the same values as int32: the same table
        assert all(torch.equal(a, b) for a, b in zip((t.count, t.starts, t.values), (i32.count, i32.starts, i32.values))), kind
        assert np.array_equal(_host(mmsa.run_decode(t))[0], m), kind           # the round trip
        s, l, v = t.host(0)
        assert all(np.array_equal(a, b) for a, b in zip((s, l, v), RR.runs(m, order)))


@pytest.mark.parametrize("order", RR.ORDERS)
def test_more_scan_units_than_the_scan_workgroup_has_lanes(order):
    import mmsa
    block = mmsa.lib.raw.mmsa_run_lengths_block
    H, W = RR.LARGE                                                            # in either order a scan unit is a block of the (transposed) map: from the library
    assert -(-H * W // block(0)) > block(3) > block(2)                         # more units than the scan workgroup has lanes, and than one trip takes
    m = _case("noise25", H, W)
    t = _run([m], order, H * W)
    count, starts, values = RR.table([m], order, H * W, CANARY)
    assert count[0] > 2000000 and torch.equal(t.count.cpu(), torch.from_numpy(count))
    assert torch.equal(t.starts.cpu(), torch.from_numpy(starts)) and torch.equal(t.values.cpu(), torch.from_numpy(values))
    assert torch.equal(mmsa.run_decode(t).cpu()[0], torch.from_numpy(m.astype(np.int32)))


@pytest.mark.parametrize("order", RR.ORDERS)
def test_ids_with_minus_one(order):
    import mmsa
    for H, W in RR.MANY + [(RR.TILE + 1, RR.TILE + 1)]:
        m = _case("ids", H, W)
        assert m.dtype == np.int32 and (m == -1).any() and m.max() > 1 << 16
        t = _run([m], order, H * W)
        _same(t, [m])
        assert np.array_equal(_host(mmsa.run_decode(t, fill=-9))[0], m)


@pytest.mark.parametrize("order", RR.ORDERS)
def test_three_different_images_in_a_batch(order):
    import mmsa
    H, W = 50, 70
    maps = [_case(k, H, W) for k in ("blocky", "seams", "one")]
    t = _run(maps, order, H * W)
    _same(t, maps)
    assert _host(t.count).tolist() == [RR.count_of(k, H, W, order) for k in ("blocky", "seams", "one")] and int(t.count[2]) == 1
    assert np.array_equal(_host(mmsa.run_decode(t)), np.stack(maps))
    assert all(np.array_equal(a, b) for a, b in zip(t.host(1), RR.runs(maps[1], order)))


# ---- 2. capacity

@pytest.mark.parametrize("order", RR.ORDERS)
@pytest.mark.parametrize("kind", ["noise", "seams"])
def test_overflow_keeps_the_count_and_the_first_rows(kind, order):
    import mmsa
    H, W = 67, 131
    n = RR.count_of(kind, H, W, order)
    for spec, capacity in (("count-1", n - 1), (1, 1)):
        m = _case(kind, H, W, spec, (True, True))
        assert capacity == RR.capacity_of(kind, H, W, spec, order)
        t = _run([m], order, capacity)
        _same(t, [m], (kind, capacity))                                        # the first `capacity` rows, the true count
        assert _host(t.count).tolist() == [n] and t.overflow() is True
        with pytest.raises(RuntimeError, match=rf"image 0 has {n} runs and the table {capacity} rows.*capacity="):
            t.host(0)
        got = _host(mmsa.run_decode(t, fill=-5))[0]
        assert np.array_equal(got, RR.decode(m, order, capacity, -5)) and (got == -5).sum() == H * W - int(RR.runs(m, order)[0][capacity - 1]) - 1
        roomy = _run([m], order, n)                                            # exactly enough rows: no overflow
        _same(roomy, [m])
        assert roomy.overflow() is False and np.array_equal(_host(mmsa.run_decode(roomy))[0], m)


def test_rows_behind_the_table_stay():
    """starts and values as the first rows of a larger buffer: what lies behind row `capacity` of the LAST image is not the table's, and stays."""
    import mmsa
    H, W = 67, 131
    m = _case("noise", H, W, "count-1", (True, True))
    for order in RR.ORDERS:
        capacity = RR.count_of("noise", H, W, order) - 1
        buf = torch.full((2, capacity + 64), CANARY, dtype=torch.int32, device=DEV)
        t = mmsa.RunTable(torch.zeros(1, dtype=torch.int32, device=DEV), buf[0, :capacity].view(1, capacity), buf[1, :capacity].view(1, capacity), order,
                          (1, H, W), capacity)
        mmsa.run_lengths(_dev(m[None]), table=t)
        _same(t, [m])
        assert (_host(buf)[:, capacity:] == CANARY).all() and int(t.count[0]) == capacity + 1


def test_default_capacity_and_a_new_table():
    import mmsa
    H, W = 130, 200
    m = _case("blocky", H, W, None)
    t = mmsa.run_lengths(_dev(m[None]))                                        # column order, max(4096, H * W // 8) rows
    assert t.order == "column" and t.capacity == 4096 == RR.default_capacity(H, W) and t.overflow() is False
    n = RR.count_of("blocky", H, W, "column")
    count, starts, values = RR.table([m], "column", n)
    assert _host(t.count).tolist() == [n] and np.array_equal(_host(t.starts)[:, :n], starts) and np.array_equal(_host(t.values)[:, :n], values)
    t = mmsa.run_lengths(_dev(m[None]), order="row", capacity=5000)
    assert t.order == "row" and t.capacity == 5000 and all(np.array_equal(a, b) for a, b in zip(t.host(0), RR.runs(m, "row")))
    over = mmsa.run_lengths(_dev(_case("noise", H, W, None, (True, True))[None]))
    assert over.overflow() is True and _host(over.count).tolist() == [H * W]
    with pytest.raises(RuntimeError, match="order='row' with a table made with order='column'"):
        mmsa.run_lengths(_dev(m[None]), order="row", table=over)
    with pytest.raises(RuntimeError, match="capacity=7 with a table made with capacity=4096"):
        mmsa.run_lengths(_dev(m[None]), capacity=7, table=over)
    with pytest.raises(RuntimeError, match=r"a RunTable of 2 images holds contiguous int32 count \[2\]"):
        mmsa.run_lengths(_dev(np.stack([m, m])), table=over)
    with pytest.raises(RuntimeError, match="map must be a uint8 .* or int32 .* tensor, got torch.float32"):
        mmsa.run_lengths(torch.zeros(1, 4, 4, device=DEV))


# ---- 3. the segment table with runs

@pytest.mark.parametrize("kind", ["blocky", "special", "blobs"])
def test_segment_table_with_runs_carries_every_mask(kind):
    import mmsa
    H, W = 67, 131
    maps = np.stack([SR.image(kind, H, W), SR.image(kind, H, W)[::-1].copy()])
    d = _dev(maps)
    root = mmsa.components(d, num_classes=SR.C)                                # device roots
    st = mmsa.SegmentTable(num_classes=SR.C, capacity=H * W, runs="column", run_capacity=H * W)
    st.update(d, root=root)
    plain = mmsa.SegmentTable(num_classes=SR.C, capacity=H * W).update(d, root=root)
    assert plain.runs is None and all(_host(a).tobytes() == _host(b).tobytes() for a, b in ((st.count, plain.count), (st.ids, plain.ids),
                                                                                           (st.records, plain.records)))
    assert isinstance(st.runs, mmsa.RunTable) and st.runs.order == "column" and st.runs.shape == (2, H, W)
    ids, rec = _host(st.ids), _host(st.records)
    assert torch.equal(mmsa.run_decode(st.runs), st.ids)
    for b in range(2):
        runs = st.runs.host(b)
        assert all(np.array_equal(a, r) for a, r in zip(runs, RR.runs(ids[b], "column")))
        info = st.segments_info(b, masks=True)
        assert len(info) == int(st.count[b]) > 0 and [d_["id"] for d_ in info] == list(range(1, len(info) + 1))
        bare = st.segments_info(b)
        for k, (s, p) in enumerate(zip(info, bare)):
            rle = mmsa.coco_rle_of(*runs, k, H, W)
            assert s["segmentation"] == rle and {key: v for key, v in s.items() if key != "segmentation"} == p and "segmentation" not in p
            assert mmsa.rle_area_of(rle) == rec[b, k, SR.AREA] == s["area"]
            assert mmsa.rle_bbox_of(rle) == [rec[b, k, SR.X0], rec[b, k, SR.Y0], rec[b, k, SR.X1] - rec[b, k, SR.X0] + 1, rec[b, k, SR.Y1] - rec[b, k, SR.Y0] + 1]
            assert mmsa.rle_bbox_of(rle) == s["bbox"] and np.array_equal(RR.rle_mask(rle), ids[b] == k)
    rows = mmsa.SegmentTable(num_classes=SR.C, capacity=H * W, runs="row", run_capacity=H * W).update(d, root=root)
    assert rows.runs.order == "row" and rows.runs.capacity == H * W and torch.equal(mmsa.run_decode(rows.runs), st.ids)
    if kind == "blocky":                 # a few hundred runs: the default capacity holds them
        few = mmsa.SegmentTable(num_classes=SR.C, capacity=H * W, runs="column").update(d, root=root)
        assert few.runs.capacity == RR.default_capacity(H, W) == 4096 and not few.runs.overflow() and few.segments_info(1, masks=True) == st.segments_info(1, masks=True)
    with pytest.raises(ValueError, match=r"segments_info\(masks=True\) reads the column-major runs"):
        rows.segments_info(0, masks=True)


# ---- 4. the same bytes run after run, no allocation, and a captured launch

def test_determinism_no_allocation_and_graph_replay():
    import mmsa
    H, W = 130, 200
    a, b = _case("seams", H, W), _case("blocky", H, W)
    for order in RR.ORDERS:
        d = _dev(np.stack([a, b]))
        t = _table(2, H, W, order, H * W)
        mmsa.run_lengths(d, table=t)
        first = [_host(x).tobytes() for x in (t.count, t.starts, t.values)]
        out = mmsa.run_decode(t)
        torch.cuda.synchronize()
        before = torch.cuda.memory_allocated()
        for _ in range(3):
            mmsa.run_lengths(d, table=t)
            mmsa.run_decode(t, out=out)
        torch.cuda.synchronize()
        assert torch.cuda.memory_allocated() == before                        # with table= nothing is allocated
        assert [_host(x).tobytes() for x in (t.count, t.starts, t.values)] == first and np.array_equal(_host(out), np.stack([a, b]))
        g = torch.cuda.CUDAGraph()
        stream = torch.cuda.Stream()
        stream.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(stream):
            t2 = _table(2, H, W, order, H * W)
            mmsa.run_lengths(d, table=t2)                                      # the warm-up on the capture's stream
            with torch.cuda.graph(g, stream=stream):
                mmsa.run_lengths(d, table=t2)
        torch.cuda.current_stream().wait_stream(stream)
        d.copy_(_dev(np.stack([b, a])))                                        # new bytes in the captured input
        t2.count.fill_(CANARY), t2.starts.fill_(CANARY), t2.values.fill_(CANARY)
        g.replay()
        torch.cuda.synchronize()
        _same(t2, [b, a], order)
    st = mmsa.SegmentTable(num_classes=SR.C, capacity=H * W, runs="column", run_capacity=H * W)      # the second update of a shape allocates nothing, runs included
    d = _dev(np.stack([a, b]))
    st.update(d)
    torch.cuda.synchronize()
    before = torch.cuda.memory_allocated()
    st.update(d)
    torch.cuda.synchronize()
    assert torch.cuda.memory_allocated() == before and torch.equal(mmsa.run_decode(st.runs), st.ids)
