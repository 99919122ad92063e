"""The segment table without a GPU: the numpy restatement of tests/segment_table_ref.py against scipy.ndimage, the host readings on hand-made records, the
refusals, the exports, and -- for every input of tests/test_segment_table_gpu.py -- the predicted number of segments against the capacity its test uses."""
import inspect

import numpy as np
import pytest
from scipy import ndimage

from tests import segment_table_ref as SR

STRUCT = {4: ndimage.generate_binary_structure(2, 1), 8: np.ones((3, 3), dtype=int)}


# ---- 1. the restatement against scipy

@pytest.mark.parametrize("connectivity", [4, 8])
@pytest.mark.parametrize("kind,H,W", [("noise", 31, 63), ("blocky", 67, 131), ("special", 67, 131), ("blocky", 130, 200), ("spiral", 31, 63), ("one", 1, 1)])
def test_restatement_equals_scipy(kind, H, W, connectivity):
    import mmsa
    code = np.minimum(SR.image(kind, H, W), SR.C)
    values = SR.image_values("nasty", H, W)
    n, ids, rec = SR.table(code, SR.image_roots(kind, H, W, connectivity), void=True, values=values)
    assert n == int(ids.max()) + 1 and (ids >= 0).all() and not rec[n:].any()
    seg = mmsa.segment_records_of(rec, n)
    q = SR.q24(values).astype(np.float64)
    seen = 0
    for c in np.unique(code):
        lab, m = ndimage.label(code == c, STRUCT[connectivity])      # numbered in raster order of the first pixel, as the table is within a class
        rows = rec[:n][rec[:n, SR.CLASS] == c]
        assert len(rows) == m
        index = np.arange(1, m + 1)
        assert np.array_equal(rows[:, SR.AREA], ndimage.sum_labels(np.ones_like(lab), lab, index).astype(np.int64))
        assert np.array_equal(rows[:, SR.SUM_Q], ndimage.sum_labels(q, lab, index).astype(np.int64))      # below 2^53: exact in float64
        for row, sl, com, k in zip(rows, ndimage.find_objects(lab), ndimage.center_of_mass(np.ones_like(lab), lab, index), index):
            assert (row[SR.Y0], row[SR.Y1] + 1, row[SR.X0], row[SR.X1] + 1) == (sl[0].start, sl[0].stop, sl[1].start, sl[1].stop)
            assert row[SR.ROOT] == np.flatnonzero(lab == k)[0] and (ids[lab == k] == ids.ravel()[row[SR.ROOT]]).all()
            s = seg[ids.ravel()[row[SR.ROOT]]]
            assert s["root"] == row[SR.ROOT] and s["category"] == c and np.allclose(s["centroid"], (com[1], com[0]), rtol=1e-12, atol=1e-12)
            assert list(s["bbox"]) == [sl[1].start, sl[0].start, sl[1].stop - sl[1].start, sl[0].stop - sl[0].start]
        seen += m
    assert seen == n and np.array_equal(rec[:n, SR.ROOT], np.sort(rec[:n, SR.ROOT]))      # ascending root index: raster order of the first pixel


def test_listing_rules_and_capacity_of_the_restatement():
    from mmsa.evaluate import SEGMENT_FIELDS
    assert len(SEGMENT_FIELDS) == SR.FIELDS
    H, W = 67, 131
    code, root = np.minimum(SR.image("special", H, W), SR.C), SR.image_roots("special", H, W)
    n_all, ids_all, rec_all = SR.table(code, root, void=True)
    n, ids, rec = SR.table(code, root)
    classes = rec_all[:n_all, SR.CLASS] < SR.C
    assert n == classes.sum() < n_all and np.array_equal(rec[:n], rec_all[:n_all][classes]) and ((ids >= 0) == (code < SR.C)).all()
    code, root = SR.image("blobs", H, W), SR.image_roots("blobs", H, W)
    n_all, ids_all, rec_all = SR.table(code, root, void=True)
    for a in (2, 5, 64):
        big = rec_all[:n_all, SR.AREA] >= a
        na, ida, ra = SR.table(code, root, min_area=a, void=True)
        assert 0 < na == big.sum() < n_all and np.array_equal(ra[:na], rec_all[:n_all][big]) and ((ida >= 0) == big[ids_all]).all()
    cut = SR.table(code, root, void=True, capacity=5)
    assert cut[0] == n_all and np.array_equal(cut[1], ids_all) and np.array_equal(cut[2], rec_all[:5])      # the first rows in raster order; ids complete
    wide = SR.table(code, root, void=True, capacity=n_all + 3)
    assert np.array_equal(wide[2][:n_all], rec_all[:n_all]) and not wide[2][n_all:].any()


# ---- 2. the host readings

def test_host_readings_on_hand_made_records():
    import mmsa
    from mmsa import evaluate as E
    assert E.SEGMENT_FIELDS == ("ROOT", "CLASS", "AREA", "X0", "Y0", "X1", "Y1", "SUM_X", "SUM_Y", "SUM_Q") and E.SCORE_ONE == SR.ONE == E.CONF_ONE
    assert (E.ROOT, E.CLASS, E.AREA, E.X0, E.Y0, E.X1, E.Y1, E.SUM_X, E.SUM_Y, E.SUM_Q) == tuple(range(10))
    rec = np.array([[5, 3, 4, 5, 0, 6, 1, 22, 2, 3 * SR.ONE], [40, 25, 1, 7, 2, 7, 2, 7, 2, 0], [0, 0, 0, 0, 0, 0, 0, 0, 0, 0]], dtype=np.int64)
    s = mmsa.segment_records_of(rec, 3, image=4)
    assert s.dtype == E.SEGMENT_DTYPE and s["image"].tolist() == [4, 4, 4] and s["id"].tolist() == [0, 1, 2] and s["root"].tolist() == [5, 40, 0]
    assert s["category"].tolist() == [3, 25, 0] and s["area"].tolist() == [4, 1, 0] and s["bbox"].tolist() == [[5, 0, 2, 2], [7, 2, 1, 1], [0, 0, 1, 1]]
    assert s["centroid"][:2].tolist() == [[5.5, 0.5], [7.0, 2.0]] and s["score"][:2].tolist() == [0.75, 0.0]
    assert np.isnan(s["centroid"][2]).all() and np.isnan(s["score"][2])                                  # 0 / 0
    assert np.isnan(mmsa.segment_records_of(rec, 2, scored=False)["score"]).all() and len(mmsa.segment_records_of(rec, 0)) == 0
    with pytest.raises(RuntimeError, match=r"image 0 has 4 listed segments and the table 3 rows.*capacity="):
        mmsa.segment_records_of(rec, 4)
    with pytest.raises(ValueError, match=r"segment records are an integer \[rows, 10\] array"):
        mmsa.segment_records_of(rec[:, :9], 1)
    with pytest.raises(ValueError, match="segment records are an integer"):
        mmsa.segment_records_of(rec.astype(np.float64), 1)


def test_the_integer_score_threshold_at_an_exact_edge():
    from mmsa.evaluate import score_threshold_q
    assert score_threshold_q(0) == 0 and score_threshold_q(1) == SR.ONE and score_threshold_q(0.5) == SR.ONE // 2 and score_threshold_q(0.75) == 3 * SR.ONE // 4
    assert score_threshold_q(0.1) == 1677721 and score_threshold_q(2.0 ** -24) == 1 and score_threshold_q(np.nextafter(2.0 ** -24, 0)) == 0      # floor
    for bad in (-0.1, 1.5, "0.5", True, None, float("nan")):
        with pytest.raises(ValueError, match="min_score = .*a score in \\[0, 1\\]"):
            score_threshold_q(bad)
    # SUM_Q >= q * AREA: a mean of exactly 3/4 passes 0.75 and one unit less fails; in float64 the two means differ by 2^-26
    q = score_threshold_q(0.75)
    rec = np.zeros((2, 3, 10), dtype=np.int64)
    rec[0, :, SR.AREA], rec[0, :, SR.SUM_Q] = 4, (4 * q, 4 * q - 1, 4 * q + 1)
    assert SR.keep(rec, min_score_q=q).tolist() == [[1, 0, 1], [0, 0, 0]]


# ---- 3. refusals and exports

def test_constructor_refusals():
    import mmsa
    from mmsa.evaluate import LabelPrep, SegmentTable, default_segment_capacity
    assert default_segment_capacity(31, 63) == 1024 == SR.default_capacity(31, 63) and default_segment_capacity(1024, 1024) == 16384 == SR.default_capacity(1024, 1024)
    for bad in (0, -4, 2.5, "9", True, 1 << 31):
        with pytest.raises(ValueError, match="mmsa.SegmentTable: capacity = .*a positive number of rows per image"):
            SegmentTable(num_classes=5, capacity=bad)
    with pytest.raises(ValueError, match="takes num_classes= .* or labels_prep= .*one of them"):
        SegmentTable()
    with pytest.raises(ValueError, match="one of them"):
        SegmentTable(num_classes=5, labels_prep=LabelPrep(5))
    with pytest.raises(ValueError, match="mmsa.SegmentTable: connectivity = 6"):
        SegmentTable(num_classes=5, connectivity=6)
    with pytest.raises(ValueError, match="mmsa.SegmentTable: min_area = 0"):
        SegmentTable(num_classes=5, min_area=0)
    with pytest.raises(ValueError, match="mmsa.SegmentTable: void = 1"):
        SegmentTable(num_classes=5, void=1)
    with pytest.raises(ValueError, match="num_classes 255"):
        SegmentTable(num_classes=255)
    st = SegmentTable(num_classes=5, capacity=77)
    assert st.capacity == 77 and st.count is None and (st.num_classes, st.connectivity, st.min_area, st.void) == (5, 8, 1, False)
    assert SegmentTable(labels_prep=LabelPrep(7)).num_classes == 7 and SegmentTable(num_classes=5).capacity is None
    for call in (st.overflow, st.host, lambda: st.segments_info(0), st.keep):
        with pytest.raises(RuntimeError, match="nothing was filled yet"):
            call()
    with pytest.raises(RuntimeError, match="table= takes an mmsa.evaluate.SegmentTable, got int"):
        mmsa.segment_table(None, table=3)
    with pytest.raises(RuntimeError, match="min_area=4 with a table made with min_area=1"):
        mmsa.segment_table(None, min_area=4, table=st)
    with pytest.raises(RuntimeError, match="table takes an mmsa.evaluate.SegmentTable, got NoneType"):
        mmsa.select_segments(None, None, None)
    with pytest.raises(RuntimeError, match="map must be a tensor"):
        st.update(np.zeros((1, 4, 4), dtype=np.uint8))


def test_exports_and_entries():
    import mmsa
    import mmsa.inference as inf
    for name in ("SegmentTable", "segment_table", "select_segments", "segment_records_of"):
        assert getattr(mmsa, name) is getattr(mmsa.evaluate, name) and name in mmsa.__all__
    assert mmsa.evaluate.SEGTAB_BLOCK == SR.BLOCK and SR.LARGE[0] * SR.LARGE[1] > SR.BLOCK * mmsa.evaluate.SCAN_LANES
    assert SR.LARGER[0] * SR.LARGER[1] > SR.BLOCK * mmsa.evaluate.SCAN_TRIP and mmsa.evaluate.SCAN_TRIP > mmsa.evaluate.SCAN_LANES
    assert [mmsa.lib.raw.mmsa_run_lengths_block(k) for k in (2, 3)] == [mmsa.evaluate.SCAN_LANES, mmsa.evaluate.SCAN_TRIP]      # the scan is the one of both tables
    for name in ("mmsa_segment_table", "mmsa_segment_table_block", "mmsa_select_segments_u8"):
        assert name in mmsa.lib.SIGNATURES and hasattr(mmsa.lib.raw, name)
    assert len(mmsa.lib.SIGNATURES["mmsa_segment_table"]) == 20 and len(mmsa.lib.SIGNATURES["mmsa_select_segments_u8"]) == 10 and mmsa.lib.raw.mmsa_segment_table_block() == SR.BLOCK and mmsa.lib.version() == 114
    for fn in (inf.slide_class_map, inf.whole_class_map, inf.class_map, inf.aug_class_map, inf.MapPlan.class_map, inf.SlideRunner.run):
        assert inspect.signature(fn).parameters["segment_table"].default is None, fn.__qualname__


def test_map_options_refusals():
    import mmsa
    import mmsa.inference as inf
    from mmsa.evaluate import LabelPrep
    assert inf.MapOptions.of("slide_class_map").segment_table is None
    st = mmsa.SegmentTable(num_classes=5)
    assert inf.MapOptions.of("aug_class_map", segment_table=st).segment_table is st          # it needs no labels=
    with pytest.raises(RuntimeError, match="mmsa.slide_class_map: segment_table= takes an mmsa.evaluate.SegmentTable, got int"):
        inf.MapOptions.of("slide_class_map", segment_table=3)
    with pytest.raises(RuntimeError, match="mmsa.whole_class_map: segment_table= with return_map=False"):
        inf.MapOptions.of("whole_class_map", segment_table=st, labels=object(), evaluator=object(), return_map=False)
    with pytest.raises(RuntimeError, match="mmsa.class_map: segment_table= takes a SegmentTable made with num_classes="):
        inf.MapOptions.of("class_map", segment_table=mmsa.SegmentTable(labels_prep=LabelPrep(5)))
    with pytest.raises(RuntimeError, match="mmsa.SlideRunner.run: segment_table= takes an mmsa.evaluate.SegmentTable, got str"):
        inf.MapOptions.of("SlideRunner").with_call("SlideRunner.run", segment_table="st")


# ---- 4. the inputs of the GPU tests, predicted

def test_every_gpu_input_has_the_overflow_its_test_expects():
    from mmsa.evaluate import default_segment_capacity
    over = []
    for kind, H, W, connectivity, min_area, void, capacity, overflows in SR.CASES:
        n = SR.table(np.minimum(SR.image(kind, H, W), SR.C), SR.image_roots(kind, H, W, connectivity), min_area=min_area, void=void)[0]
        cap = default_segment_capacity(H, W) if capacity is None else capacity
        assert (n > cap) == overflows, (kind, H, W, connectivity, min_area, void, n, cap)
        assert capacity is None or capacity >= H * W or n <= capacity
        over += [(kind, H, W)] * overflows
    assert over == [("noise", 31, 63)]                       # exactly the intended one; the large map runs at capacity = H * W, which can never overflow


def test_reference_counts_of_the_shared_maps():
    """The segments of the noise and blocky maps at 25 classes, connectivity 8, pinned from these seeds (scipy's count, which the restatement equals above)."""
    want = {("noise", 31, 63): 1618, ("noise", 67, 131): 7415, ("noise", 130, 200): 22002, ("noise", 600, 900): 457508,
            ("blocky", 31, 63): 7, ("blocky", 67, 131): 14, ("blocky", 130, 200): 92, ("blocky", 600, 900): 1188}
    from mmsa.evaluate import default_segment_capacity
    for (kind, H, W), n in want.items():
        m = SR.image(kind, H, W)
        assert sum(ndimage.label(m == c, STRUCT[8])[1] for c in np.unique(m)) == n, (kind, H, W)
        if H * W <= 130 * 200:
            assert SR.table(m, SR.image_roots(kind, H, W))[0] == n
        assert (n > default_segment_capacity(H, W)) == (kind == "noise")      # noise overflows the default capacity at every size, blocky never does
        assert n <= H * W
