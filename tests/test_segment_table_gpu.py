"""The segment table on the GPU (csrc/segtable.hip): count, ids and records against the numpy restatement of tests/segment_table_ref.py, byte for byte.
Everything is integers: every comparison is equality.  The shapes are the smallest at which each mechanism can fail: one pixel, one row, one column, maps of
one and of several scan blocks, the edges of a scan block, more scan blocks than the scan workgroup has lanes and than one trip of the scan takes; one segment that takes every add, 64 segments
in a wave; the listing rules, the label side, the overflow; then the identities that tie the records to the passes that were there before, and the entries on
the tiny model.  Every input is listed in segment_table_ref.CASES, where tests/test_segment_table_cpu.py predicts its number of segments."""
import numpy as np
import pytest
import torch

from tests import boundary_ref as BR
from tests import components_ref as CR
from tests import eval_ref as ER
from tests import segment_table_ref as SR
from tests.test_topk_gpu import NUM_CLASSES, models  # noqa: F401  (the tiny model of the entry tests, a module-scoped fixture)

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
C = SR.C


def _dev(a):
    return torch.from_numpy(np.array(a)).to(DEV)      # a copy: the cached cases are read-only


def _host(t):
    return t.cpu().numpy()


def _case(kind, H, W, connectivity=8, min_area=1, void=False, capacity="HW", overflows=False):
    """The image of a listed case: an input that is not in the list has no prediction in the CPU file."""
    capacity = H * W if capacity == "HW" else capacity
    assert (kind, H, W, connectivity, min_area, void, capacity, overflows) in SR.CASES, (kind, H, W, connectivity, min_area, void, capacity)
    return SR.image(kind, H, W)


def _want(kinds, H, W, connectivity=8, values=None, **kw):
    codes = [np.minimum(SR.image(k, H, W), C) for k in kinds]
    return SR.table_batch(codes, [SR.image_roots(k, H, W, connectivity) for k in kinds], values=values, **kw)


def _fill(maps, values=None, connectivity=8, min_area=1, void=False, capacity=None, table=None):
    import mmsa
    st = mmsa.segment_table(_dev(np.stack(maps)), num_classes=None if table is not None else C, values=None if values is None else _dev(values),
                            connectivity=connectivity, min_area=min_area, void=void, capacity=capacity, table=table)
    B, (H, W) = len(maps), maps[0].shape
    assert st.count.dtype == torch.int32 and tuple(st.count.shape) == (B,) and st.ids.dtype == torch.int32 and tuple(st.ids.shape) == (B, H, W)
    assert st.records.dtype == torch.int64 and tuple(st.records.shape) == (B, st.capacity, 10) and st.shape == (B, H, W)
    return st


def _same(st, want, what=None):
    count, ids, records = want
    assert np.array_equal(_host(st.count), count), what
    assert np.array_equal(_host(st.ids), ids), what
    assert np.array_equal(_host(st.records), records), what      # the zero rows included


# ---- 1. the table equals the restatement

@pytest.mark.parametrize("connectivity", [4, 8])
@pytest.mark.parametrize("H,W", SR.SHAPES)
def test_noise_blocky_and_special_maps(H, W, connectivity):
    for kind in ("noise", "blocky", "special"):
        m = _case(kind, H, W, connectivity)
        values = SR.image_values("plain", H, W)[None]
        _same(_fill([m], values, connectivity, capacity=H * W), _want([kind], H, W, connectivity, values=values), kind)
        if kind == "special":      # without values: SUM_Q stays 0
            st = _fill([m], None, connectivity, capacity=H * W)
            _same(st, _want([kind], H, W, connectivity), kind)
            assert not _host(st.records)[..., SR.SUM_Q].any() and not st.scored


def test_values_that_are_no_probabilities():
    H, W = 67, 131
    values = SR.image_values("nasty", H, W)
    assert np.isnan(values).any() and np.isinf(values).any() and (values < 0).any() and (values > 1).any() and (values == 1).any()
    assert (np.signbit(values) & (values == 0)).any() and ((np.abs(values) > 0) & (np.abs(values) < 1e-38)).any()
    for kind in ("blocky", "noise"):
        _same(_fill([_case(kind, H, W)], values[None], capacity=H * W), _want([kind], H, W, values=values[None]), kind)


@pytest.mark.parametrize("kind,H,W", [("one", 67, 131), ("one", 130, 200), ("spiral", 67, 131), ("serpentine", 67, 131), ("comb", 67, 131)])
def test_one_row_takes_every_add(kind, H, W):
    values = SR.image_values("plain", H, W)[None]
    st = _fill([_case(kind, H, W)], values, capacity=H * W)
    want = _want([kind], H, W, values=values)
    _same(st, want)
    if kind == "one":              # the closed forms
        assert _host(st.count).tolist() == [1] and not _host(st.ids).any()
        row = _host(st.records)[0, 0]
        assert row[:9].tolist() == [0, 7, H * W, 0, 0, W - 1, H - 1, H * W * (W - 1) // 2, H * W * (H - 1) // 2] and row[SR.SUM_Q] == SR.q24(values).sum()
    else:                          # two segments; the path takes about half of the adds
        assert _host(st.count)[0] >= 2 and _host(st.records)[0, 0, SR.AREA] == (SR.image(kind, H, W) == 1).sum() > H * W // 3


@pytest.mark.parametrize("d", [-1, 0, 1])
def test_the_edges_of_a_scan_block(d):
    from mmsa.evaluate import SEGTAB_BLOCK
    assert SEGTAB_BLOCK == SR.BLOCK
    W = SEGTAB_BLOCK + d
    values = SR.image_values("plain", 1, W)[None]
    _same(_fill([_case("noise", 1, W)], values, capacity=W), _want(["noise"], 1, W, values=values))


def _large_map_equals_the_restatement_on_the_gpu_roots(H, W, n_want):
    """The roots come from mmsa.components and the restatement is applied to THOSE roots: the test judges the table, not the labelling a second time."""
    import mmsa
    m = SR.image("noise", H, W)
    values = SR.image_values("plain", H, W)[None]
    d = _dev(m[None])
    root = mmsa.components(d, num_classes=C)
    st = mmsa.segment_table(d, num_classes=C, values=_dev(values), root=root, capacity=H * W)
    assert st.root is root
    n, ids, rec = SR.table(m, _host(root)[0], values=values[0])
    assert n == n_want and _host(st.count).tolist() == [n] and np.array_equal(_host(st.ids)[0], ids) and np.array_equal(_host(st.records)[0], rec)
    return ids


def test_more_scan_blocks_than_the_scan_workgroup_has_lanes():
    from mmsa.evaluate import SEGTAB_BLOCK, SCAN_LANES
    H, W = SR.LARGE
    assert -(-H * W // SEGTAB_BLOCK) > SCAN_LANES
    _large_map_equals_the_restatement_on_the_gpu_roots(H, W, 457508)


def test_more_scan_blocks_than_one_trip_of_the_scan_takes():
    """1027 blocks: the scan's second trip starts from the carry of the first, and the last block, behind it, writes the count."""
    import mmsa
    H, W = SR.LARGER
    block = mmsa.lib.raw.mmsa_run_lengths_block                                # the scan of both tables: lanes and counts per trip from the library
    blocks = -(-H * W // mmsa.lib.raw.mmsa_segment_table_block())
    assert blocks > block(3) > block(2)
    ids = _large_map_equals_the_restatement_on_the_gpu_roots(H, W, 1780301)
    assert ids.ravel()[(blocks - 1) * SR.BLOCK:].max() > ids.ravel()[:block(3) * SR.BLOCK].max()      # listed roots in the last block, numbered past the first trip's


def test_three_images_in_a_batch_then_a_batch_of_two():
    import mmsa
    H, W = 96, 160
    kinds = ("blocky", "one", "noise")
    st = mmsa.SegmentTable(num_classes=C, capacity=H * W)
    values = np.stack([SR.image_values("plain", H, W)] * 3)
    st.update(_dev(np.stack([_case(k, H, W, capacity=H * W) for k in kinds])), values=_dev(values))
    _same(st, _want(kinds, H, W, values=values))
    first = st.records
    st.update(_dev(np.stack([_case(k, 50, 70, capacity=H * W) for k in ("special", "blocky")])))      # buffers of a second shape
    _same(st, _want(("special", "blocky"), 50, 70, capacity=H * W))
    assert st.records is not first and st.shape == (2, 50, 70) and tuple(st.records.shape) == (2, H * W, 10) and not st.scored


# ---- 2. what is listed

@pytest.mark.parametrize("connectivity", [4, 8])
@pytest.mark.parametrize("void", [False, True])
def test_min_area(void, connectivity):
    import mmsa
    H, W = 67, 131
    counts = []
    for min_area in (1, 2, 5, 64):
        m = _case("blobs", H, W, connectivity, min_area, void)
        st = _fill([m], None, connectivity, min_area, void, H * W)
        _same(st, _want(["blobs"], H, W, connectivity, min_area=min_area, void=void), min_area)
        counts.append(int(st.count[0]))
        area = _host(mmsa.component_areas(st.root))[0].ravel()
        assert ((_host(st.ids)[0] >= 0) == (area[_host(st.root)[0]] >= min_area)).all()
    assert counts[0] > counts[1] > counts[2] > counts[3] and counts[2] > 0 and (counts[3] > 0) == (connectivity == 8)      # three-class noise at 4: no blob of 64


def test_void_lists_the_other_codes():
    H, W = 67, 131
    for min_area in (1, 64):
        m = _case("special", H, W, 8, min_area, True)
        st = _fill([m], None, min_area=min_area, void=True, capacity=H * W)
        _same(st, _want(["special"], H, W, min_area=min_area, void=True))
        assert (min_area > 1 or (_host(st.ids) >= 0).all()) and (_host(st.records)[0, :int(st.count[0]), SR.CLASS] == C).any()
    plain = _fill([_case("special", H, W)], None, capacity=H * W)
    assert ((_host(plain.ids)[0] >= 0) == (m < C)).all() and int(plain.count[0]) > 0


@pytest.mark.parametrize("connectivity", [4, 8])
def test_the_label_side(connectivity):
    import mmsa
    from mmsa.evaluate import LabelPrep
    rng = np.random.default_rng(77)
    label = np.stack([CR.blocky(rng, 50, 90, 8, 3, 9), rng.integers(0, 8, size=(50, 90)).astype(np.uint8)])
    label[0, 10:20, 30:60] = 255
    label[1, 30:35, :] = 255
    label[0, 40:, :20] = 40                                                # beyond the classes: the code C
    H, W = 67, 131
    ymap, xmap = ER.nearest_index(50, H), ER.nearest_index(90, W)
    values = np.stack([SR.image_values("plain", H, W), SR.image_values("nasty", H, W)])
    for kw in (dict(reduce_zero_label=True, label_map={3: 1, 5: 255}), dict()):
        lp = LabelPrep(6, resize=dict(seg_scale=(W, H), keep_ratio=False), **kw)
        codes = [BR.codes(np.zeros((H, W), dtype=np.uint8), label[b], ER.lut(6, **kw), 6, ymap, xmap)[0] for b in range(2)]
        roots = [CR.roots(L, connectivity) for L in codes]
        assert all((L == 255).any() and (L == 6).any() for L in codes)
        for void in (False, True):      # capacity H * W: no overflow
            st = mmsa.segment_table(_dev(label), labels_prep=lp, values=_dev(values), connectivity=connectivity, void=void, capacity=H * W)
            want = SR.table_batch(codes, roots, num_classes=6, void=void, values=values)
            _same(st, want, (kw, void))
            listed = _host(st.records)[0, :int(st.count[0]), SR.CLASS]
            assert ({6, 255} <= set(listed.tolist())) == void and (void or (listed < 6).all())      # 255 and C are codes of their own


def test_overflow_is_visible_and_keeps_the_first_rows():
    import mmsa
    H, W = 31, 63
    m = _case("noise", H, W, capacity=None, overflows=True)
    st = _fill([m])                                                        # the default capacity
    count, ids, full = _want(["noise"], H, W)
    assert st.capacity == 1024 and count.tolist() == [1618]
    assert _host(st.count).tolist() == [1618] and np.array_equal(_host(st.ids), ids)                      # the true number; ids complete
    assert np.array_equal(_host(st.records), full[:, :1024]) and _host(st.records)[0, 1023, SR.AREA] > 0  # exactly the first 1024 rows
    assert st.overflow() is True
    for call in (st.host, lambda: st.host(0), lambda: st.segments_info(0)):
        with pytest.raises(RuntimeError, match=r"image 0 has 1618 listed segments and the table 1024 rows.*capacity="):
            call()
    keep = torch.zeros(1, 1024, dtype=torch.uint8, device=DEV)
    got = _host(mmsa.select_segments(_dev(m[None]), st, keep, fill=200))
    assert np.array_equal(got, np.where((ids >= 0) & (ids < 1024), 200, m[None])) and (got[ids >= 1024] == m[None][ids >= 1024]).all() and (ids >= 1024).any()
    roomy = _fill([m], capacity=H * W)
    assert roomy.overflow() is False and len(roomy.host()) == 1618 and len(roomy.segments_info(0)) == 1618


# ---- 3. identities on device results

def test_records_agree_with_the_passes_that_were_there_before():
    import mmsa
    from mmsa.evaluate import LabelPrep, SegmentEvaluator
    H, W = 67, 131
    for kind in ("blocky", "noise"):
        m = _case(kind, H, W)
        d = _dev(np.stack([m, m[::-1].copy()]))
        conf = _dev(np.stack([SR.image_values("plain", H, W), SR.image_values("nasty", H, W)]))
        st = mmsa.segment_table(d, num_classes=C, values=conf, capacity=H * W)
        n = _host(st.count)
        area = _host(mmsa.component_areas(st.root))
        lp = LabelPrep(C)
        labels = _dev(np.stack([SR.image("blocky", H, W)] * 2))                # all classes: nothing ignored, nothing out of range
        se = SegmentEvaluator(lp, bins=1, images=2, device=DEV).add(d, labels)
        cal = _host(mmsa.calibration(d, conf, labels, lp, bins=15))
        for b in range(2):
            rec = _host(st.records)[b, :n[b]]
            assert np.array_equal(rec[:, SR.AREA], area[b].ravel()[rec[:, SR.ROOT]]) and n[b] == (area[b] > 0).sum()      # AREA is component_areas at ROOT
            assert np.array_equal(rec[:, SR.Y0], rec[:, SR.ROOT] // W) and (rec[:, SR.X0] <= rec[:, SR.ROOT] % W).all()
            assert np.array_equal(np.bincount(rec[:, SR.CLASS], weights=rec[:, SR.AREA], minlength=C).astype(np.int64), np.bincount(_host(d)[b].ravel(), minlength=C))
            by = np.zeros((C, 24), dtype=np.int64)
            np.add.at(by, (rec[:, SR.CLASS], np.minimum(23, np.floor(np.log2(rec[:, SR.AREA])).astype(int))), 1)
            assert np.array_equal(by, se.host_counts()[b, 1].sum(-1))        # the rows per (class, size bucket): SegmentEvaluator's prediction side
            assert rec[:, SR.SUM_Q].sum() == cal[b, 2].sum()                   # the confidence-sum row of mmsa.calibration over the bins


# ---- 4. select_segments

def test_select_segments_equals_the_restatement_in_and_out_of_place():
    import mmsa
    from mmsa.evaluate import score_threshold_q
    H, W = 67, 131
    maps = np.stack([_case("blocky", H, W, void=True), _case("special", H, W, void=True)[::-1].copy()])
    values = np.stack([SR.image_values("plain", H, W), SR.image_values("nasty", H, W)])
    d = _dev(maps)
    st = mmsa.segment_table(d, num_classes=C, values=_dev(values), void=True, capacity=H * W)
    rec = _host(st.records)
    for kw in (dict(min_area=40), dict(max_area=64), dict(min_score=0.5), dict(classes=[0, 2, C]), dict(min_area=8, max_area=4096, min_score=0.45, classes=range(4))):
        keep = st.keep(**kw)
        ref = dict(kw, min_score_q=score_threshold_q(kw["min_score"])) if "min_score" in kw else dict(kw)
        ref.pop("min_score", None)
        want_keep = SR.keep(rec, **ref)
        assert keep.dtype == torch.uint8 and np.array_equal(_host(keep), want_keep) and 0 < want_keep.sum() < (rec[..., SR.AREA] > 0).sum(), kw
        want = SR.select(maps, _host(st.ids), want_keep, 200)
        got = mmsa.select_segments(d, st, keep, fill=200)
        assert got.data_ptr() != d.data_ptr() and np.array_equal(_host(got), want) and (want != maps).any() and (want == maps).any(), kw
        inplace = d.clone()
        assert mmsa.select_segments(inplace, st, keep, fill=200, out=inplace) is inplace and _host(inplace).tobytes() == _host(got).tobytes()
    with pytest.raises(RuntimeError, match=r"keep must be a contiguous uint8 \(2, 8777\) tensor"):
        mmsa.select_segments(d, st, keep[:, :100])
    with pytest.raises(RuntimeError, match="min_score= on a table filled without values="):
        mmsa.segment_table(d, num_classes=C, capacity=H * W).keep(min_score=0.5)


@pytest.mark.parametrize("connectivity", [4, 8])
def test_select_segments_is_suppress_small(connectivity):
    import mmsa
    H, W = 67, 131
    pred = np.stack([_case("blobs", H, W, connectivity, 1, True), _case("special", H, W, connectivity if connectivity == 4 else 8, 1, True)])
    d = _dev(pred)
    st = mmsa.segment_table(d, num_classes=C, connectivity=connectivity, void=True, capacity=H * W)
    for k in (2, 5, 64):
        got = mmsa.select_segments(d, st, st.keep(min_area=k), fill=200)
        want = mmsa.suppress_small(d, k, num_classes=C, connectivity=connectivity, fill=200)
        assert _host(got).tobytes() == _host(want).tobytes() == CR.suppress(pred, C, k, connectivity, fill=200).tobytes() and (_host(got) != pred).any()


# ---- 5. the entries on the tiny model

def test_entries_fill_the_table_from_the_returned_map(models):  # noqa: F811
    import mmsa
    import mmsa.inference as inf
    cfg, m, h, frame, x = models

    def fresh(shape):
        return mmsa.SegmentTable(num_classes=NUM_CLASSES, capacity=shape[1] * shape[2])      # H * W rows: no overflow

    def same(st, cm, conf):
        want = mmsa.segment_table(cm, num_classes=NUM_CLASSES, values=conf, capacity=cm.shape[1] * cm.shape[2])
        assert st.shape == tuple(cm.shape) and st.scored == (conf is not None) and int(want.count.sum()) > 0
        assert torch.equal(st.count, want.count) and torch.equal(st.ids, want.ids) and torch.equal(st.records, want.records)

    plain = inf.whole_class_map(m, h, x, ori_shape=(200, 310), confidence=True)                # a rescaled size
    st = fresh(plain[0].shape)
    got = inf.whole_class_map(m, h, x, ori_shape=(200, 310), confidence=True, segment_table=st)
    assert len(got) == len(plain) and all(torch.equal(a, b) for a, b in zip(got, plain))
    same(st, got[0], got[-1])
    none = inf.whole_class_map(m, h, x, ori_shape=(200, 310), confidence=True, segment_table=None)
    assert all(torch.equal(a, b) for a, b in zip(none, plain))
    bare = inf.whole_class_map(m, h, x)
    st = fresh(bare.shape)
    cm = inf.whole_class_map(m, h, x, segment_table=st)                                        # no confidence: no values
    assert torch.equal(cm, bare)
    same(st, cm, None)
    plain = inf.slide_class_map(m, h, frame, (256, 256), (170, 170), max_batch=2, confidence=True)
    st = fresh(plain[0].shape)
    got = inf.slide_class_map(m, h, frame, (256, 256), (170, 170), max_batch=2, confidence=True, segment_table=st)
    assert all(torch.equal(a, b) for a, b in zip(got, plain))
    same(st, got[0], got[2])
    cm, unc, tk = inf.slide_class_map(m, h, frame, (256, 256), (170, 170), max_batch=2, topk=2, segment_table=st)
    assert torch.equal(cm, plain[0]) and cm.data_ptr() == tk.classes[0].data_ptr()
    same(st, tk.classes[0], tk.probs[0])                                                       # plane 0, and probs[0] as the values
    sr = inf.SlideRunner(m, h, frame, (256, 256), (170, 170), chains=2, confidence=True)
    res = sr.run(segment_table=st)
    out = res.outputs()
    assert torch.equal(out[0], plain[0])
    same(st, out[0], res.confidence())
    with pytest.raises(RuntimeError, match="mmsa.whole_class_map: segment_table= takes an mmsa.evaluate.SegmentTable, got int"):
        inf.whole_class_map(m, h, x, segment_table=3)


# ---- 6. the same bytes run after run, and no allocation

def test_determinism_and_no_allocation_on_the_second_update():
    import mmsa
    H, W = 130, 200
    for kind in ("noise", "one"):
        d = _dev(np.stack([_case(kind, H, W)] * 2))
        values = _dev(np.stack([SR.image_values("plain", H, W)] * 2))
        st = mmsa.SegmentTable(num_classes=C, capacity=H * W, min_area=1)
        st.update(d, values=values)
        first = [_host(t).tobytes() for t in (st.count, st.ids, st.records)]
        keep = st.keep(min_area=2)
        out = mmsa.select_segments(d, st, keep)
        torch.cuda.synchronize()
        before = torch.cuda.memory_allocated()
        for _ in range(3):
            st.update(d, values=values)
            mmsa.select_segments(d, st, keep, out=out)
        torch.cuda.synchronize()
        assert torch.cuda.memory_allocated() == before                        # the second update of a shape allocates nothing
        assert [_host(t).tobytes() for t in (st.count, st.ids, st.records)] == first
    area = mmsa.SegmentTable(num_classes=C, capacity=H * W, min_area=5)           # with the area plane
    area.update(d)
    torch.cuda.synchronize()
    before = torch.cuda.memory_allocated()
    area.update(d)
    torch.cuda.synchronize()
    assert torch.cuda.memory_allocated() == before
