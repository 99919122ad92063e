"""The segment tracker on the GPU (csrc/track.hip): state, stats, totals, next_track, tracks, the successor and previous-area columns and the occupied pair
slots (as a sorted multiset) against the numpy restatement of tests/segment_tracker_ref.py, byte for byte, after EVERY frame of a sequence.  Everything is
integers: every comparison is equality.  The shapes are the smallest at which each mechanism can fail: one pixel, one row, one column, a wave's edge, ragged
blocks with three images, more rows than one trip of the assign scan, an empty frame, a first frame and a reset, the hand-made IoU cases, a table smaller than
its segments, a pair table that overflows.  Every tracker is listed in segment_tracker_ref.CASES, where tests/test_segment_tracker_cpu.py predicts its pair
tables."""
import numpy as np
import pytest
import torch

from tests import segment_table_ref as SR
from tests import segment_tracker_ref as TR
from tests.test_topk_gpu import NUM_CLASSES, models  # noqa: F401  (the tiny model of the entry tests, a module-scoped fixture)

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
C = TR.C


def _dev(a):
    return torch.from_numpy(np.array(a)).to(DEV)      # a copy: the cached sequences are read-only


def _host(t):
    return t.cpu().numpy()


def _pairs(tr):
    keys, counts = _host(tr.pairs.keys), _host(tr.pairs.counts)
    used = keys != -1
    order = np.argsort(keys[used], kind="stable")
    assert not counts[~used].any()
    return keys[used][order], counts[used][order].astype(np.int64)


def _same(st, tr, want, table, what=None):
    count, ids, records = table
    assert np.array_equal(_host(st.count), count) and np.array_equal(_host(st.ids), ids) and np.array_equal(_host(st.records), records), what
    keys, inters = _pairs(tr)                                                   # the pair list first: what the other arrays are made from
    assert np.array_equal(keys, want["keys"]) and np.array_equal(inters, want["inters"]) and tr.overflow() == 0, (what, len(keys), len(want["keys"]))
    for name in ("state", "stats", "totals", "next_track", "succ", "prev_area"):
        got = _host(getattr(tr, name))
        assert got.dtype == want[name].dtype and got.shape == want[name].shape, (what, name)
        at = np.argwhere(got != want[name])
        assert len(at) == 0, (what, name, len(at), at[0].tolist(), got[tuple(at[0])].tolist(), want[name][tuple(at[0])].tolist())
    if tr.tracks is not None:
        assert tr.tracks.dtype == torch.int32 and np.array_equal(_host(tr.tracks), want["tracks"]), what
    assert np.array_equal(_host(tr.prev_ids), ids) and np.array_equal(_host(tr.prev_count), count), what      # carried over for the next frame


def _drive(name, capacity=None, same_class=True, pair_capacity=None, resets=(), tracks=True, frames=None):
    """A new table and tracker over the named sequence, held to the restatement after every frame -> (table, tracker, the restatement's results)."""
    import mmsa
    assert (name, capacity, same_class, pair_capacity, tuple(resets), False) in TR.CASES, name      # an input that is not listed has no predicted pair table
    seq = TR.sequence(name)
    B, H, W = seq[0].shape
    st = mmsa.SegmentTable(num_classes=C, capacity=H * W if capacity is None else capacity)
    tr = mmsa.SegmentTracker(st, same_class=same_class, pair_capacity=pair_capacity, tracks=tracks)
    want, tabs = TR.run(name, capacity, same_class, resets), TR.tables(name, capacity)
    for t, f in enumerate(seq[:frames]):
        for at, b in resets:
            if at == t:
                assert tr.reset(b) is tr
        st.update(_dev(f))
        assert tr.update() is tr
        _same(st, tr, want[t], tabs[t], (name, t))
    assert tuple(tr.state.shape) == (B, st.capacity, 4) and tr.state.dtype == torch.int32 and tr.totals.dtype == torch.int64
    return st, tr, want


# ---- 1. the tracker equals the restatement, frame by frame

@pytest.mark.parametrize("name", ["1x1", "row", "column", "w63", "w64", "w65", "gap"])
def test_small_shapes_and_an_empty_frame(name):
    st, tr, want = _drive(name)
    assert (want[-1]["totals"][0] > 0).all() and np.array_equal(_host(tr.totals), want[-1]["totals"])      # something continued, was born and ended
    if name == "gap":      # the frame without a listed segment: nothing alive, everything ended; the frame behind it is all new
        assert int(want[1]["stats"][0, 2]) == int(want[0]["stats"][0, 1]) > 0 and not (want[1]["state"][..., TR.TRACK] >= 0).any()


def test_three_images_do_not_see_each_other():
    _, tr, want = _drive("ragged")
    assert all(int(w["stats"][b, 0]) > 0 for w in want[1:] for b in range(3))
    _, twins, _ = _drive("twins")
    s = _host(twins.state)
    assert np.array_equal(s[0], s[1]) and np.array_equal(s[0], s[2]) and (s[0, :, TR.AGE] > 1).any()
    _drive("ragged", same_class=False)


def test_first_frame_and_reset_of_one_image_of_three():
    st, tr, want = _drive("ragged", frames=1)
    n = _host(st.count)
    assert want[0]["stats"].tolist() == [[0, int(v), 0] for v in n] and _host(tr.next_track).tolist() == n.tolist()      # everything is born, nothing ends
    _, tr, want = _drive("ragged", resets=((2, 1),))
    plain = TR.run("ragged")
    assert int(want[2]["stats"][1, 0]) == 0 < int(plain[2]["stats"][1, 0]) and np.array_equal(want[2]["state"][0], plain[2]["state"][0])


def test_more_rows_than_one_trip_of_the_assign_scan():
    import mmsa
    counts = [int(c[0]) for c, _, _ in TR.tables("blobs")]
    assert max(counts) > TR.TRIP == mmsa.lib.raw.mmsa_track_trip()
    _, tr, want = _drive("blobs", pair_capacity=8192)
    behind = want[3]["state"][0, TR.TRIP:counts[3]]
    assert (behind[:, TR.PREV] >= 0).any() and (behind[:, TR.PREV] < 0).any()      # continued and born rows behind the first trip, numbered from its carry


@pytest.mark.parametrize("same_class", [True, False])
def test_hand_made_cases(same_class):
    st, tr, want = _drive("hand", same_class=same_class)
    _, at = TR.hand()
    ids, s = _host(st.ids)[0], _host(tr.state)[0]
    row = lambda name: ids[at[name][1], at[name][2]]      # noqa: E731  (the names of the second frame)
    assert s[row("half_cur"), TR.PREV] == -1 and s[row("twothirds_cur")].tolist()[1:] == [2, TR.tables("hand")[0][1][0, 3, 2], 4]
    assert s[row("split_left"), TR.INTER] == 6 and s[row("split_right"), TR.PREV] == -1 and s[row("even_left"), TR.PREV] == -1 == s[row("even_right"), TR.PREV]
    assert s[row("merge_cur"), TR.INTER] == 7 and s[row("tie_cur"), TR.PREV] == -1 and (s[row("class_cur"), TR.PREV] >= 0) == (not same_class)
    rows = tr.host(0)
    assert len(rows) == 11 and rows["iou"][row("twothirds_cur")] == 4 / 6 and np.isnan(rows["iou"][row("half_cur")]) and rows["track"].tolist() == s[:11, TR.TRACK].tolist()
    info = tr.segments_info(0)
    assert [d["track_id"] for d in info] == rows["track"].tolist() and [d["age"] for d in info] == rows["age"].tolist() and info[0]["id"] == 1
    assert tr.summary() == dict(alive=11, continued=int(want[1]["totals"][0, 0]), born=int(want[1]["totals"][0, 1]), ended=int(want[1]["totals"][0, 2]),
                                mean_age=float(s[:11, TR.AGE].sum()) / 11)


# ---- 2. what is never silent

def test_a_table_smaller_than_its_segments():
    st, tr, want = _drive("noise", capacity=100)
    assert st.overflow() and int(_host(tr.stats)[0, 1]) > 0 and (_host(st.ids) >= 100).any()
    assert ((_host(tr.tracks) >= 0) == ((_host(st.ids) >= 0) & (_host(st.ids) < 100))).all()      # ids beyond the rows take part nowhere
    for call in (tr.host, lambda: tr.host(0), lambda: tr.segments_info(0), tr.summary):
        with pytest.raises(RuntimeError, match=r"image 0 has \d+ listed segments and the table 100 rows.*capacity="):
            call()
    assert tuple(tr.keep(min_age=1).shape) == (1, 100)      # the device mask needs no complete table


def test_a_pair_table_that_overflows():
    import mmsa
    name, capacity, same_class, pair_capacity, resets, overflows = TR.CASES[-1]
    assert (name, pair_capacity, overflows) == ("ragged", 2, True)
    seq = TR.sequence(name)
    st = mmsa.SegmentTable(num_classes=C, capacity=67 * 131)
    tr = mmsa.SegmentTracker(st, pair_capacity=2)
    st.update(_dev(seq[0]))
    tr.update()
    assert tr.overflow() == 0 and len(tr.host()) == int(_host(st.count).sum())      # a first frame forms no key
    st.update(_dev(seq[1]))
    tr.update()
    torch.cuda.synchronize()                                                    # nothing hangs: two slots, a bounded walk
    lost = tr.overflow()
    keys, inters = _pairs(tr)
    want_keys, want_inters = TR.pairs_of(TR.tables(name)[1][1], TR.tables(name)[0][1], 67 * 131)
    assert 0 < lost == want_inters.sum() - inters.sum() and len(keys) == 2 and set(keys.tolist()) <= set(want_keys.tolist())
    assert all(inters[i] == want_inters[np.searchsorted(want_keys, keys[i])] for i in range(2))      # what has a slot is complete
    for call in (tr.host, lambda: tr.segments_info(0), tr.summary):
        with pytest.raises(RuntimeError, match=r"the pair table of 2 slots overflowed \(\d+ pixels.*pair_capacity="):
            call()
    assert tr.reset().overflow() == 0


def test_entry_limits_are_refused_before_any_launch():
    import mmsa
    ids = torch.zeros(1, 4, 4, dtype=torch.int32, device=DEV)
    with pytest.raises(ValueError, match="capacity = 6 is not a power of two"):
        mmsa.track_pairs(ids, ids.clone(), 16, capacity=6)
    with pytest.raises(ValueError, match="rows = 0"):
        mmsa.track_pairs(ids, ids.clone(), 0)
    with pytest.raises(RuntimeError, match=r"ids_prev is \(1, 4, 5\)"):
        mmsa.track_pairs(ids, torch.zeros(1, 4, 5, dtype=torch.int32, device=DEV), 16)
    t = mmsa.PairTable.empty(8, DEV)
    p = ids.data_ptr()
    with pytest.raises(RuntimeError, match=r"track_pairs: rows = 0 per image"):
        mmsa.lib.call("mmsa_track_pairs", p, p, 1, 4, 4, 0, t.keys.data_ptr(), t.counts.data_ptr(), 8, t.overflow.data_ptr(), None)
    with pytest.raises(RuntimeError, match=r"track_pairs: capacity = 6; a power of two"):
        mmsa.lib.call("mmsa_track_pairs", p, p, 1, 4, 4, 16, t.keys.data_ptr(), t.counts.data_ptr(), 6, t.overflow.data_ptr(), None)
    with pytest.raises(RuntimeError, match=r"track_update: ids_cur, count, records, .* are required"):
        mmsa.lib.call("mmsa_track_update", t.keys.data_ptr(), t.counts.data_ptr(), 8, p, None, None, 1, 4, 4, 16, 1, *([None] * 10), None)
    st = mmsa.SegmentTable(num_classes=C, capacity=16)
    tr = mmsa.SegmentTracker(st)
    st.update(torch.zeros(1, 4, 4, dtype=torch.uint8, device=DEV))
    tr.update()
    assert tr.overflow() == 0 and _pairs(tr)[0].size == 0                       # a first frame forms no key: nothing to predict, nothing to drop
    st.update(torch.zeros(1, 4, 5, dtype=torch.uint8, device=DEV))
    with pytest.raises(RuntimeError, match=r"the table holds a \(1, 4, 5\) batch of 16 rows .* the tracker follows \(1, 4, 4\)"):
        tr.update()


# ---- 3. the maps and masks that go on

def test_track_pairs_alone_and_the_tracks_map_through_the_run_tables():
    import mmsa
    st, tr, want = _drive("ragged")
    tabs = TR.tables("ragged")
    R = 67 * 131
    table = mmsa.track_pairs(_dev(tabs[3][1]), _dev(tabs[2][1]), R)
    image, cur, prev, inter = table.host()
    assert isinstance(table, mmsa.PairTable) and table.shape == (3, 1, R) and int(table.overflow.item()) == 0
    assert np.array_equal(((image * R + cur) << 31) | prev, want[3]["keys"]) and np.array_equal(inter, want[3]["inters"])
    again = mmsa.track_pairs(_dev(tabs[3][1]), _dev(tabs[2][1]), R, table=table)
    assert again is table and np.array_equal(table.host()[3], want[3]["inters"])
    for order in ("row", "column"):
        runs = mmsa.run_lengths(tr.tracks, order=order, capacity=R)
        assert torch.equal(mmsa.run_decode(runs), tr.tracks)
    off = mmsa.SegmentTracker(st, tracks=False)
    assert off.update().tracks is None and torch.equal(off.state[..., TR.AGE], (tr.state[..., TR.TRACK] >= 0).to(torch.int32))      # a tracker of its own: a first frame


def test_keep_by_age_through_select_segments():
    import mmsa
    st, tr, want = _drive("ragged")
    pred = _dev(TR.sequence("ragged")[3])
    state, records, ids = want[3]["state"], TR.tables("ragged")[3][2], TR.tables("ragged")[3][1]
    for kw in (dict(min_age=2), dict(min_age=3), dict(max_age=2), dict(min_age=2, max_age=4), dict(tracks=[0, 1, 2, 3, 5, 8, 13])):
        keep = tr.keep(**kw)
        want_keep = TR.keep(state, **kw)
        assert keep.dtype == torch.uint8 and tuple(keep.shape) == (3, st.capacity) and np.array_equal(_host(keep), want_keep) and want_keep.any(), kw
    both = st.keep(min_area=2) & tr.keep(min_age=2)
    want_both = SR.keep(records, min_area=2) & TR.keep(state, min_age=2)
    got = mmsa.select_segments(pred, st, both, fill=254)
    want_map = SR.select(_host(pred), ids, want_both, 254)
    assert np.array_equal(_host(got), want_map) and (want_map == 254).any() and (want_map != 254).any()
    filled = mmsa.select_segments(pred, st, both, fill=254, nearest=32)
    assert torch.equal(filled, mmsa.fill_nearest(got, hole=254, cap=32)) and not (filled == 254).all()
    with pytest.raises(ValueError, match="min_age = 0"):
        tr.keep(min_age=0)
    with pytest.raises(ValueError, match=r"tracks = \[-1\]"):
        tr.keep(tracks=[-1])


# ---- 4. captured, through the runner, and run after run

def test_three_replays_of_a_captured_update_equal_the_eager_sequence():
    import mmsa
    seq = TR.sequence("ragged")
    want, tabs = TR.run("ragged"), TR.tables("ragged")
    st = mmsa.SegmentTable(num_classes=C, capacity=67 * 131)
    tr = mmsa.SegmentTracker(st, tracks=True)
    st.update(_dev(seq[0]))
    tr.update()                                                                 # frame 0, eager: the buffers exist
    _same(st, tr, want[0], tabs[0])
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        tr.update()                                                             # captured, not run: fixed addresses, no pointer swap
    for t in (1, 2, 3):
        st.update(_dev(seq[t]))                                                 # the table refilled, into the buffers the graph reads
        graph.replay()
        torch.cuda.synchronize()
        _same(st, tr, want[t], tabs[t], t)


def test_slide_runner_tracks_its_frames(models):  # noqa: F811
    import mmsa
    import mmsa.dist
    import mmsa.inference as inf
    cfg, m, h, frame, x = models
    sr = inf.SlideRunner(m, h, frame.clone(), (256, 256), (170, 170), chains=2, confidence=True)
    R = 320 * 400
    st, by_hand = mmsa.SegmentTable(num_classes=NUM_CLASSES, capacity=R), mmsa.SegmentTable(num_classes=NUM_CLASSES, capacity=R)
    tr, tr_hand = mmsa.SegmentTracker(st, tracks=True), mmsa.SegmentTracker(by_hand, tracks=True)
    plain = None
    for t in range(3):
        sr.frame.copy_(torch.roll(frame, shifts=(t, 2 * t), dims=(2, 3)))       # the same scene moved by (1, 2) px per frame
        res = sr.run(segment_table=st, tracker=tr)
        cm, conf = res.outputs()[0].clone(), res.confidence().clone()
        by_hand.update(cm, values=conf)
        tr_hand.update()
        for name in ("state", "stats", "totals", "next_track", "tracks"):
            assert torch.equal(getattr(tr, name), getattr(tr_hand, name)), (t, name)
        assert torch.equal(st.records, by_hand.records) and tr.overflow() == 0
        if t == 2:
            plain = sr.run(segment_table=st).outputs()[0].clone()               # tracker=None: the frame's map as before, the tracker untouched
            assert torch.equal(plain, cm) and torch.equal(tr.totals, tr_hand.totals)
    assert int(_host(tr.totals)[0, 1]) > 0 and int(_host(tr.stats)[0, :2].sum()) == int(_host(st.count)[0])      # continued + born = the frame's segments
    assert mmsa.dist.allreduce_counts(tr.totals) is tr.totals
    with pytest.raises(RuntimeError, match="mmsa.SlideRunner.run: tracker= needs segment_table="):
        sr.run(tracker=tr)
    with pytest.raises(RuntimeError, match="mmsa.SlideRunner.run: tracker= is bound to another SegmentTable"):
        sr.run(segment_table=by_hand, tracker=tr)


def test_the_same_bytes_on_a_second_run_and_no_allocation():
    import mmsa
    runs = []
    for _ in range(2):
        st, tr, _ = _drive("blobs", pair_capacity=8192)
        runs.append([_host(t).tobytes() for t in (tr.state, tr.stats, tr.totals, tr.next_track, tr.tracks, tr.succ, tr.prev_area)] + [a.tobytes() for a in _pairs(tr)])
    assert runs[0] == runs[1]
    again = ("blobs_again", None, True, 8192, (), False)
    assert again in TR.CASES and all(np.array_equal(a, b) for a, b in zip(TR.sequence("blobs_again")[:5], TR.sequence("blobs")))      # these updates are predicted too
    d = _dev(TR.sequence("blobs_again")[7])
    torch.cuda.synchronize()
    before = torch.cuda.memory_allocated()
    for _ in range(3):
        st.update(d)
        tr.update()
    torch.cuda.synchronize()
    assert torch.cuda.memory_allocated() == before                              # a later update allocates nothing
    _same(st, tr, TR.run(*again[:3])[7], TR.tables("blobs_again")[7], "blobs_again")
    n = int(_host(st.count)[0])
    assert _host(tr.stats)[0].tolist() == [n, 0, 0] and _host(tr.state)[0, :n, TR.AGE].min() >= 4      # the same frame again: every segment continues itself
