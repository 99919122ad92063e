"""The segment tracker without a GPU: the numpy restatement of tests/segment_tracker_ref.py against a brute-force statement from sets of pixels and Fractions,
the uniqueness of matches, the hand-made cases, the host readings on hand-made state, the refusals, the exports, and -- for every tracker of
tests/test_segment_tracker_gpu.py -- the pair table of every update: no key can be dropped there, or one must be where the test wants the overflow."""
import inspect
from fractions import Fraction

import numpy as np
import pytest

from tests import components_ref as CR
from tests import panoptic_ref as PR
from tests import segment_table_ref as SR
from tests import segment_tracker_ref as TR


def _frames(seed, H, W, T):
    """T frames of `components_ref.blocky` shifted by 0-2 px with some pixels re-drawn, as one-image tables at capacity H * W."""
    out = []
    for f in TR.moving(seed, H, W, T, salt=0.03, lo=3, hi=9):
        out.append(SR.table_batch([f], [CR.roots(f)], capacity=H * W))
    return out


# ---- 1. the restatement against sets of pixels

@pytest.mark.parametrize("same_class", [True, False])
@pytest.mark.parametrize("seed,H,W", [(1, 17, 23), (2, 9, 40), (3, 30, 30), (4, 1, 50), (5, 25, 1)])
def test_restatement_equals_brute_force(seed, H, W, same_class):
    R = H * W
    tabs = _frames(seed, H, W, 4)
    tr = TR.Tracker(1, R, same_class)
    live = {}                                                                   # id of the previous frame -> (track, age), kept from sets alone
    next_track = continued = 0
    for t, (count, ids, records) in enumerate(tabs):
        got = tr.update(count, ids, records)
        n = int(count[0])
        cls = records[0, :n, SR.CLASS]
        matches = {} if t == 0 else TR.brute_force(ids[0], cls, tabs[t - 1][1][0], tabs[t - 1][2][0, :, SR.CLASS], R, same_class)
        assert all(len(v) == 1 for v in matches.values())                       # at most one j per k ...
        js = [v[0][0] for v in matches.values()]
        assert len(set(js)) == len(js)                                          # ... and one k per j
        now, born = {}, 0
        for k in range(n):
            row = got["state"][0, k]
            if k in matches:
                j, iou = matches[k][0]
                track, age = live[j]
                now[k] = (track, age + 1)
                inter = int(row[TR.INTER])
                assert row[TR.PREV] == j and Fraction(inter, int(records[0, k, SR.AREA]) + int(got["prev_area"][0, k]) - inter) == iou > Fraction(1, 2)
            else:
                now[k] = (next_track + born, 1)
                born += 1
                assert row[TR.PREV] == -1 and row[TR.INTER] == 0 and got["prev_area"][0, k] == 0
            assert (row[TR.TRACK], row[TR.AGE]) == now[k], (t, k)
        next_track += born
        assert got["stats"][0].tolist() == [n - born, born, len(live) - len(matches)] and got["next_track"][0] == next_track
        assert (got["state"][0, n:] == TR.UNMATCHED).all()
        assert np.array_equal(got["tracks"][0], np.array([now[k][0] for k in range(n)], dtype=np.int32)[ids[0]])      # every pixel is listed here
        continued += len(matches)
        live = now
    assert continued > 0 and tr.totals[0].tolist()[0] == continued and tr.totals[0, 1] == next_track


def test_uniqueness_holds_with_and_without_the_class_test():
    """The restatement asserts `at most one` both ways inside update(); here the brute force shows it on frames where classes are few, so that a segment
    overlaps many segments of its own class."""
    for seed in range(6):
        H, W = 24, 31
        a, b = TR.moving(50 + seed, H, W, 2, salt=0.1, classes=3, lo=2, hi=6)
        ta, tb = (SR.table_batch([f], [CR.roots(f)], capacity=H * W) for f in (a, b))
        for same_class in (True, False):
            m = TR.brute_force(tb[1][0], tb[2][0, :, SR.CLASS], ta[1][0], ta[2][0, :, SR.CLASS], H * W, same_class)
            js = [j for v in m.values() for j, _ in v]
            assert all(len(v) == 1 for v in m.values()) and len(set(js)) == len(js)
        strict = TR.brute_force(tb[1][0], tb[2][0, :, SR.CLASS], ta[1][0], ta[2][0, :, SR.CLASS], H * W, True)
        assert set(strict) <= set(m) and all(m[k] == v for k, v in strict.items())      # the class test only removes candidates


# ---- 2. hand-made cases

def _row_of(tabs, at, name):
    t, y, x = at[name]
    return int(tabs[t][1][0, y, x])


@pytest.mark.parametrize("same_class", [True, False])
def test_hand_made_cases(same_class):
    frames, at = TR.hand()
    tabs = TR.tables("hand")
    first, second = TR.run("hand", same_class=same_class)
    s0, s1 = first["state"][0], second["state"][0]
    assert (s0[:11, TR.AGE] == 1).all() and first["stats"][0].tolist() == [0, 11, 0] and s0[:11, TR.TRACK].tolist() == list(range(11))
    row = lambda name: _row_of(tabs, at, name)      # noqa: E731
    born = lambda name: s1[row(name), TR.PREV] == -1 and s1[row(name), TR.AGE] == 1 and s1[row(name), TR.TRACK] >= 11      # noqa: E731
    ended = lambda name: second["succ"][0, row(name)] == -1      # noqa: E731

    def continues(cur, prev, inter):
        r = s1[row(cur)]
        return r[TR.PREV] == row(prev) and r[TR.TRACK] == s0[row(prev), TR.TRACK] and r[TR.AGE] == 2 and r[TR.INTER] == inter

    assert s1[0, TR.PREV] == 0 and s1[0, TR.AGE] == 2                                        # the background goes on
    assert born("half_cur") and ended("half_prev")                                           # IoU exactly 1/2: 3 * 2 == 3 + 3
    assert continues("twothirds_cur", "twothirds_prev", 4)                                   # IoU 2/3: 3 * 4 > 5 + 5
    assert continues("split_left", "split_prev", 6) and born("split_right")                  # the larger half inherits
    assert born("even_left") and born("even_right") and ended("even_prev")                   # 5 of 10: nobody does
    assert continues("merge_cur", "merge_long", 7) and ended("merge_short")
    assert born("tie_cur") and ended("tie_a") and ended("tie_b")
    assert born("new") and ended("gone")
    if same_class:
        assert born("class_cur") and ended("class_prev") and second["stats"][0].tolist() == [4, 7, 7]
    else:
        assert continues("class_cur", "class_prev", 9) and second["stats"][0].tolist() == [5, 6, 6]
    new = np.sort(s1[:11, TR.TRACK][s1[:11, TR.PREV] < 0])
    assert new.tolist() == list(range(11, 11 + len(new))) and second["next_track"][0] == 11 + len(new)      # handed out in ascending k


def test_a_gap_of_one_frame_ends_every_track():
    out = TR.run("gap")
    n = out[0]["stats"][0, 1]
    assert n > 0 and out[1]["stats"][0].tolist() == [0, 0, n] and (out[1]["state"][0] == TR.UNMATCHED).all()
    assert out[2]["stats"][0].tolist() == [0, n, 0] and out[2]["state"][0, :n, TR.TRACK].tolist() == list(range(n, 2 * n))      # the same frame again: new ids
    assert out[3]["stats"][0, 0] > 0 and out[3]["state"][0, :, TR.AGE].max() == 2
    one = TR.run("1x1")
    assert [o["stats"][0].tolist() for o in one] == [[0, 1, 0], [1, 0, 0], [0, 1, 1], [0, 0, 1], [0, 1, 0]]
    assert [o["state"][0, 0].tolist() for o in one] == [[0, 1, -1, 0], [0, 2, 0, 1], [1, 1, -1, 0], [-1, 0, -1, 0], [2, 1, -1, 0]]


def test_reset_and_rows_beyond_the_table():
    plain, reset = TR.run("ragged"), TR.run("ragged", resets=((2, 1),))
    for t in range(4):
        for b in (0, 2):
            assert np.array_equal(plain[t]["state"][b], reset[t]["state"][b])
    n = int(TR.tables("ragged")[2][0][1])
    assert reset[2]["stats"][1].tolist() == [0, n, 0] and reset[2]["state"][1, :n, TR.TRACK].tolist() == list(range(n)) and plain[2]["stats"][1, 0] > 0
    assert reset[3]["stats"][1, 0] > 0 and reset[3]["totals"][1, 1] == plain[3]["totals"][1, 1] + reset[2]["stats"][1, 1] - plain[2]["stats"][1, 1]
    cut = TR.run("noise", capacity=100)
    count, ids, _ = TR.tables("noise", 100)[1]
    assert count[0] > 100 and cut[1]["stats"][0].tolist() == [100, 0, 0] and cut[2]["stats"][0, 1] > 0
    assert ((cut[1]["tracks"][0] >= 0) == ((ids[0] >= 0) & (ids[0] < 100))).all() and (ids[0] >= 100).any()      # ids beyond the rows take part nowhere
    assert int(cut[1]["keys"].max() >> 31) < 100 and int((cut[1]["keys"] & ((1 << 31) - 1)).max()) < 100


def test_the_blob_sequence_takes_the_second_trip_of_the_scan():
    from mmsa.evaluate import TRACK_TRIP
    assert TRACK_TRIP == TR.TRIP
    out = TR.run("blobs")
    counts = [int(c[0]) for c, _, _ in TR.tables("blobs")]
    assert max(counts) > TR.TRIP and counts[2] > TR.TRIP and counts[3] > TR.TRIP
    s = out[3]["state"][0]
    behind = s[TR.TRIP:counts[3]]
    assert (behind[:, TR.PREV] >= 0).sum() > 50 and (behind[:, TR.PREV] < 0).sum() > 50      # continued and born rows behind the first trip
    born_before = int((s[:TR.TRIP, TR.PREV] < 0).sum())
    first_new = behind[behind[:, TR.PREV] < 0][0, TR.TRACK]
    assert born_before > 0 and first_new == out[2]["next_track"][0] + born_before            # the carry of the first trip


# ---- 3. the host readings, refusals and exports

def test_host_readings_on_hand_made_state():
    import mmsa
    from mmsa import evaluate as E
    assert E.TRACK_FIELDS == ("TRACK", "AGE", "PREV", "INTER") and (E.TRACK, E.AGE, E.PREV, E.INTER) == (TR.TRACK, TR.AGE, TR.PREV, TR.INTER)
    assert E.TRACK_STATS == ("continued", "born", "ended")
    rec = np.zeros((4, 10), dtype=np.int64)
    rec[:3, SR.AREA], rec[:3, SR.CLASS] = (6, 5, 1), (3, 3, 9)
    state = np.array([[7, 3, 2, 4], [12, 1, -1, 0], [0, 9, 0, 1], [-1, 0, -1, 0]], dtype=np.int32)
    prev_area = np.array([4, 0, 1, 0], dtype=np.int32)
    s = mmsa.track_records_of(rec, 3, state, prev_area, image=2)
    assert s.dtype == E.TRACK_DTYPE and s["image"].tolist() == [2, 2, 2] and s["track"].tolist() == [7, 12, 0] and s["age"].tolist() == [3, 1, 9]
    assert s["prev"].tolist() == [2, -1, 0] and s["area"].tolist() == [6, 5, 1] and s["category"].tolist() == [3, 3, 9]
    assert s["iou"][0] == 4 / 6 and np.isnan(s["iou"][1]) and s["iou"][2] == 1.0              # 4 / (6 + 4 - 4); NaN at birth
    assert len(mmsa.track_records_of(rec, 0, state, prev_area)) == 0
    with pytest.raises(RuntimeError, match=r"image 0 has 5 listed segments and the table 4 rows.*capacity="):
        mmsa.track_records_of(rec, 5, state, prev_area)
    with pytest.raises(ValueError, match=r"a tracker's state is an integer \[..., rows, 4\] array"):
        mmsa.track_records_of(rec, 3, state[:, :3], prev_area)
    with pytest.raises(ValueError, match="a tracker's state is an integer"):
        mmsa.track_records_of(rec, 3, state[:3], prev_area)
    with pytest.raises(ValueError, match=r"prev_area is an integer \[4\] array"):
        mmsa.track_records_of(rec, 3, state, prev_area[:2])
    totals = np.array([[5, 9, 4], [1, 2, 0]], dtype=np.int64)
    got = mmsa.track_summary_of(np.stack([state, state]), totals)
    assert got == dict(alive=6, continued=6, born=11, ended=4, mean_age=26 / 6)
    assert np.isnan(mmsa.track_summary_of(state[3:], totals[:1])["mean_age"])
    with pytest.raises(ValueError, match=r"a tracker's totals are an integer \[..., 3\] array"):
        mmsa.track_summary_of(state, totals[:, :2])
    assert TR.keep(state, min_age=3).tolist() == [1, 0, 1, 0] and TR.keep(state, max_age=3).tolist() == [0, 1, 0, 0] and TR.keep(state, tracks=[0, 12]).tolist() == [0, 1, 1, 0]


def test_constructor_and_call_refusals():
    import mmsa
    import mmsa.inference as inf
    st = mmsa.SegmentTable(num_classes=5)
    with pytest.raises(RuntimeError, match="mmsa.SegmentTracker: table takes an mmsa.evaluate.SegmentTable, got int"):
        mmsa.SegmentTracker(3)
    with pytest.raises(ValueError, match="mmsa.SegmentTracker: same_class = 1; True or False"):
        mmsa.SegmentTracker(st, same_class=1)
    with pytest.raises(ValueError, match="mmsa.SegmentTracker: tracks = 'yes'"):
        mmsa.SegmentTracker(st, tracks="yes")
    with pytest.raises(ValueError, match="mmsa.SegmentTracker: capacity = 100 is not a power of two"):
        mmsa.SegmentTracker(st, pair_capacity=100)
    tr = mmsa.SegmentTracker(st, same_class=False, pair_capacity=64, tracks=True)
    assert tr.table is st and (tr.same_class, tr.pair_capacity, tr.with_tracks) == (False, 64, True) and tr.state is None and tr.tracks is None
    assert tr.reset() is tr and tr.reset(0) is tr                               # nothing to forget yet
    for call in (tr.overflow, tr.host, tr.summary, tr.keep, lambda: tr.segments_info(0)):
        with pytest.raises(RuntimeError, match="nothing was tracked yet"):
            call()
    with pytest.raises(RuntimeError, match="nothing was filled yet"):
        tr.update()
    with pytest.raises(RuntimeError, match="ids_cur must be a contiguous int32"):
        mmsa.track_pairs(np.zeros((1, 2, 2), dtype=np.int32), None, 4)
    # SlideRunner.run(tracker=): only with the tracker's own table
    o = inf.MapOptions.of("SlideRunner")
    assert o.tracker is None and o.with_call("SlideRunner.run", segment_table=st, tracker=tr).tracker is tr
    with pytest.raises(RuntimeError, match="mmsa.SlideRunner.run: tracker= takes an mmsa.evaluate.SegmentTracker, got str"):
        o.with_call("SlideRunner.run", segment_table=st, tracker="tr")
    with pytest.raises(RuntimeError, match="mmsa.SlideRunner.run: tracker= needs segment_table="):
        o.with_call("SlideRunner.run", tracker=tr)
    with pytest.raises(RuntimeError, match="mmsa.SlideRunner.run: tracker= is bound to another SegmentTable"):
        o.with_call("SlideRunner.run", segment_table=mmsa.SegmentTable(num_classes=5), tracker=tr)


def test_exports_and_prototypes():
    import mmsa
    import mmsa.inference as inf
    from mmsa.lib import I, L, P
    for name in ("SegmentTracker", "track_pairs", "track_records_of", "track_summary_of"):
        assert getattr(mmsa, name) is getattr(mmsa.evaluate, name) and name in mmsa.__all__
    for name in ("mmsa_track_pairs", "mmsa_track_update", "mmsa_track_trip"):
        assert name in mmsa.lib.SIGNATURES and hasattr(mmsa.lib.raw, name)
    # the two prototypes of include/mmsa.h against the ctypes table, argument by argument
    assert mmsa.lib.SIGNATURES["mmsa_track_pairs"] == [P, P, I, I, I, I, P, P, L, P, P]
    assert mmsa.lib.SIGNATURES["mmsa_track_update"] == [P, P, L, P, P, P, I, I, I, I, I] + [P] * 11
    import os
    header = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include", "mmsa.h")).read()
    for name in ("mmsa_track_pairs", "mmsa_track_update"):
        proto = header[header.index(f"int {name}("):]
        args = [a.strip() for a in proto[proto.index("(") + 1:proto.index(");")].replace("\n", " ").split(",")]
        kinds = [P if "*" in a or a.startswith("mmsa_stream_t") else L if a.startswith("long ") else I for a in args]
        assert kinds == mmsa.lib.SIGNATURES[name], name
    assert mmsa.lib.raw.mmsa_track_trip() == TR.TRIP == mmsa.evaluate.TRACK_TRIP and mmsa.lib.version() == 114
    assert inspect.signature(inf.SlideRunner.run).parameters["tracker"].default is None
    for fn in (inf.slide_class_map, inf.whole_class_map, inf.class_map, inf.aug_class_map, inf.MapPlan.class_map):
        assert "tracker" not in inspect.signature(fn).parameters, fn.__qualname__      # a single frame has no previous one


# ---- 4. the pair tables of the GPU tests, predicted

def test_every_gpu_update_has_the_pair_table_its_test_expects():
    from mmsa.evaluate import default_pair_capacity
    overflowed = []
    for name, capacity, same_class, pair_capacity, resets, overflows in TR.CASES:
        B, H, W = TR.sequence(name)[0].shape
        cap = default_pair_capacity(B * H * W) if pair_capacity is None else pair_capacity
        certain = False
        for t, got in enumerate(TR.run(name, capacity, same_class, resets)):
            p = PR.table_prediction(got["keys"], cap)
            if overflows:
                certain = certain or p["overflow_certain"]
            else:
                assert p["overflow_impossible"], (name, t, p["longest_walk"], p["load"])
            assert int(got["inters"].sum()) <= B * H * W and (t > 0 or len(got["keys"]) == 0)      # a first frame forms no key
        assert certain == overflows, name
        overflowed += [name] * overflows
    assert overflowed == ["ragged"]
