"""Timing of the segment tracker for profiles/segment_tracker.txt.  Legs interleaved in ONE process, every repetition timing each leg once (order rotated),
`--inner` calls per timing between two events on the launch stream, all on stored maps and into given buffers.  Consecutive frames = the class map of the
seeded logits (frame 0) and the same map moved by 2 px down and right (frame 1).  A tracker is bound to ONE table, so the stream is timed as a user runs it:
the table is refilled with the other frame before every tracker update, and the table's share is taken off with a leg that does the refills alone:
  (tp)    mmsa_track_pairs alone, ids of frame 1 against ids of frame 0: the launch that empties the table and the pair launch, at the default capacity;
  (st)    SegmentTable.update() of frame 1, then of frame 0, per update: the call the tracker follows (yardstick);
  (sup)   table.update(frame 1), tracker.update(), table.update(frame 0), tracker.update(), per frame, without `tracks`;   (supt) with tracks=True;
  (upd)   = (sup) - (st), the full SegmentTracker.update() (mmsa_track_pairs + mmsa_track_update: six launches), a difference of two medians;
          (updt) = (supt) - (st);
  (noi)   the worst case of the in-wave reduction and of the table: SegmentTracker.update() of a 25-class NOISE map against itself at capacity = H * W --
          every pixel a pair of its own segment, 64 keys in most waves;   (one) a one-code map against itself: one key takes every add;
  yardsticks on the same maps: (pa) mmsa_segment_pairs and (pm) mmsa_eval_panoptic of frame 1 against frame 0 as labels (the launches of the same kind),
          (e) mmsa_eval_confusion_u8 (the floor);
  (host)  the route a user had, timed with the wall clock (3 repetitions): copy both ids maps to the host, then numpy.unique over the paired ids.
Before anything is timed every device result is checked on the full-size maps: state, stats, tracks and the sorted pair list of both updates against the numpy
restatement of tests/segment_tracker_ref.py (fed with the device's own tables: it judges the tracker, not the table a second time), and the two worst cases
against their closed form (every segment continues itself).
Workloads, 25 classes, as tools/exp/segment_table_bench.py: two 1024 x 1024 maps and the 1080 x 1920 frame.  No threshold: the medians and p10 .. p90 are
the record."""
import argparse
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "multimodal-sam-adapter_amd"))
sys.path.insert(0, ROOT)


def restatement_check(frames, st, tr, R):
    """table `st` refilled with the frames in turn and its tracker `tr` (tracks=True, fresh) updated behind it, against the restatement -> the stats of the
    last update."""
    from tests import segment_tracker_ref as TR
    ref = TR.Tracker(frames[0].shape[0], R)
    for f in frames:
        st.update(f)
        tr.update()
        want = ref.update(st.count.cpu().numpy(), st.ids.cpu().numpy(), st.records.cpu().numpy())
        assert tr.overflow() == 0
        for name in ("state", "stats", "totals", "next_track", "tracks"):
            assert np.array_equal(getattr(tr, name).cpu().numpy(), want[name]), f"{name} differs from the restatement"
        image, cur, prev, inter = tr.pairs.host()
        assert np.array_equal(((image * R + cur) << 31) | prev, want["keys"]) and np.array_equal(inter, want["inters"]), "the pair list differs"
    return want["stats"].tolist()


def host_route(ids_cur, ids_prev):
    """copy, then numpy.unique over the paired ids: the intersections of every (current, previous) pair of every image."""
    a, b = ids_cur.cpu().numpy().astype(np.int64), ids_prev.cpu().numpy().astype(np.int64)
    n = 0
    for x, y in zip(a, b):
        both = (x >= 0) & (y >= 0)
        n += len(np.unique((x[both] << 31) | y[both], return_counts=True)[0])
    return n


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--inner", type=int, default=3)
    ap.add_argument("--out", default=None)
    ap.add_argument("--tag", default="", help="a line for the head of the report: which build this is")
    ap.add_argument("--no-host", action="store_true", help="skip the host alternative (variant runs)")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("segment_tracker_bench: no GPU (a timing needs one)")
    import mmsa
    import mmsa.inference as inf
    from mmsa.evaluate import LabelPrep, PairTable, SegmentTable, SegmentTracker, default_pair_capacity
    import torch.nn.functional as F
    dev = torch.device("cuda", 0)
    lines = []
    C = 25

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    def logits(n, g):
        coarse = torch.randn(n, C, 32, 32, generator=g)
        return (F.interpolate(coarse, size=(256, 256), mode="bilinear") + 0.05 * torch.randn(n, C, 256, 256, generator=g)).to(dev)

    say(f"device {torch.cuda.get_device_name(0)}; reps {a.reps}, {a.inner} calls per timing; times in microseconds per call; {C} classes"
        + (f"; {a.tag}" if a.tag else ""))
    g = torch.Generator().manual_seed(7)
    lp = LabelPrep(C)
    for name, plan in (("two 1024 x 1024 maps", inf.MapPlan.whole(2, 1024, 1024)),
                       ("1080 x 1920 frame, six windows", inf.MapPlan.slide(1, 1080, 1920, (1024, 1024), (640, 640)))):
        lg = logits(plan.n, g)
        B, H, W = plan.B, plan.Ho, plan.Wo
        frame0 = torch.empty(B, H, W, dtype=torch.uint8, device=dev)
        unc = torch.zeros(1, dtype=torch.int32, device=dev)
        plan.class_map(lg, frame0, unc)
        assert int(unc.item()) == 0
        del lg
        frame1 = torch.roll(frame0, (2, 2), (1, 2)).contiguous()
        noise = torch.randint(0, C, (B, H, W), generator=g, dtype=torch.uint8).to(dev)
        one = torch.full((B, H, W), 7, dtype=torch.uint8, device=dev)
        npx = B * H * W
        st0, st1, st_upd = (SegmentTable(num_classes=C) for _ in range(3))
        st_noise, st_one = SegmentTable(num_classes=C, capacity=H * W), SegmentTable(num_classes=C)
        st0.update(frame0)
        st1.update(frame1)
        st_noise.update(noise)
        st_one.update(one)
        assert not st0.overflow() and not st1.overflow() and not st_noise.overflow()
        R = st0.capacity
        counts = [st0.count.cpu().tolist(), st1.count.cpu().tolist()]
        n_noise = st_noise.count.cpu().tolist()
        # checks first, on trackers of their own
        st_chk = SegmentTable(num_classes=C)
        stats = restatement_check((frame0, frame1, frame0), st_chk, SegmentTracker(st_chk, tracks=True), R)
        cap_n = default_pair_capacity(npx)
        while cap_n < 2 * sum(n_noise):
            cap_n *= 2
        tr_noise, tr_one = SegmentTracker(st_noise, pair_capacity=cap_n), SegmentTracker(st_one)
        for tr, st in ((tr_noise, st_noise), (tr_one, st_one)):
            tr.update().update()
            n = st.count.cpu()
            assert tr.overflow() == 0 and tr.stats.cpu().tolist() == [[int(v), 0, 0] for v in n], "a map against itself: every segment continues itself"
            for b in range(B):
                assert torch.equal(tr.state[b, :int(n[b]), 2].cpu(), torch.arange(int(n[b]), dtype=torch.int32))
        st_a, st_b = SegmentTable(num_classes=C), SegmentTable(num_classes=C)      # each the ONE table of its tracker
        tr, trt = SegmentTracker(st_a), SegmentTracker(st_b, tracks=True)
        t_pairs = PairTable.empty(default_pair_capacity(npx), dev)
        rp, rl = mmsa.components(frame1, num_classes=C), mmsa.components(frame0, labels_prep=lp)
        planes = torch.empty(4, B, H, W, dtype=torch.int32, device=dev)
        mmsa.segment_counts(frame1, frame0, lp, rp, rl, 1, scratch=planes)
        t_pan = PairTable.empty(default_pair_capacity(npx), dev)
        match = torch.empty(2, B, H, W, dtype=torch.int32, device=dev)
        pq = torch.zeros(B, C, 24, 4, dtype=torch.int64, device=dev)
        ebuf = torch.zeros(B, C + 1, C + 1, dtype=torch.int64, device=dev)

        def stream(table, tracker):
            def leg():
                for f in (frame1, frame0):
                    table.update(f)
                    if tracker is not None:
                        tracker.update()
            return leg

        legs = dict(
            tp=lambda: mmsa.track_pairs(st1.ids, st0.ids, R, table=t_pairs),
            st=stream(st_upd, None), sup=stream(st_a, tr), supt=stream(st_b, trt),
            noi=lambda: tr_noise.update(),
            one=lambda: tr_one.update(),
            pa=lambda: mmsa.segment_pairs(frame1, frame0, lp, rp, rl, table=t_pan),
            pm=lambda: mmsa.panoptic_counts(frame1, frame0, lp, rp, rl, planes, t_pan, counts=pq, match=match),
            e=lambda: mmsa.confusion(frame1, frame0, lp, counts=ebuf))
        per_call = dict(st=2, sup=2, supt=2)                                     # frames per call of the leg
        what = dict(tp="mmsa_track_pairs alone, ids of frame 1 against ids of frame 0",
                    st="SegmentTable.update(), frames 1 and 0 in turn, per frame (yardstick: the call it follows)",
                    sup="table.update() + tracker.update(), frames 1 and 0 in turn, per frame, no tracks", supt="the same with tracks=True", noi="SegmentTracker.update(), 25-class noise map against itself, capacity = H * W",
                    one="SegmentTracker.update(), one-code map against itself: one key takes every add",
                    pa="mmsa_segment_pairs, frame 1 against frame 0 as labels (yardstick: the same kind of launch)",
                    pm="mmsa_eval_panoptic on that table (yardstick: match + count launches)",
                    e="mmsa_eval_confusion_u8 (the floor)")
        for _ in range(2):
            for k in legs:
                legs[k]()
        torch.cuda.synchronize()
        assert tr.overflow() == 0 and trt.overflow() == 0 and int(t_pairs.overflow.item()) == 0 and int(t_pan.overflow.item()) == 0
        times = {k: [] for k in legs}
        order = list(legs)
        for rep in range(a.reps):
            for k in order[rep % len(order):] + order[:rep % len(order)]:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(a.inner):
                    legs[k]()
                e1.record()
                e1.synchronize()
                times[k].append(e0.elapsed_time(e1) * 1e3 / (a.inner * per_call.get(k, 1)))
        say()
        say(f"{name}: {npx} pixels; state, stats, totals, next_track, tracks and the sorted pair list of three updates (frame 0, 1, 0) equal the numpy "
            f"restatement on the full-size maps; segments per image {counts[0]} / {counts[1]} at capacity {R}, the last update's continued / born / ended "
            f"{stats}; pair table {t_pairs.capacity} slots; noise map {n_noise} segments at capacity {H * W}, pair table {cap_n} slots: it and the one-code "
            f"map continue every segment")
        med = {}
        for k in legs:
            t = np.array(times[k])
            med[k] = float(np.median(t))
            say(f"  ({k:4s}) {what[k]:100s} median {med[k]:10.2f}   p10 {np.percentile(t, 10):10.2f}   p90 {np.percentile(t, 90):10.2f}")
        span = {k: float(np.percentile(times[k], 90) - np.percentile(times[k], 10)) for k in legs}
        med["upd"], med["updt"] = med["sup"] - med["st"], med["supt"] - med["st"]
        say(f"  (upd ) SegmentTracker.update(), no tracks = (sup) - (st) = {med['upd']:.2f}; (updt) with tracks = (supt) - (st) = {med['updt']:.2f} (differences of "
            f"medians; the spans of their terms: (sup) {span['sup']:.2f}, (supt) {span['supt']:.2f}, (st) {span['st']:.2f})")
        say(f"  (tp) / (pa) = {med['tp'] / med['pa']:.2f} x; (upd) / ((pa) + (pm)) = {med['upd'] / (med['pa'] + med['pm']):.2f} x; (upd) / (st) = "
            f"{med['upd'] / med['st']:.2f} x; (updt) - (upd) = {med['updt'] - med['upd']:.2f}; (upd) - (tp) = {med['upd'] - med['tp']:.2f} (clear, match, "
            f"assign, carry); (upd) / (e) = {med['upd'] / med['e']:.2f} x; (noi) / (upd) = {med['noi'] / med['upd']:.2f} x, (one) / (upd) = "
            f"{med['one'] / med['upd']:.2f} x; p10 .. p90 spans: (pa) {span['pa']:.2f}, (pm) {span['pm']:.2f}, (st) {span['st']:.2f}, (e) {span['e']:.2f}")
        if not a.no_host:
            ts = []
            for _ in range(3):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                nh = host_route(st1.ids, st0.ids)      # st0 / st1: the tables of frame 0 / 1, filled once, for (tp) and this route
                ts.append((time.perf_counter() - t0) * 1e3)
            say(f"  (host) copy both ids maps + numpy.unique over the paired ids: {nh} pairs, {min(ts):.1f} .. {max(ts):.1f} ms per batch (wall clock, 3 "
                f"repetitions), {np.median(ts) * 1e3 / med['upd']:.0f} x (upd)")
        del frame0, frame1, noise, one, st0, st1, st_upd, st_a, st_b, st_chk, st_noise, st_one, tr, trt, tr_noise, tr_one, t_pairs, t_pan, planes, match, rp, rl
        torch.cuda.empty_cache()
    say()
    say("not measured: hardware counters; the launches of mmsa_track_update one by one (no kernel trace was taken: (upd) - (tp) is their sum); "
        "(upd) itself is a difference of two medians, not a timed interval")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
