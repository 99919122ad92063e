"""Timing of the segment table for profiles/segment_table.txt.  Legs interleaved in ONE process, every repetition timing each leg once (order rotated),
`--inner` calls per timing between two events on the launch stream, all on the same stored maps and into given buffers:
  (scan)  mmsa_segment_table on the class map with its roots given and capacity 1: the memset, the three launches of the prefix sum and an accumulate launch
          that writes ids and finds (almost) no row -- the table without its atomics;
  (tab)   mmsa_segment_table on the class map with its roots given, no values, at the default capacity; (tab) - (scan) is what the accumulate launch adds;
  (tabv)  the same with the confidence map as `values`;
  (upd)   the full SegmentTable.update(): mmsa_components_u8 + (tab);   (updv) with `values`;
  (sel)   mmsa_select_segments_u8 with keep = table.keep(min_area=64);
  (one)   the worst case of one address: a one-code map, every add on one row;   (noi) a 25-class noise map at capacity = H * W: 64 distinct ids in most waves;
  yardsticks on the same maps: (ar) mmsa_component_area, (su) suppress_small(min_area=64), (add) SegmentEvaluator.add(), (e) mmsa_eval_confusion_u8;
  (host)  the host alternative, timed with the wall clock (3 repetitions): copy the map to the host, then scipy.ndimage.label / find_objects / sum_labels per
          class present.
Before anything is timed the device table of image 0 is checked against scipy on the full-size map: per class the number of segments, their boxes
(find_objects), areas and score sums (sum_labels), in raster order of the first pixel.
The constants of csrc/segtable.hip are chosen by running this program on variant builds (tools/build_variant.sh ... segtable.hip -DSEGTAB_WAVE_ROUNDS=N
-DSEGTAB_BLOCK=N, loaded through MMSA_LIB, with --block N for the latter; tools/exp/jobs/segment_table_profile.sh).
Workloads, 25 classes, as tools/exp/components_bench.py: two 1024 x 1024 maps and the 1080 x 1920 frame.  No threshold: the medians and p10 .. p90 are the
record."""
import argparse
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "multimodal-sam-adapter_amd"))
sys.path.insert(0, ROOT)


def scipy_check(pred, conf, st, C):
    """The table of image 0 against scipy on the full-size map -> the number of segments."""
    from scipy import ndimage
    m = pred[0].cpu().numpy()
    v = conf[0].cpu().numpy()
    c = np.where(v > 0, np.where(v > 1, np.float32(1), v), np.float32(0)).astype(np.float32)
    q = (c * np.float32(1 << 24)).astype(np.int64).astype(np.float64)
    n = int(st.count[0])
    rec = st.records[0, :n].cpu().numpy()
    seen = 0
    for k in np.unique(m):
        lab, cnt = ndimage.label(m == k, np.ones((3, 3), dtype=int))
        rows = rec[rec[:, 1] == k]
        assert len(rows) == cnt, f"class {k}: {len(rows)} rows, scipy labels {cnt}"
        index = np.arange(1, cnt + 1)
        assert np.array_equal(rows[:, 2], ndimage.sum_labels(np.ones_like(lab), lab, index).astype(np.int64)), f"class {k}: areas"
        assert np.array_equal(rows[:, 9], ndimage.sum_labels(q, lab, index).astype(np.int64)), f"class {k}: score sums"
        box = np.array([(s[1].start, s[0].start, s[1].stop - 1, s[0].stop - 1) for s in ndimage.find_objects(lab)]).reshape(-1, 4)
        assert np.array_equal(rows[:, 3:7], box), f"class {k}: boxes"
        seen += cnt
    assert seen == n
    return n


def host_route(pred):
    """copy, then scipy per class present: labelling, boxes and areas of every image."""
    from scipy import ndimage
    m = pred.cpu().numpy()
    n = 0
    for img in m:
        for k in np.unique(img):
            lab, cnt = ndimage.label(img == k, np.ones((3, 3), dtype=int))
            ndimage.find_objects(lab)
            ndimage.sum_labels(np.ones_like(lab), lab, np.arange(1, cnt + 1))
            n += cnt
    return n


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--inner", type=int, default=3)
    ap.add_argument("--out", default=None)
    ap.add_argument("--tag", default="", help="a line for the head of the report: which build this is")
    ap.add_argument("--block", type=int, default=None, help="SEGTAB_BLOCK of the library loaded through MMSA_LIB (sizes the scratch)")
    ap.add_argument("--no-host", action="store_true", help="skip the host alternative (variant runs)")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("segment_table_bench: no GPU (a timing needs one)")
    import mmsa
    import mmsa.inference as inf
    from mmsa import evaluate as E
    from mmsa.evaluate import LabelPrep, SegmentEvaluator, SegmentTable
    import torch.nn.functional as F
    if a.block is not None:
        E.SEGTAB_BLOCK = a.block                 # the Python layer sizes the scratch by it
    dev = torch.device("cuda", 0)
    lines = []
    C = 25

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    def logits(n, g):
        coarse = torch.randn(n, C, 32, 32, generator=g)
        return (F.interpolate(coarse, size=(256, 256), mode="bilinear") + 0.05 * torch.randn(n, C, 256, 256, generator=g)).to(dev)

    say(f"device {torch.cuda.get_device_name(0)}; reps {a.reps}, {a.inner} calls per timing; times in microseconds per call; {C} classes; scan block "
        f"{E.SEGTAB_BLOCK} pixels" + (f"; {a.tag}" if a.tag else ""))
    g = torch.Generator().manual_seed(7)
    lp = LabelPrep(C)
    for name, plan in (("two 1024 x 1024 maps", inf.MapPlan.whole(2, 1024, 1024)),
                       ("1080 x 1920 frame, six windows", inf.MapPlan.slide(1, 1080, 1920, (1024, 1024), (640, 640)))):
        lg = logits(plan.n, g)
        B, H, W = plan.B, plan.Ho, plan.Wo
        pred = torch.empty(B, H, W, dtype=torch.uint8, device=dev)
        conf = torch.empty(B, H, W, dtype=torch.float32, device=dev)
        unc = torch.zeros(1, dtype=torch.int32, device=dev)
        plan.class_map(lg, pred, unc, conf=conf)
        assert int(unc.item()) == 0
        del lg
        lab = torch.roll(pred, (3, 2), (1, 2)).contiguous()
        noise = torch.randint(0, C, (B, H, W), generator=g, dtype=torch.uint8).to(dev)
        one = torch.full((B, H, W), 7, dtype=torch.uint8, device=dev)
        npx = B * H * W
        root, root_n, root_1 = (mmsa.components(m, num_classes=C) for m in (pred, noise, one))
        area = torch.empty_like(root)
        st, st_scan, st_upd = SegmentTable(num_classes=C), SegmentTable(num_classes=C, capacity=1), SegmentTable(num_classes=C)
        st_noise, st_one = SegmentTable(num_classes=C, capacity=H * W), SegmentTable(num_classes=C)
        st.update(pred, values=conf, root=root)
        n0 = scipy_check(pred, conf, st, C)
        counts = st.count.cpu().tolist()
        assert not st.overflow()
        keep = st.keep(min_area=64)
        out, sup = torch.empty_like(pred), torch.empty_like(pred)
        mmsa.select_segments(pred, st, keep, fill=255, out=out)
        mmsa.suppress_small(pred, 64, num_classes=C, out=sup)
        assert torch.equal(out, sup), "select_segments(keep(min_area=64)) is not suppress_small(64)"
        st_noise.update(noise, values=conf, root=root_n)
        st_one.update(one, values=conf, root=root_1)
        n_noise = st_noise.count.cpu().tolist()
        assert st_one.count.cpu().tolist() == [1] * B and int(st_one.records[0, 0, 2]) == H * W and int(st_one.records[0, 0, 7]) == H * W * (W - 1) // 2
        se = SegmentEvaluator(lp, images=B, device=dev)
        ebuf = torch.zeros(B, C + 1, C + 1, dtype=torch.int64, device=dev)
        legs = dict(
            scan=lambda: st_scan.update(pred, root=root),
            tab=lambda: st.update(pred, root=root),
            tabv=lambda: st.update(pred, values=conf, root=root),
            upd=lambda: st_upd.update(pred),
            updv=lambda: st_upd.update(pred, values=conf),
            sel=lambda: mmsa.select_segments(pred, st, keep, out=out),
            one=lambda: st_one.update(one, values=conf, root=root_1),
            noi=lambda: st_noise.update(noise, values=conf, root=root_n),
            ar=lambda: mmsa.component_areas(root, out=area),
            su=lambda: mmsa.suppress_small(pred, 64, num_classes=C, out=sup),
            add=lambda: se.add(pred, lab, slots=list(range(B))),
            e=lambda: mmsa.confusion(pred, lab, lp, counts=ebuf))
        what = dict(scan="mmsa_segment_table at capacity 1: memset, count, scan, id launches + an accumulate launch without rows",
                    tab="mmsa_segment_table, roots given, no values, default capacity", tabv="mmsa_segment_table, roots given, with values",
                    upd="SegmentTable.update(): mmsa_components_u8 + the table", updv="SegmentTable.update() with values",
                    sel="mmsa_select_segments_u8, keep = table.keep(min_area=64)", one="mmsa_segment_table of a one-code map, with values: one row takes every add",
                    noi="mmsa_segment_table of a 25-class noise map, with values, capacity = H * W", ar="mmsa_component_area of the class map's roots (yardstick)",
                    su="suppress_small(min_area=64): components + areas + pointwise (yardstick)",
                    add="SegmentEvaluator.add(): 2 x components + mmsa_eval_segments (yardstick)", e="mmsa_eval_confusion_u8 (the floor)")
        for _ in range(2):
            for k in legs:
                legs[k]()
        torch.cuda.synchronize()
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
                times[k].append(e0.elapsed_time(e1) * 1e3 / a.inner)
        say()
        say(f"{name}: {npx} pixels; the table of image 0 equals scipy.ndimage on the full-size map (label per class, find_objects, sum_labels of areas and "
            f"scores: {n0} segments); segments per image {counts} at capacity {st.capacity}, noise map {n_noise} at capacity {H * W}; "
            f"select_segments(keep(min_area=64)) equals suppress_small(64)")
        med = {}
        for k in legs:
            t = np.array(times[k])
            med[k] = float(np.median(t))
            say(f"  ({k:4s}) {what[k]:108s} median {med[k]:10.2f}   p10 {np.percentile(t, 10):10.2f}   p90 {np.percentile(t, 90):10.2f}")
        spread = float(np.percentile(times["e"], 90) - np.percentile(times["e"], 10))
        say(f"  accumulate = (tab) - (scan) = {med['tab'] - med['scan']:.2f}; values add (tabv) - (tab) = {med['tabv'] - med['tab']:.2f}; (upd) - (tab) = "
            f"{med['upd'] - med['tab']:.2f} (the components); (tab) / (ar) = {med['tab'] / med['ar']:.2f} x, (updv) / (su) = {med['updv'] / med['su']:.2f} x, (updv) / (add) = "
            f"{med['updv'] / med['add']:.2f} x; p10 .. p90 of (e) spans {spread:.2f}")
        if not a.no_host:
            ts = []
            for _ in range(3):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                nh = host_route(pred)
                ts.append((time.perf_counter() - t0) * 1e3)
            say(f"  (host) copy + scipy label / find_objects / sum_labels per class present: {nh} segments, {min(ts):.1f} .. {max(ts):.1f} ms per batch "
                f"(wall clock, 3 repetitions), {np.median(ts) * 1e3 / med['updv']:.0f} x (updv)")
        del pred, conf, lab, noise, one, root, root_n, root_1, area, st, st_scan, st_upd, st_noise, st_one, se, out, sup, keep
        torch.cuda.empty_cache()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
