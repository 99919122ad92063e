"""Timing of the panoptic passes for profiles/panoptic.txt.  Legs interleaved in ONE process, every repetition timing each leg once (order rotated),
`--inner` calls per timing between two events on the launch stream, all on the same stored maps and into given buffers:
  (add)   the yardstick: the full SegmentEvaluator.add() -- two component calls and mmsa_eval_segments -- which supplies the same components and planes;
  (pa)    mmsa_segment_pairs on the class map and its labels: two memsets and the pair launch, at the default capacity;
  (pm)    mmsa_eval_panoptic on that table: one memset, the match launch (a lane per slot) and the count launch (a lane per pixel);
  (padd)  the full PanopticEvaluator.add(): (add) at bins=1, (pa), (pm);
  (pan)   the worst case of the in-wave reduction and of the table: mmsa_segment_pairs of a 25-class NOISE map against ITSELF as labels -- every pixel a hit,
          64 distinct keys in most waves, as many pairs as the map has components -- at the smallest capacity that holds them at a load below 1/2;
  (pmn)   mmsa_eval_panoptic on that table;
  (pai)   mmsa_segment_pairs of the noise map against ANOTHER noise map: 1 pixel in 25 is a hit, every hit a pair of its own, at the default capacity;
  (e)     mmsa_eval_confusion_u8 on the same maps: the floor of any pass over them.
Before anything is timed: no table overflowed, the table grouped by label root is plane hit0 and grouped by prediction root plane hit1, and TP + FN is the
label side of SegmentEvaluator's counts.  Reported with the times: the pairs and the load of every table and the longest walk of a key to its first free slot
(the probe rule of tests/panoptic_ref.py applied to the occupied slots, which do not depend on the schedule) -- what PAIR_MAX_PROBES must stay above.
The library's two constants are chosen by running this program on variant builds (tools/build_variant.sh ... pairs.hip -DPAIR_WAVE_ROUNDS=N
-DPAIR_MAX_PROBES=N, loaded through MMSA_LIB; tools/exp/jobs/panoptic_profile.sh).
Workloads, 25 classes, as tools/exp/components_bench.py: two 1024 x 1024 maps and the 1080 x 1920 frame.  No threshold: the medians and p10 .. p90 are the
record."""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "multimodal-sam-adapter_amd"))
sys.path.insert(0, ROOT)

HASH_MUL = np.uint64(0x9E3779B97F4A7C15)


def table_stats(table):
    """(pairs, load, longest walk, overflow) of a PairTable, on the host."""
    keys = table.keys.cpu().numpy()
    cap = keys.size
    used = keys != -1
    n = int(used.sum())
    lost = int(table.overflow.item())
    if n == 0 or n == cap:
        return n, n / cap, n, lost
    with np.errstate(over="ignore"):
        homes = ((keys[used].astype(np.uint64) * HASH_MUL) >> np.uint64(64 - (cap.bit_length() - 1))).astype(np.int64)
    free = np.nonzero(~used)[0]
    nxt = free[np.searchsorted(free, homes) % len(free)]
    return n, n / cap, int(((nxt - homes) % cap).max()), lost


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--inner", type=int, default=3)
    ap.add_argument("--out", default=None)
    ap.add_argument("--tag", default="", help="a line for the head of the report: which build this is")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("panoptic_bench: no GPU (a timing needs one)")
    import mmsa
    import mmsa.inference as inf
    from mmsa.evaluate import LabelPrep, PairTable, PanopticEvaluator, SegmentEvaluator, default_pair_capacity
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
        pred = torch.empty(B, H, W, dtype=torch.uint8, device=dev)
        unc = torch.zeros(1, dtype=torch.int32, device=dev)
        plan.class_map(lg, pred, unc)
        assert int(unc.item()) == 0
        del lg
        lab = torch.roll(pred, (3, 2), (1, 2)).cpu()
        r = torch.rand(B, (H + 15) // 16, (W + 15) // 16, generator=g).repeat_interleave(16, 1).repeat_interleave(16, 2)[:, :H, :W]
        other = torch.randint(0, C, (B, (H + 15) // 16, (W + 15) // 16), generator=g, dtype=torch.uint8).repeat_interleave(16, 1).repeat_interleave(16, 2)[:, :H, :W]
        lab = torch.where(r < 0.04, other, lab)
        lab[(r >= 0.04) & (r < 0.07)] = 255
        lab = lab.contiguous().to(dev)
        noise = torch.randint(0, C, (B, H, W), generator=g, dtype=torch.uint8).to(dev)
        noise2 = torch.randint(0, C, (B, H, W), generator=g, dtype=torch.uint8).to(dev)
        npx = B * H * W

        def roots(p, l):
            return mmsa.components(p, num_classes=C), mmsa.components(l, labels_prep=lp)

        def planes_of(p, l, rp, rl):
            s = torch.empty(4, B, H, W, dtype=torch.int32, device=dev)
            mmsa.segment_counts(p, l, lp, rp, rl, 1, scratch=s)
            return s

        rp, rl = roots(pred, lab)
        rpn, rln = roots(noise, noise)
        rpi, rli = roots(noise, noise2)
        planes, planes_n = planes_of(pred, lab, rp, rl), planes_of(noise, noise, rpn, rln)
        n_noise = int((rpn == torch.arange(H * W, device=dev, dtype=torch.int32).view(1, H, W)).sum())
        cap_n = default_pair_capacity(npx)
        while cap_n < 2 * n_noise:
            cap_n *= 2
        t_map, t_noise, t_ind = (PairTable.empty(c, dev) for c in (default_pair_capacity(npx), cap_n, default_pair_capacity(npx)))
        match = torch.empty(2, B, H, W, dtype=torch.int32, device=dev)
        pq, pqn = (torch.zeros(B, C, 24, 4, dtype=torch.int64, device=dev) for _ in range(2))
        se, pe = SegmentEvaluator(lp, images=B, device=dev), PanopticEvaluator(lp, images=B, device=dev)
        ebuf = torch.zeros(B, C + 1, C + 1, dtype=torch.int64, device=dev)
        legs = dict(
            add=lambda: se.add(pred, lab, slots=list(range(B))),
            pa=lambda: mmsa.segment_pairs(pred, lab, lp, rp, rl, table=t_map),
            pm=lambda: mmsa.panoptic_counts(pred, lab, lp, rp, rl, planes, t_map, counts=pq, match=match),
            padd=lambda: pe.add(pred, lab, slots=list(range(B))),
            pan=lambda: mmsa.segment_pairs(noise, noise, lp, rpn, rln, table=t_noise),
            pmn=lambda: mmsa.panoptic_counts(noise, noise, lp, rpn, rln, planes_n, t_noise, counts=pqn, match=match),
            pai=lambda: mmsa.segment_pairs(noise, noise2, lp, rpi, rli, table=t_ind),
            e=lambda: mmsa.confusion(pred, lab, lp, counts=ebuf))
        what = dict(add="SegmentEvaluator.add(): 2 x components + mmsa_eval_segments (the yardstick)", pa="mmsa_segment_pairs, class map against its labels",
                    pm="mmsa_eval_panoptic on that table (match + count launches)", padd="PanopticEvaluator.add(): (add) at bins=1 + (pa) + (pm)",
                    pan="mmsa_segment_pairs, noise map against itself (every pixel a hit)", pmn="mmsa_eval_panoptic on the noise table",
                    pai="mmsa_segment_pairs, noise map against another noise map", e="mmsa_eval_confusion_u8 (the floor)")
        # checks first
        for k in ("pa", "pan", "pai"):
            legs[k]()
        torch.cuda.synchronize()
        stats = {k: table_stats(t) for k, t in (("pa", t_map), ("pan", t_noise), ("pai", t_ind))}
        for k, t, pl in (("pa", t_map, planes), ("pan", t_noise, planes_n)):
            if stats[k][3]:
                continue
            img, g_, p_, n_ = t.host()
            hit0, hit1 = np.zeros(npx, dtype=np.int64), np.zeros(npx, dtype=np.int64)
            np.add.at(hit0, img * H * W + g_, n_)
            np.add.at(hit1, img * H * W + p_, n_)
            host = pl.cpu().numpy().reshape(4, -1)
            assert np.array_equal(hit0, host[1]) and np.array_equal(hit1, host[3]), f"{name}: the table of ({k}) does not sum to the hit planes"
        for k in ("add", "pm", "padd", "pmn"):
            legs[k]()
        torch.cuda.synchronize()
        if not stats["pa"][3]:
            one = SegmentEvaluator(lp, bins=1, images=B, device=dev).add(pred, lab).host_counts().sum(-1)
            c = pq.cpu().numpy()
            assert np.array_equal(c[..., 0] + c[..., 2], one[:, 0]), f"{name}: TP + FN is not the label side"
            assert pe.overflow() == 0 and np.array_equal(c, pe.counts.cpu().numpy()), f"{name}: the evaluator's counts are not the functional path's"
            tp, fp, fn = (int(c[..., i].sum()) for i in range(3))
            summary = mmsa.panoptic_summary_of(c.sum(0))
        for buf in (pq, pqn):
            buf.zero_()
        pe.reset()
        se.reset()
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
        say(f"{name}: {npx} pixels; every table sums to the hit planes and TP + FN is SegmentEvaluator's label side"
            + ("" if stats["pa"][3] else f"; class map: TP {tp} FP {fp} FN {fn}, PQ {summary['PQ']:.4f} SQ {summary['SQ']:.4f} RQ {summary['RQ']:.4f}"))
        for k, t in (("pa", t_map), ("pan", t_noise), ("pai", t_ind)):
            n, load, walk, lost = stats[k]
            say(f"  table of ({k:3s}): capacity {t.capacity:8d}, {n:8d} pairs, load {load:.4f}, longest walk {walk:4d} slots, overflow {lost}")
        med = {}
        for k in legs:
            t = np.array(times[k])
            med[k] = float(np.median(t))
            say(f"  ({k:4s}) {what[k]:76s} median {med[k]:10.2f}   p10 {np.percentile(t, 10):10.2f}   p90 {np.percentile(t, 90):10.2f}")
        spread = float(np.percentile(times["e"], 90) - np.percentile(times["e"], 10))
        say(f"  (padd) - (add) = {med['padd'] - med['add']:.2f}, (pa) + (pm) = {med['pa'] + med['pm']:.2f}, (padd) / (add) = {med['padd'] / med['add']:.2f} x, "
            f"(pan) / (pa) = {med['pan'] / med['pa']:.2f} x; p10 .. p90 of (e) spans {spread:.2f}")
        del pred, lab, noise, noise2, rp, rl, rpn, rln, rpi, rli, planes, planes_n, t_map, t_noise, t_ind, match, se, pe
        torch.cuda.empty_cache()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
