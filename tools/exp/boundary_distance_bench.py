"""Timing of the Euclidean boundary passes for profiles/boundary_distance.txt.  Legs interleaved in ONE process, every repetition timing each leg once (order
rotated), `--inner` calls per timing between two events on the launch stream, all on the same stored maps:
  (d8) .. (d255)  mmsa_boundary_distance_u8 of the class map at cap 8, 32, 64, 255 (both launches: the row pass and the column pass), into given buffers;
  (a8) (a32)      the full EuclideanBoundaryEvaluator.add() at radius = cap = 8 and 32: two distance maps, the zone counts and the displacement histogram;
  (b8) (b32)      the yardstick: mmsa_eval_boundary_u8 (the Chebyshev band in one launch) at radius 8 and 32 on the same maps;
  (e)             mmsa_eval_confusion_u8 on the same maps: the floor of any pass over them.
And, outside the interleaving (host clock, `--host-reps` runs, one image): what a user has without the distance launch -- the class map copied to the host
and `scipy.ndimage.distance_transform_edt` per class present (where scipy is importable there; else the copy plus the numpy restatement of
tests/boundary_distance_ref.py on a 96 x 96 crop, and the report says so).  The scipy result, squared and capped, must equal the device map at cap 255 pixel
for pixel before anything is timed.
Workloads, 25 classes, as tools/exp/boundary_bench.py: two 1024 x 1024 maps and the 1080 x 1920 frame; the class map is the argmax launch's on seeded
head-resolution logits (smooth blobs, as a model's map: the synthetic stand-in of a seeded model's output), the label map is that map with its contours moved
by (3, 2) pixels, 16 x 16 patches of other classes on 4 % of the blocks and ignored patches on 3 %.  No threshold: the medians and p10 .. p90 spreads are
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

CAPS = (8, 32, 64, 255)
RADII = (8, 32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--inner", type=int, default=3)
    ap.add_argument("--host-reps", type=int, default=2)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("boundary_distance_bench: no GPU (a timing needs one)")
    import mmsa
    import mmsa.inference as inf
    from mmsa.evaluate import DISTANCE_FAR, EuclideanBoundaryEvaluator, LabelPrep
    import torch.nn.functional as F
    try:
        from scipy import ndimage
    except ImportError:
        ndimage = None
    dev = torch.device("cuda", 0)
    lines = []
    C = 25

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    def logits(n, g):
        coarse = torch.randn(n, C, 32, 32, generator=g)
        return (F.interpolate(coarse, size=(256, 256), mode="bilinear") + 0.05 * torch.randn(n, C, 256, 256, generator=g)).to(dev)

    def host_edt(pred_dev):
        """The host alternative on image 0: (seconds of the copy, seconds of the transform, uint16 map at cap 255 or None, what was run)."""
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        m = pred_dev[0].cpu().numpy()
        t1 = time.perf_counter()
        if ndimage is not None:
            d2 = np.full(m.shape, np.iinfo(np.int64).max, dtype=np.int64)
            for c in np.unique(m):
                if (m != c).any():
                    d = ndimage.distance_transform_edt(m == c)
                    d2[m == c] = np.rint(d[m == c] ** 2).astype(np.int64)
            t2 = time.perf_counter()
            return t1 - t0, t2 - t1, np.where(d2 <= 255 * 255, d2, DISTANCE_FAR).astype(np.uint16), "scipy.ndimage.distance_transform_edt per class present"
        from tests import boundary_distance_ref as DR
        DR.d2_map(m[:96, :96], 255)
        t2 = time.perf_counter()
        return t1 - t0, t2 - t1, None, "the numpy restatement on a 96 x 96 crop (scipy is not importable here)"

    say(f"device {torch.cuda.get_device_name(0)}; reps {a.reps}, {a.inner} calls per timing; times in microseconds per call; {C} classes")
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
        npx = B * H * W
        d2 = {c: torch.empty(B, H, W, dtype=torch.uint16, device=dev) for c in CAPS}
        scratch = torch.empty(npx, dtype=torch.uint16, device=dev)
        evs = {d: EuclideanBoundaryEvaluator(lp, d, cap=d, images=B, device=dev) for d in RADII}
        bbuf = {d: torch.zeros(B, 4, C + 1, C + 1, dtype=torch.int64, device=dev) for d in RADII}
        ebuf = torch.zeros(B, C + 1, C + 1, dtype=torch.int64, device=dev)
        legs = dict(e=lambda: mmsa.confusion(pred, lab, lp, counts=ebuf))
        what = dict(e="mmsa_eval_confusion_u8 (the floor)")
        for c in CAPS:
            legs[f"d{c}"] = lambda c=c: mmsa.boundary_distance(pred, c, num_classes=C, scratch=scratch, out=d2[c])
            what[f"d{c}"] = f"mmsa_boundary_distance_u8 of the class map, cap {c}"
        for d in RADII:
            legs[f"a{d}"] = lambda d=d: evs[d].add(pred, lab, slots=list(range(B)))
            what[f"a{d}"] = f"EuclideanBoundaryEvaluator.add(), radius = cap = {d}"
            legs[f"b{d}"] = lambda d=d: mmsa.boundary_counts(pred, lab, lp, d, counts=bbuf[d])
            what[f"b{d}"] = f"mmsa_eval_boundary_u8, radius {d} (the yardstick)"
        for _ in range(2):
            for k in legs:
                legs[k]()
        torch.cuda.synchronize()
        # checks first: the device map against the host transform, the caps against each other, the zone sum against the floor
        copy_s, edt_s, host_map, how = host_edt(pred)
        full = d2[255].cpu().numpy()
        if host_map is not None:
            assert np.array_equal(full[0], host_map), f"{name}: the device map at cap 255 is not the host transform's"
        for c in CAPS[:-1]:
            assert np.array_equal(d2[c].cpu().numpy(), np.where(full <= c * c, full, DISTANCE_FAR)), f"{name}: cap {c} is not cap 255 thresholded"
        conf = mmsa.confusion(pred, lab, lp)
        share = {}
        for d in RADII:
            one = EuclideanBoundaryEvaluator(lp, d, cap=d, images=B, device=dev).add(pred, lab)
            assert torch.equal(one.counts.sum(1), conf), f"{name}: radius {d}: the zone sum is not the confusion matrix"
            share[d] = float(one.counts[:, 2:].sum()) / float(one.counts.sum())
        far = float((full == DISTANCE_FAR).mean())
        host = [host_edt(pred)[:2] for _ in range(a.host_reps)]
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
        say(f"{name}: {npx} pixels; the map at cap 255 equals the host transform on image 0 ({'checked' if host_map is not None else 'NOT checked: no scipy'}), every "
            f"smaller cap equals it thresholded, the zone sums equal (e); share of the counted pixels in the Euclidean label band: "
            + ", ".join(f"radius {d}: {share[d]:.3f}" for d in RADII) + f"; pixels further than 255 from any contour: {far:.3f}")
        med = {}
        for k in legs:
            t = np.array(times[k])
            med[k] = float(np.median(t))
            say(f"  ({k:4s}) {what[k]:58s} median {med[k]:10.2f}   p10 {np.percentile(t, 10):10.2f}   p90 {np.percentile(t, 90):10.2f}")
        spread = float(np.percentile(times["e"], 90) - np.percentile(times["e"], 10))
        say("  " + "; ".join(f"(d{d}) / (b{d}) = {med[f'd{d}'] / med[f'b{d}']:.2f} x, (a{d}) / (b{d}) = {med[f'a{d}'] / med[f'b{d}']:.2f} x" for d in RADII)
            + f"; p10 .. p90 of (e) spans {spread:.2f}")
        say(f"  host alternative, image 0 only ({H} x {W}), {how}: copy {np.median([h[0] for h in host]) * 1e3:.2f} ms, transform "
            f"{np.median([h[1] for h in host]) * 1e3:.1f} ms (host clock, {a.host_reps} runs)")
        del pred, lab, d2, scratch, evs
        torch.cuda.empty_cache()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
