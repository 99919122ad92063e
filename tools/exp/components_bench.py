"""Timing of the segment passes for profiles/components.txt.  Legs interleaved in ONE process, every repetition timing each leg once (order rotated),
`--inner` calls per timing between two events on the launch stream, all on the same stored maps and into given buffers:
  (c8) (c4)   mmsa_components_u8 of the class map at connectivity 8 and 4 (tile pass, merge pass, flatten pass);
  (cl)        mmsa_components_u8 of the label map (through the label LUT), connectivity 8;
  (ar)        mmsa_component_area of the class map's roots (memset + one launch);
  (su)        mmsa.suppress_small(min_area=64) into given root / area / out buffers: (c8) + (ar) + the pointwise launch;
  (add)       the full SegmentEvaluator.add(): two component calls and mmsa_eval_segments (memset + two launches);
  (cn) (an)   the worst case of the per-wave reduction, a 25-class NOISE map of the same size: components, and areas with 64 distinct roots in most waves;
  (d32)       the yardstick: mmsa_boundary_distance_u8 at cap 32 on the same class map, the existing two-launch primitive of the same kind;
  (e)         mmsa_eval_confusion_u8 on the same maps: the floor of any pass over them.
And, outside the interleaving (host clock, `--host-reps` runs, one image): what a user has without the component launches -- the class map copied to the host
and `scipy.ndimage.label` per class present (where scipy is importable there; else the copy plus the numpy restatement of tests/components_ref.py, and the
report says so).  The host labels, relabelled to the smallest linear index of each component, must equal the device roots pixel for pixel before anything is
timed.  Which of the three component launches holds the time is read from a kernel trace of a run of this program (the report of profiles/components.txt).
Workloads, 25 classes, as tools/exp/boundary_distance_bench.py: two 1024 x 1024 maps and the 1080 x 1920 frame; the class map is the argmax launch's on
seeded head-resolution logits (smooth blobs, as a model's map), the label map is that map with its contours moved by (3, 2) pixels, 16 x 16 patches of other
classes on 4 % of the blocks and ignored patches on 3 %.  No threshold: the medians and p10 .. p90 spreads are the record."""
import argparse
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "multimodal-sam-adapter_amd"))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--inner", type=int, default=3)
    ap.add_argument("--host-reps", type=int, default=2)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("components_bench: no GPU (a timing needs one)")
    import mmsa
    import mmsa.inference as inf
    from mmsa.evaluate import LabelPrep, SegmentEvaluator
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

    def host_label(pred_dev):
        """The host alternative on image 0: (seconds of the copy, seconds of the labelling, int64 roots [H, W], what was run)."""
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        m = pred_dev[0].cpu().numpy()
        t1 = time.perf_counter()
        if ndimage is None:
            from tests import components_ref as CR
            r = CR.roots(m, 8).astype(np.int64)
            return t1 - t0, time.perf_counter() - t1, r, "the numpy restatement of tests/components_ref.py (scipy is not importable here)"
        labs = [ndimage.label(m == c, structure=np.ones((3, 3))) for c in np.unique(m)]
        t2 = time.perf_counter()                                             # the labelling alone is what a user pays; the relabelling below is the check's
        idx = np.arange(m.size, dtype=np.int64).reshape(m.shape)
        r = np.full(m.shape, -1, dtype=np.int64)
        for lab, n in labs:
            low = np.asarray(ndimage.minimum(idx, lab, index=np.arange(1, n + 1))).astype(np.int64)
            r[lab > 0] = low[lab[lab > 0] - 1]
        return t1 - t0, t2 - t1, r, "scipy.ndimage.label per class present"

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
        noise = torch.randint(0, C, (B, H, W), generator=g, dtype=torch.uint8).to(dev)
        npx = B * H * W

        def plane():
            return torch.empty(B, H, W, dtype=torch.int32, device=dev)

        roots = {k: plane() for k in ("c8", "c4", "cl", "cn", "su")}
        area, area_n, area_su = plane(), plane(), plane()
        out = torch.empty_like(pred)
        d2, scratch = torch.empty(B, H, W, dtype=torch.uint16, device=dev), torch.empty(npx, dtype=torch.uint16, device=dev)
        se = SegmentEvaluator(lp, images=B, device=dev)
        ebuf = torch.zeros(B, C + 1, C + 1, dtype=torch.int64, device=dev)
        legs = dict(
            c8=lambda: mmsa.components(pred, num_classes=C, connectivity=8, out=roots["c8"]),
            c4=lambda: mmsa.components(pred, num_classes=C, connectivity=4, out=roots["c4"]),
            cl=lambda: mmsa.components(lab, labels_prep=lp, connectivity=8, out=roots["cl"]),
            ar=lambda: mmsa.component_areas(roots["c8"], out=area),
            su=lambda: mmsa.suppress_small(pred, 64, num_classes=C, out=out, root=roots["su"], area=area_su),
            add=lambda: se.add(pred, lab, slots=list(range(B))),
            cn=lambda: mmsa.components(noise, num_classes=C, connectivity=8, out=roots["cn"]),
            an=lambda: mmsa.component_areas(roots["cn"], out=area_n),
            d32=lambda: mmsa.boundary_distance(pred, 32, num_classes=C, scratch=scratch, out=d2),
            e=lambda: mmsa.confusion(pred, lab, lp, counts=ebuf))
        what = dict(c8="mmsa_components_u8 of the class map, connectivity 8", c4="mmsa_components_u8 of the class map, connectivity 4",
                    cl="mmsa_components_u8 of the label map, connectivity 8", ar="mmsa_component_area of the class map's roots",
                    su="suppress_small(min_area=64): components + areas + pointwise", add="SegmentEvaluator.add(): 2 x components + mmsa_eval_segments",
                    cn="mmsa_components_u8 of a 25-class noise map", an="mmsa_component_area of the noise map's roots (64 roots per wave)",
                    d32="mmsa_boundary_distance_u8, cap 32 (the yardstick)", e="mmsa_eval_confusion_u8 (the floor)")
        for _ in range(2):
            for k in legs:
                legs[k]()
        torch.cuda.synchronize()
        # checks first: the device roots against the host labelling, the areas against the roots
        copy_s, label_s, host_roots, how = host_label(pred)
        got = roots["c8"].cpu().numpy()
        assert np.array_equal(got[0], host_roots), f"{name}: the device roots are not the host labelling's"
        ar = area.cpu().numpy()
        assert all(int(ar[b].sum()) == H * W for b in range(B)) and np.array_equal(ar != 0, got == np.arange(H * W).reshape(1, H, W)), f"{name}: the areas"
        nseg = [int((roots[k].cpu().numpy() == np.arange(H * W).reshape(1, H, W)).sum()) for k in ("c8", "c4", "cl", "cn")]
        kept = float((out == pred).float().mean())
        host = [host_label(pred)[:2] for _ in range(a.host_reps)]
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
        say(f"{name}: {npx} pixels; the roots at connectivity 8 equal the host labelling on image 0 ({how}), the areas sum to H * W per image and are non-zero "
            f"exactly at the roots; components: class map {nseg[0]} at 8 / {nseg[1]} at 4, label map {nseg[2]}, noise map {nseg[3]}; suppress_small(64) keeps "
            f"{kept:.4f} of the pixels")
        med = {}
        for k in legs:
            t = np.array(times[k])
            med[k] = float(np.median(t))
            say(f"  ({k:4s}) {what[k]:64s} median {med[k]:10.2f}   p10 {np.percentile(t, 10):10.2f}   p90 {np.percentile(t, 90):10.2f}")
        spread = float(np.percentile(times["e"], 90) - np.percentile(times["e"], 10))
        say(f"  (c8) / (d32) = {med['c8'] / med['d32']:.2f} x, (add) / (d32) = {med['add'] / med['d32']:.2f} x, (cn) / (c8) = {med['cn'] / med['c8']:.2f} x, "
            f"(an) / (ar) = {med['an'] / med['ar']:.2f} x; p10 .. p90 of (e) spans {spread:.2f}")
        say(f"  host alternative, image 0 only ({H} x {W}), {how}: copy {np.median([h[0] for h in host]) * 1e3:.2f} ms, labelling "
            f"{np.median([h[1] for h in host]) * 1e3:.1f} ms (host clock, {a.host_reps} runs)")
        del pred, lab, noise, roots, area, area_n, area_su, out, d2, scratch, se
        torch.cuda.empty_cache()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
