"""Timing of the majority filter for profiles/majority_filter.txt.  Legs interleaved in ONE process, every repetition timing each leg once (order rotated),
`--inner` calls per timing between two events on the launch stream, all on stored maps and into given buffers (out, support):
  (m1) (m2) (m3) (m8) (m16) (m32)   mmsa_majority_filter_u8 of the class map at radius 1 / 2 / 3 / 8 / 16 / 32, where="all", num_classes=25;
  (m1s) ... (m32s)            the same with the support output;
  (h3) (f32)                  where="holes" at radius 3 on the REALISTIC map with holes, suppress_small(min_area=64, fill=254) of the class map, and
                              mmsa_fill_nearest_u8 at cap 32 on the same map: the two ways to close a hole;
  (w25) (w25x) (w200)         the worst cases: 25-value noise at radius 2 and at radius 32, 200-value noise (num_classes=None) at radius 2;
  (b1) (b2) (b3) (b8) (b16) (b32)   the yardstick: mmsa_eval_boundary_u8 at the same radii, the existing window stencil over the same staged tiles;
  (e)                         mmsa_eval_confusion_u8 on the same maps: the floor of any pass over them.
Before anything is timed EVERY device result (out and support of every (map, radius, target) above) must equal the numpy restatement of tests/majority_ref.py
on the full-size map, byte for byte.  Outside the interleaving: the device alternative in torch at radius 2 (one-hot canvas -> avg_pool2d(divisor_override=1) ->
argmax; events, `--torch-reps` runs; its map must equal the filter's wherever the window holds no tie, and the share of equal pixels is reported), and the host
route on image 0 (host clock): the copy, per-class `scipy.ndimage.uniform_filter` counts with an argmax, and `scipy.ndimage.generic_filter` with a mode on a
128 x 128 crop, where scipy imports.  Every leg is reported as a ratio to the boundary pass at equal radius and to the floor with the yardstick's own
p10 .. p90 spread next to it.  `--legs` restricts the run to some legs, `--summarise DIR` appends the per-kernel times of a kernel trace to `--out`.
Workloads, 25 classes, as tools/exp/fill_nearest_bench.py: two 1024 x 1024 maps and the 1080 x 1920 frame, the class map the argmax launch's on seeded
head-resolution logits.  No threshold: the medians and p10 .. p90 spreads are the record."""
import argparse
import csv
import glob
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "multimodal-sam-adapter_amd"))
sys.path.insert(0, ROOT)

RADII = (1, 2, 3, 8, 16, 32)


def summarise(trace_dir, out):
    """The kernel-trace CSV(s) under trace_dir -> one line per (kernel, grid) of the majority and boundary launches, appended to `out`."""
    rows = {}
    files = sorted(glob.glob(os.path.join(trace_dir, "**", "*kernel_trace.csv"), recursive=True))
    for f in files:
        for r in csv.DictReader(open(f)):
            name = r["Kernel_Name"].split("(")[0].replace("void ", "")
            if not name.startswith(("majority_", "eval_boundary_")):
                continue
            wg, grid = int(r.get("Workgroup_Size_X") or r.get("Workgroup_Size") or 256), int(r.get("Grid_Size_X") or r.get("Grid_Size") or 0)
            rows.setdefault((name, grid // max(wg, 1)), []).append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3)
    if not rows:
        raise SystemExit(f"majority_filter_bench: no majority or boundary launch in the kernel trace under {trace_dir} ({len(files)} files)")
    lines = ["", "kernel trace of a short run of the same program with --legs m2,b2,m32,b32 (no counters), microseconds per launch: launches, mean, min .. max"]
    for (name, blocks), t in sorted(rows.items()):
        lines.append(f"  {name:28s} {blocks:6d} workgroups {len(t):4d} launches   mean {np.mean(t):8.2f}   min {np.min(t):8.2f}   max {np.max(t):8.2f}")
    print("\n".join(lines), flush=True)
    open(out, "a").write("\n".join(lines) + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--inner", type=int, default=3)
    ap.add_argument("--torch-reps", type=int, default=5)
    ap.add_argument("--legs", default=None, help="comma-separated legs to time (default: all)")
    ap.add_argument("--no-check", action="store_true", help="skip the comparison with the restatement (the short run under a kernel trace)")
    ap.add_argument("--summarise", default=None, help="a kernel-trace directory: append its per-kernel times to --out and exit")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.summarise:
        if not a.out:
            raise SystemExit("majority_filter_bench: --summarise appends to --out")
        return summarise(a.summarise, a.out)
    if not torch.cuda.is_available():
        raise SystemExit("majority_filter_bench: no GPU (a timing needs one)")
    import mmsa
    import mmsa.inference as inf
    from mmsa.evaluate import LabelPrep
    import torch.nn.functional as F
    from tests import majority_ref as MR
    try:
        from scipy import ndimage
    except ImportError:
        ndimage = None
    dev = torch.device("cuda", 0)
    lines = []
    C, HOLE = 25, 254

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    def logits(n, g):
        coarse = torch.randn(n, C, 32, 32, generator=g)
        return (F.interpolate(coarse, size=(256, 256), mode="bilinear") + 0.05 * torch.randn(n, C, 256, 256, generator=g)).to(dev)

    def torch_route(m, r):
        """One-hot canvas -> box sums -> argmax: the mode filter of a map whose every byte is a class, ties to the smallest class."""
        onehot = F.one_hot(m.long(), C).permute(0, 3, 1, 2).float()
        return F.avg_pool2d(onehot, 2 * r + 1, stride=1, padding=r, divisor_override=1).argmax(dim=1).to(torch.uint8)

    say(f"device {torch.cuda.get_device_name(0)}; reps {a.reps}, {a.inner} calls per timing; times in microseconds per call; {C} classes; hole byte {HOLE}")
    say("ONE kernel form is built: per value present in a tile, rows as ballot masks, popcounts, a sliding column sum.  The per-lane LDS histogram column is not "
        "built.  Tiles of 64 columns x 16 rows up to radius 8, x 32 up to radius 16, x 64 above (MMSA_MAJ_TH of a debug-knob build overrides the height).")
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
        lab = torch.roll(pred, (3, 2), (1, 2)).contiguous()
        real = mmsa.suppress_small(pred, 64, num_classes=C, fill=HOLE)
        noise25 = torch.randint(0, C, (B, H, W), generator=g, dtype=torch.uint8).to(dev)
        noise200 = torch.randint(0, 200, (B, H, W), generator=g, dtype=torch.uint8).to(dev)
        npx = B * H * W
        out = torch.empty_like(pred)
        support, scratch = torch.empty(B, H, W, dtype=torch.uint16, device=dev), torch.empty(npx, dtype=torch.uint16, device=dev)
        ebuf = torch.zeros(B, C + 1, C + 1, dtype=torch.int64, device=dev)
        bbuf = torch.zeros(B, 4, C + 1, C + 1, dtype=torch.int64, device=dev)

        # leg -> (map, radius, keywords of majority_filter)
        spec = {}
        for r in RADII:
            spec[f"m{r}"] = (pred, r, dict(num_classes=C))
        spec["h3"] = (real, 3, dict(num_classes=C, hole=HOLE, where="holes"))
        spec["w25"], spec["w25x"], spec["w200"] = (noise25, 2, dict(num_classes=C)), (noise25, 32, dict(num_classes=C)), (noise200, 2, dict())
        what = {f"m{r}": f"mmsa_majority_filter_u8 of the class map, radius {r}" for r in RADII}
        what.update(h3="mmsa_majority_filter_u8, the holes of the realistic map alone, radius 3", w25="mmsa_majority_filter_u8, 25-value noise, radius 2",
                    w25x="mmsa_majority_filter_u8, 25-value noise, radius 32", w200="mmsa_majority_filter_u8, 200-value noise, radius 2")

        def filt(k, with_support):
            m, r, kw = spec[k]
            return lambda: mmsa.majority_filter(m, r, out=out, support=support if with_support else None, **kw)

        legs = {}
        for r in RADII:
            legs[f"m{r}"], legs[f"m{r}s"] = filt(f"m{r}", False), filt(f"m{r}", True)
            what[f"m{r}s"] = what[f"m{r}"] + ", with support"
        legs["h3"] = filt("h3", False)
        legs["f32"], what["f32"] = (lambda: mmsa.fill_nearest(real, hole=HOLE, cap=32, out=out, scratch=scratch)), "mmsa_fill_nearest_u8 of the realistic map, cap 32"
        for k in ("w25", "w25x", "w200"):
            legs[k] = filt(k, False)
        for r in RADII:
            legs[f"b{r}"] = lambda r=r: mmsa.boundary_counts(pred, lab, lp, r, counts=bbuf)
            what[f"b{r}"] = f"mmsa_eval_boundary_u8 of the class map, radius {r} (the yardstick)"
        legs["e"], what["e"] = (lambda: mmsa.confusion(pred, lab, lp, counts=ebuf)), "mmsa_eval_confusion_u8 (the floor)"
        if a.legs:
            legs = {k: legs[k] for k in a.legs.split(",")}
        for _ in range(2):
            for k in legs:
                legs[k]()
        torch.cuda.synchronize()

        # checks first: every device result against the restatement on the full-size map
        checked = "not compared with the restatement in this run (--no-check)"
        changed = {}
        votes2 = None
        if not a.no_check:
            n_checked = 0
            for k, (m, r, kw) in spec.items():
                if a.legs and k not in legs:
                    continue
                host = m.cpu().numpy()
                role = MR.roles(kw.get("num_classes"), kw.get("hole", ()), ())
                vts = [MR.votes(one, role, r) for one in host]
                if k == "m2":
                    votes2 = vts
                for half in (False, True):
                    res = [MR.apply(one, role, vt, kw.get("where", "all") == "all", half) for one, vt in zip(host, vts)]
                    out.fill_(0xA5)
                    mmsa.majority_filter(m, r, half=half, out=out, support=support, **kw)
                    assert np.array_equal(out.cpu().numpy(), np.stack([o for o, _ in res])), f"{name}: ({k}) half={half}: out is not the restatement's"
                    assert np.array_equal(support.cpu().numpy(), np.stack([s for _, s in res])), f"{name}: ({k}) half={half}: support is not the restatement's"
                    n_checked += 1
                    if not half:
                        changed[k] = int((np.stack([o for o, _ in res]) != host).sum())
            checked = f"out and support of all {n_checked} (map, radius, target, half) combinations equal the numpy restatement on the full-size map byte for byte"

        # the alternatives a user has, outside the interleaving
        alt = []
        if not a.legs:
            tt = []
            for _ in range(a.torch_reps + 1):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                tmap = torch_route(pred, 2)
                e1.record()
                e1.synchronize()
                tt.append(e0.elapsed_time(e1) * 1e3)
            ours = mmsa.majority_filter(pred, 2, num_classes=C)
            share = float((tmap == ours).float().mean().item())
            line = (f"  device torch at radius 2 (one-hot float canvas [B, {C}, H, W] = {npx * C * 4 / 1e6:.0f} MB -> avg_pool2d(divisor_override=1) -> argmax): "
                    f"median {np.median(tt[1:]):.1f} (events, {a.torch_reps} runs after one warm-up); {share:.6f} of its pixels equal the filter's")
            if votes2 is not None:
                untied = torch.from_numpy(np.stack([vt.tied for vt in votes2]) == 1).to(dev)
                assert torch.equal(tmap[untied], ours[untied]), f"{name}: the torch route differs from the filter where the window holds no tie"
                line += f", and all {int(untied.sum().item())} pixels whose window holds no tie (the rest: torch gives a tie to the smallest class, also against the own value)"
            alt.append(line)
            del tmap
            torch.cuda.empty_cache()
            if ndimage is not None:
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                m0 = pred[0].cpu().numpy()
                t1 = time.perf_counter()
                counts = np.stack([ndimage.uniform_filter((m0 == v).astype(np.float32), 5, mode="constant") for v in range(C)])
                hmap = counts.argmax(axis=0).astype(np.uint8)
                t2 = time.perf_counter()
                crop = m0[:128, :128]
                ndimage.generic_filter(crop, lambda w: np.bincount(w.astype(np.int64)).argmax(), size=5, mode="constant", cval=255)
                t3 = time.perf_counter()
                alt.append(f"  host route, image 0 only ({H} x {W}), radius 2, host clock, one run: copy {(t1 - t0) * 1e3:.2f} ms; {C} x scipy.ndimage.uniform_filter + "
                           f"argmax {(t2 - t1) * 1e3:.0f} ms ({float((hmap == ours[0].cpu().numpy()).mean()):.6f} of its pixels equal the filter's: float counts, ties to "
                           f"the smallest class); scipy.ndimage.generic_filter with a bincount mode on a 128 x 128 crop {(t3 - t2) * 1e3:.0f} ms = "
                           f"{(t3 - t2) / (128 * 128) * H * W:.1f} s per image at that rate")
            else:
                alt.append("  host route: scipy is not importable here; not measured")

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
        holes = int((real == HOLE).sum().item())
        say(f"{name}: {npx} pixels; {checked}; the realistic map has {holes} holes ({holes / npx:.4f} of the pixels); pixels changed: "
            + (", ".join(f"({k}) {v}" for k, v in changed.items()) or "not counted"))
        med, p10, p90 = {}, {}, {}
        for k in legs:
            t = np.array(times[k])
            med[k], p10[k], p90[k] = float(np.median(t)), float(np.percentile(t, 10)), float(np.percentile(t, 90))
            say(f"  ({k:5s}) {what[k]:76s} median {med[k]:10.2f}   p10 {p10[k]:10.2f}   p90 {p90[k]:10.2f}")

        def against(k, r):
            """Leg k as a ratio to the boundary pass at radius r and to the floor, and whether the difference to the yardstick lies inside its spread."""
            s = f"  ({k}) = {med[k]:.2f}"
            if f"b{r}" in med:
                b, spread = med[f"b{r}"], p90[f"b{r}"] - p10[f"b{r}"]
                inside = "inside" if abs(med[k] - b) <= spread else "beyond"
                s += f": {med[k] / b:.2f} x (b{r}) = {b:.2f} (its p10 .. p90 spans {spread:.2f}; the difference of {med[k] - b:+.2f} lies {inside} that spread)"
            if "e" in med:
                s += f"; {med[k] / med['e']:.2f} x the floor (e) = {med['e']:.2f} (spans {p90['e'] - p10['e']:.2f})"
            return s

        for r in RADII:
            if f"m{r}" in med:
                say(against(f"m{r}", r) + (f"; the support output costs {med[f'm{r}s'] - med[f'm{r}']:+.2f}" if f"m{r}s" in med else ""))
        for k, r in (("h3", 3), ("w25", 2), ("w25x", 32), ("w200", 2)):
            if k in med:
                say(against(k, r))
        if "h3" in med and "f32" in med:
            spread = p90["f32"] - p10["f32"]
            say(f"  closing the holes: (h3) / (f32) = {med['h3'] / med['f32']:.2f} x ({med['h3']:.2f} against {med['f32']:.2f}; the fill's p10 .. p90 spans {spread:.2f}, "
                f"the difference lies {'inside' if abs(med['h3'] - med['f32']) <= spread else 'beyond'} it)")
        for line in alt:
            say(line)
        del pred, lab, real, noise25, noise200, out, support, scratch
        torch.cuda.empty_cache()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
