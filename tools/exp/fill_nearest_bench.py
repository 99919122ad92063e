"""Timing of the nearest-label fill for profiles/fill_nearest.txt.  Legs interleaved in ONE process, every repetition timing each leg once (order rotated),
`--inner` calls per timing between two events on the launch stream, all on stored maps and into given buffers (out, d2, scratch):
  (f8) (f32) (f255)     mmsa_fill_nearest_u8 at cap 8 / 32 / 255 of the REALISTIC map: suppress_small(min_area=64, fill=254) of the class map, hole = 254;
  (f8d) (f32d) (f255d)  the same with the d2 output;
  (n32) (n32d)          50 % noise holes: every second pixel of the class map, at random, painted 254; cap 32, without and with d2;
  (w255) (w255d)        the worst case: ONE source pixel in an otherwise all-hole frame at cap 255 (every lane of the column pass walks as far as it can);
  (d8) (d32) (d255)     the yardstick: mmsa_boundary_distance_u8 at the same caps on the same realistic map -- the same two-pass structure;
  (e)                   mmsa_eval_confusion_u8 on the same maps: the floor of any pass over them.
Before anything is timed EVERY device result (out and d2 of the realistic map at the three caps, of the noise map and of the worst case) must equal the numpy
restatement of tests/fill_nearest_ref.py on the full-size map, byte for byte.  Outside the interleaving (host clock, `--host-reps` runs, image 0): what a user
has without the launches -- the map copied to the host and `scipy.ndimage.distance_transform_edt(return_indices=True)` of its hole mask, where scipy imports.
The verdict per cap: the fill's median against the distance launch's, within that launch's own p10 .. p90 spread of the same run.  `--legs` restricts the run
to some legs (a kernel trace of `--legs f32,d32` splits the two launches of each), `--summarise DIR` appends the per-kernel times of such a trace to `--out`.
Workloads, 25 classes, as tools/exp/components_bench.py: two 1024 x 1024 maps and the 1080 x 1920 frame, the class map the argmax launch's on seeded
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

# the grids of the two passes (B * H workgroups; tiles of 64 columns x groups of 4 rows x B) name the workload in a trace
WORKLOADS = {2048: "two 1024 x 1024 maps", 8192: "two 1024 x 1024 maps", 1080: "1080 x 1920 frame", 8100: "1080 x 1920 frame"}


def summarise(trace_dir, out):
    """The kernel-trace CSV(s) under trace_dir -> one line per (kernel, workload) of the fill and distance launches, appended to `out`."""
    rows = {}
    files = sorted(glob.glob(os.path.join(trace_dir, "**", "*kernel_trace.csv"), recursive=True))
    for f in files:
        for r in csv.DictReader(open(f)):
            name = r["Kernel_Name"].split("(")[0]
            if not name.startswith(("fill_", "distance_")):
                continue
            wg, grid = int(r.get("Workgroup_Size_X") or r.get("Workgroup_Size") or 256), int(r.get("Grid_Size_X") or r.get("Grid_Size") or 0)
            rows.setdefault((name, grid // max(wg, 1)), []).append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3)
    if not rows:
        raise SystemExit(f"fill_nearest_bench: no fill or distance launch in the kernel trace under {trace_dir} ({len(files)} files)")
    lines = ["", "kernel trace of a short run of the same program with --legs f32,d32 (the realistic map at cap 32 alone, no d2; no counters), microseconds per "
             "launch: launches, mean, min .. max"]
    for (name, blocks), t in sorted(rows.items()):
        wl = WORKLOADS.get(blocks, f"{blocks} workgroups")
        lines.append(f"  {name:26s} {wl:24s} {len(t):4d} launches   mean {np.mean(t):7.2f}   min {np.min(t):7.2f}   max {np.max(t):7.2f}")
    print("\n".join(lines), flush=True)
    open(out, "a").write("\n".join(lines) + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--inner", type=int, default=3)
    ap.add_argument("--host-reps", type=int, default=2)
    ap.add_argument("--legs", default=None, help="comma-separated legs to time (default: all)")
    ap.add_argument("--no-check", action="store_true", help="skip the comparison with the restatement (the short run under a kernel trace)")
    ap.add_argument("--summarise", default=None, help="a kernel-trace directory: append its per-kernel times to --out and exit")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.summarise:
        if not a.out:
            raise SystemExit("fill_nearest_bench: --summarise appends to --out")
        return summarise(a.summarise, a.out)
    if not torch.cuda.is_available():
        raise SystemExit("fill_nearest_bench: no GPU (a timing needs one)")
    import mmsa
    import mmsa.inference as inf
    from mmsa.evaluate import LabelPrep
    import torch.nn.functional as F
    from tests import fill_nearest_ref as FR
    try:
        from scipy import ndimage
    except ImportError:
        ndimage = None
    dev = torch.device("cuda", 0)
    lines = []
    C, HOLE = 25, 254
    caps = (8, 32, 255)

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    def logits(n, g):
        coarse = torch.randn(n, C, 32, 32, generator=g)
        return (F.interpolate(coarse, size=(256, 256), mode="bilinear") + 0.05 * torch.randn(n, C, 256, 256, generator=g)).to(dev)

    def host_route(map_dev):
        """The host alternative on image 0: (seconds of the copy, seconds of the transform and the gather)."""
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        m = map_dev[0].cpu().numpy()
        t1 = time.perf_counter()
        hole = m == HOLE
        dist, (iy, ix) = ndimage.distance_transform_edt(hole, return_indices=True)
        filled = np.where(hole & (dist <= 32), m[iy, ix], m)
        return t1 - t0, time.perf_counter() - t1, filled

    say(f"device {torch.cuda.get_device_name(0)}; reps {a.reps}, {a.inner} calls per timing; times in microseconds per call; {C} classes; hole byte {HOLE}")
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
        noise = torch.where(torch.rand(B, H, W, generator=g).to(dev) < 0.5, torch.full_like(pred, HOLE), pred)
        worst = torch.full_like(pred, HOLE)
        worst[:, H // 2, W // 2] = 3
        npx = B * H * W
        out = torch.empty_like(pred)
        d2, scratch = torch.empty(B, H, W, dtype=torch.uint16, device=dev), torch.empty(npx, dtype=torch.uint16, device=dev)
        ebuf = torch.zeros(B, C + 1, C + 1, dtype=torch.int64, device=dev)

        def fill(m, cap, with_d2):
            return lambda: mmsa.fill_nearest(m, hole=HOLE, cap=cap, out=out, d2=d2 if with_d2 else None, scratch=scratch)

        legs, what = {}, {}
        for c in caps:
            for tag, with_d2 in (("", False), ("d", True)):
                legs[f"f{c}{tag}"] = fill(real, c, with_d2)
                what[f"f{c}{tag}"] = f"mmsa_fill_nearest_u8 of the realistic map, cap {c}" + (", with d2" if with_d2 else "")
        for tag, with_d2 in (("", False), ("d", True)):
            legs[f"n32{tag}"], what[f"n32{tag}"] = fill(noise, 32, with_d2), "mmsa_fill_nearest_u8, 50 % noise holes, cap 32" + (", with d2" if with_d2 else "")
            legs[f"w255{tag}"] = fill(worst, 255, with_d2)
            what[f"w255{tag}"] = "mmsa_fill_nearest_u8, one source in an all-hole frame, cap 255" + (", with d2" if with_d2 else "")
        for c in caps:
            legs[f"d{c}"] = lambda c=c: mmsa.boundary_distance(real, c, num_classes=C, scratch=scratch, out=d2)
            what[f"d{c}"] = f"mmsa_boundary_distance_u8 of the realistic map, cap {c} (the yardstick)"
        legs["e"], what["e"] = (lambda: mmsa.confusion(pred, lab, lp, counts=ebuf)), "mmsa_eval_confusion_u8 (the floor)"
        if a.legs:
            legs = {k: legs[k] for k in a.legs.split(",")}
        for _ in range(2):
            for k in legs:
                legs[k]()
        torch.cuda.synchronize()
        # checks first: every device result against the restatement on the full-size map
        checked = "not compared with the restatement in this run (--no-check)"
        if not a.no_check:
            n_checked = 0
            for tag, m, cs in (("realistic", real, caps), ("noise", noise, (32,)), ("worst", worst, (255,))):
                host = m.cpu().numpy()
                for c in cs:
                    want = FR.fill_batch(host, HOLE, (), c)
                    out.fill_(0xA5)
                    fill(m, c, True)()
                    assert np.array_equal(out.cpu().numpy(), want[0]) and np.array_equal(d2.cpu().numpy(), want[1]), f"{name}: {tag} map at cap {c}: not the restatement's"
                    got = mmsa.fill_nearest(m, hole=HOLE, cap=c, scratch=scratch)
                    assert np.array_equal(got.cpu().numpy(), want[0]), f"{name}: {tag} map at cap {c} without d2: not the restatement's"
                    n_checked += 1
                    if tag == "realistic" and c == 32:
                        holes, left = int((host == HOLE).sum()), int((want[0] == HOLE).sum())
            checked = f"out and d2 of all {n_checked} (map, cap) pairs equal the numpy restatement on the full-size map byte for byte"
        else:
            host = real.cpu().numpy()
            holes, left = int((host == HOLE).sum()), -1
        host_t = None
        if ndimage is not None and not a.legs:
            host_t = [host_route(real)[:2] for _ in range(a.host_reps)]
            ref = FR.fill(real[0].cpu().numpy(), HOLE, (), 32)
            filled = host_route(real)[2]
            agree = float((filled == ref[0]).mean())                       # scipy breaks ties its own way: a share, not an assertion
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
        say(f"{name}: {npx} pixels; {checked}; the realistic map has {holes} holes ({holes / npx:.4f} of the pixels), {left} of them stay at cap 32")
        med, p10, p90 = {}, {}, {}
        for k in legs:
            t = np.array(times[k])
            med[k], p10[k], p90[k] = float(np.median(t)), float(np.percentile(t, 10)), float(np.percentile(t, 90))
            say(f"  ({k:5s}) {what[k]:72s} median {med[k]:10.2f}   p10 {p10[k]:10.2f}   p90 {p90[k]:10.2f}")
        for c in caps:
            if f"f{c}" in med and f"d{c}" in med:
                f, d, spread = med[f"f{c}"], med[f"d{c}"], p90[f"d{c}"] - p10[f"d{c}"]
                verdict = "no slower than the distance launch" if f <= d + spread else "SLOWER than the distance launch by more than its spread"
                say(f"  cap {c}: (f{c}) / (d{c}) = {f / d:.2f} x ({f:.2f} against {d:.2f}, the distance launch's p10 .. p90 spans {spread:.2f}): the fill is {verdict}; "
                    + (f"the d2 output costs {med[f'f{c}d'] - f:+.2f}" if f"f{c}d" in med else "the d2 output was not timed in this run"))
        if "n32" in med and "w255" in med and "e" in med:
            say(f"  (n32) / (f32) = {med['n32'] / med['f32']:.2f} x, (w255) / (f255) = {med['w255'] / med['f255']:.2f} x, (f32) / (e) = {med['f32'] / med['e']:.2f} x")
        if host_t:
            say(f"  host route, image 0 only ({H} x {W}): copy {np.median([h[0] for h in host_t]) * 1e3:.2f} ms, scipy.ndimage.distance_transform_edt(return_indices="
                f"True) and the gather {np.median([h[1] for h in host_t]) * 1e3:.1f} ms (host clock, {a.host_reps} runs); {agree:.6f} of its pixels equal the "
                "device map at cap 32 (the rest are ties that scipy breaks its own way)")
        elif not a.legs:
            say("  host route: scipy is not importable here; not measured")
        del pred, lab, real, noise, worst, out, d2, scratch
        torch.cuda.empty_cache()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
