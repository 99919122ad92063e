"""Timing of the guided vote filter for profiles/vote_filter.txt.  Legs interleaved in ONE process, every repetition timing each leg once (order rotated),
`--inner` calls per timing between two events on the launch stream, all on stored maps and into given buffers (out, support):
  (g1) (g2) (g4) (g8) (g16)   mmsa_vote_filter_u8 of the class map at radius 1 / 2 / 4 / 8 / 16 with the 3-channel frame as guide, sigma = 8, num_classes=25;
  (a2) (a8)                   the same with a 1-channel guide (channel 0 of the frame);
  (w2) (w8)                   no guide, the confidence map as weights;
  (gw2) (gw8)                 the 3-channel guide and the weights;
  (h2) (h8)                   where="holes" with the 3-channel guide on the REALISTIC map with holes, suppress_small(min_area=64, fill=254) of the class map;
  (n25) (n25x) (n200) (n200x) the worst cases with the 3-channel guide: 25-value noise at radius 2 and 16, 200-value noise (num_classes=None) at radius 2 and 16;
  (m1) (m2) (m4) (m8) (m16)   the yardstick: mmsa_majority_filter_u8 of the class map at the same radii, the floor of this family;
  (e)                         mmsa_eval_confusion_u8 on the same maps: the floor of any pass over them.
Before anything is timed EVERY device result (out and support of every vote leg above, with and without the half rule) must equal the numpy restatement of
tests/vote_filter_ref.py on the full-size map, byte for byte; the restatements are computed by worker processes that never touch the GPU.  Outside the
interleaving: the device composition in torch a user had (one-hot float canvas -> unfold of it and of the guide -> table look-up -> weighted sum -> argmax;
events, `--torch-reps` runs) at the radii where its unfolded canvas stays below `--torch-gb`, with the share of pixels equal to the filter's; the other radii
are named with the bytes they would need.  Every vote leg is reported as a ratio to the majority filter at equal radius with the yardstick's own p10 .. p90
span next to it.  `--legs` restricts the run to some legs, `--summarise DIR` appends the per-kernel times of a kernel trace to `--out`.
The class map and the confidence are the argmax launch's on seeded head-resolution logits, as tools/exp/majority_filter_bench.py; the frame is a colour per
class of the map displaced by (3, 2) pixels plus noise of -6 .. 6 per channel, so that its edges lie NEAR the map's contours and not on them.  Workloads, 25
classes: two 1024 x 1024 maps and the 1080 x 1920 frame.  No threshold: the medians and p10 .. p90 spans are the record."""
import argparse
import csv
import glob
import multiprocessing
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "multimodal-sam-adapter_amd"))
sys.path.insert(0, ROOT)

RADII = (1, 2, 4, 8, 16)
SIGMA = 8.0


def restate(m, role, r, all_, guide, lut, wq):
    """One image in a worker process (numpy only) -> ((out, support) without the half rule, (out, support) with it)."""
    from tests import vote_filter_ref as VR
    vt = VR.sums(m, role, r, guide, lut, wq)
    return VR.apply(m, role, vt, all_, False), VR.apply(m, role, vt, all_, True)


def summarise(trace_dir, out):
    """The kernel-trace CSV(s) under trace_dir -> one line per (kernel, grid) of the vote and majority launches, appended to `out`."""
    rows = {}
    files = sorted(glob.glob(os.path.join(trace_dir, "**", "*kernel_trace.csv"), recursive=True))
    for f in files:
        for r in csv.DictReader(open(f)):
            name = r["Kernel_Name"].split("(")[0].replace("void ", "")
            if not name.startswith(("vote_", "majority_")):
                continue
            wg, grid = int(r.get("Workgroup_Size_X") or r.get("Workgroup_Size") or 256), int(r.get("Grid_Size_X") or r.get("Grid_Size") or 0)
            rows.setdefault((name, grid // max(wg, 1)), []).append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3)
    if not rows:
        raise SystemExit(f"vote_filter_bench: no vote or majority launch in the kernel trace under {trace_dir} ({len(files)} files)")
    lines = ["", "kernel trace of a short run of the same program with --legs g2,m2,g8,m8 (no counters), microseconds per launch: launches, mean, min .. max"]
    for (name, blocks), t in sorted(rows.items()):
        lines.append(f"  {name:28s} {blocks:6d} workgroups {len(t):4d} launches   mean {np.mean(t):9.2f}   min {np.min(t):9.2f}   max {np.max(t):9.2f}")
    print("\n".join(lines), flush=True)
    open(out, "a").write("\n".join(lines) + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--inner", type=int, default=2)
    ap.add_argument("--torch-reps", type=int, default=3)
    ap.add_argument("--torch-gb", type=float, default=24.0, help="the largest unfolded one-hot canvas the torch composition is run with")
    ap.add_argument("--workers", type=int, default=12, help="processes that compute the restatements")
    ap.add_argument("--legs", default=None, help="comma-separated legs to time (default: all)")
    ap.add_argument("--no-check", action="store_true", help="skip the comparison with the restatement (the short run under a kernel trace, the tile-height runs)")
    ap.add_argument("--summarise", default=None, help="a kernel-trace directory: append its per-kernel times to --out and exit")
    ap.add_argument("--note", default=None, help="a line to put under the header (which build, which knob)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.summarise:
        if not a.out:
            raise SystemExit("vote_filter_bench: --summarise appends to --out")
        return summarise(a.summarise, a.out)
    # the workers start before this process opens the GPU, and never open it themselves
    pool = None if a.no_check else multiprocessing.get_context("spawn").Pool(a.workers)
    try:
        run(a, pool)
    finally:
        if pool is not None:
            pool.terminate()
            pool.join()


def run(a, pool):
    import torch
    import torch.nn.functional as F
    if not torch.cuda.is_available():
        raise SystemExit("vote_filter_bench: no GPU (a timing needs one)")
    import mmsa
    import mmsa.inference as inf
    from mmsa.evaluate import LabelPrep
    from tests import majority_ref as MR
    from tests import vote_filter_ref as VR
    dev = torch.device("cuda", 0)
    lines = []
    C, HOLE = 25, 254

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    def logits(n, g):
        coarse = torch.randn(n, C, 32, 32, generator=g)
        return (F.interpolate(coarse, size=(256, 256), mode="bilinear") + 0.05 * torch.randn(n, C, 256, 256, generator=g)).to(dev)

    def torch_route(m, guide, r, lut_t):
        """What a user had: one-hot canvas, unfold of it and of the guide, the table, a weighted sum, argmax (ties to the smallest class, also against the own)."""
        k = 2 * r + 1
        B, H, W = m.shape
        onehot = F.one_hot(m.long(), C).permute(0, 3, 1, 2).float()
        uo = F.unfold(onehot, k, padding=r).view(B, C, k * k, H * W)
        g = guide.permute(0, 3, 1, 2).float()
        ug = F.unfold(g, k, padding=r).view(B, 3, k * k, H * W)
        d = (ug - g.reshape(B, 3, 1, H * W)).abs().sum(1).long()
        votes = (uo * lut_t[d].unsqueeze(1)).sum(2)
        return votes.argmax(1).view(B, H, W).to(torch.uint8)

    say(f"device {torch.cuda.get_device_name(0)}; reps {a.reps}, {a.inner} calls per timing; times in microseconds per call; {C} classes; hole byte {HOLE}; "
        f"sigma {SIGMA:g}")
    say("ONE kernel form is built: a per-lane column of 32 uint32 sums in LDS over dense value slots, every tap an LDS add.  The wave-uniform form with at most 8 "
        "slots in registers was not tried.  Tiles of 64 columns x 8 rows up to radius 2, x 16 above (MMSA_VOTE_TH of a debug-knob build overrides the height).")
    if a.note:
        say(a.note)
    g = torch.Generator().manual_seed(7)
    lp = LabelPrep(C)
    lut3, lut1 = VR.range_table(SIGMA, 3), VR.range_table(SIGMA, 1)
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
        palette = torch.randint(0, 256, (C, 3), generator=g)
        frame = (palette[lab.cpu().long()] + torch.randint(-6, 7, (B, H, W, 3), generator=g)).clamp_(0, 255).to(torch.uint8).to(dev).contiguous()
        gray = frame[..., 0].contiguous()
        real = mmsa.suppress_small(pred, 64, num_classes=C, fill=HOLE)
        noise25 = torch.randint(0, C, (B, H, W), generator=g, dtype=torch.uint8).to(dev)
        noise200 = torch.randint(0, 200, (B, H, W), generator=g, dtype=torch.uint8).to(dev)
        npx = B * H * W
        out = torch.empty_like(pred)
        support, support16 = torch.empty(B, H, W, dtype=torch.uint32, device=dev), torch.empty(B, H, W, dtype=torch.uint16, device=dev)
        ebuf = torch.zeros(B, C + 1, C + 1, dtype=torch.int64, device=dev)

        # leg -> (map, radius, keywords of vote_filter)
        spec, what = {}, {}
        for r in RADII:
            spec[f"g{r}"] = (pred, r, dict(num_classes=C, guide=frame, sigma=SIGMA))
            what[f"g{r}"] = f"mmsa_vote_filter_u8 of the class map, 3-channel guide, radius {r}"
        for r in (2, 8):
            spec[f"a{r}"] = (pred, r, dict(num_classes=C, guide=gray, sigma=SIGMA))
            spec[f"w{r}"] = (pred, r, dict(num_classes=C, weights=conf))
            spec[f"gw{r}"] = (pred, r, dict(num_classes=C, guide=frame, sigma=SIGMA, weights=conf))
            spec[f"h{r}"] = (real, r, dict(num_classes=C, guide=frame, sigma=SIGMA, hole=HOLE, where="holes"))
            what[f"a{r}"], what[f"w{r}"] = f"mmsa_vote_filter_u8, 1-channel guide, radius {r}", f"mmsa_vote_filter_u8, weights alone, radius {r}"
            what[f"gw{r}"] = f"mmsa_vote_filter_u8, 3-channel guide and weights, radius {r}"
            what[f"h{r}"] = f"mmsa_vote_filter_u8, the holes of the realistic map alone, 3-channel guide, radius {r}"
        for k, m, r, kw in (("n25", noise25, 2, dict(num_classes=C)), ("n25x", noise25, 16, dict(num_classes=C)), ("n200", noise200, 2, dict()),
                            ("n200x", noise200, 16, dict())):
            spec[k] = (m, r, dict(kw, guide=frame, sigma=SIGMA))
            what[k] = f"mmsa_vote_filter_u8, {25 if k.startswith('n25') else 200}-value noise, 3-channel guide, radius {r}"

        legs = {k: (lambda k=k: mmsa.vote_filter(spec[k][0], spec[k][1], out=out, support=support, **spec[k][2])) for k in spec}
        for r in RADII:
            legs[f"m{r}"] = lambda r=r: mmsa.majority_filter(pred, r, num_classes=C, out=out, support=support16)
            what[f"m{r}"] = f"mmsa_majority_filter_u8 of the class map, radius {r} (the yardstick)"
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
        if pool is not None:
            t0 = time.perf_counter()
            jobs = {}
            for k, (m, r, kw) in spec.items():
                if k not in legs:
                    continue
                host, gd = m.cpu().numpy(), (kw["guide"].cpu().numpy() if "guide" in kw else None)
                wq = VR.wq_of(kw["weights"].cpu().numpy()) if "weights" in kw else None
                role = MR.roles(kw.get("num_classes"), kw.get("hole", ()), ())
                lut = None if gd is None else (lut3 if gd.ndim == 4 else lut1)
                jobs[k] = [pool.apply_async(restate, (host[b], role, r, kw.get("where", "all") == "all", None if gd is None else gd[b], lut,
                                                    None if wq is None else wq[b])) for b in range(B)]
            n_checked = 0
            for k, futures in jobs.items():
                res = [f.get() for f in futures]
                m, r, kw = spec[k]
                for half in (False, True):
                    want_out, want_sup = np.stack([x[half][0] for x in res]), np.stack([x[half][1] for x in res])
                    out.fill_(0xA5)
                    support.fill_(0xA5A5A5A5)
                    mmsa.vote_filter(m, r, half=half, out=out, support=support, **kw)
                    assert np.array_equal(out.cpu().numpy(), want_out), f"{name}: ({k}) half={half}: out is not the restatement's"
                    assert np.array_equal(support.cpu().numpy(), want_sup), f"{name}: ({k}) half={half}: support is not the restatement's"
                    n_checked += 1
                    if not half:
                        changed[k] = int((want_out != m.cpu().numpy()).sum())
            checked = (f"out and support of all {n_checked} (leg, half) combinations equal the numpy restatement on the full-size map byte for byte "
                       f"({time.perf_counter() - t0:.0f} s of restating in {a.workers} processes)")

        # the composition a user had, outside the interleaving
        alt = []
        if not a.legs:
            lut_t = torch.from_numpy(lut3.astype(np.float32)).to(dev)
            for r in RADII:
                need = B * C * (2 * r + 1) ** 2 * H * W * 4
                if need > a.torch_gb * 1e9:
                    alt.append(f"  device torch at radius {r}: not run; the unfolded one-hot canvas [B, {C}, {(2 * r + 1) ** 2}, H W] alone is {need / 1e9:.0f} GB "
                               f"(the limit of this run: {a.torch_gb:g} GB)")
                    continue
                tt = []
                for _ in range(a.torch_reps + 1):
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    tmap = torch.cat([torch_route(pred[b:b + 1], frame[b:b + 1], r, lut_t) for b in range(B)])
                    e1.record()
                    e1.synchronize()
                    tt.append(e0.elapsed_time(e1) * 1e3)
                ours = mmsa.vote_filter(pred, r, num_classes=C, guide=frame, sigma=SIGMA)
                share = float((tmap == ours).float().mean().item())
                alt.append(f"  device torch at radius {r} (one-hot float canvas -> unfold ({need / 1e9:.1f} GB for the batch; run image by image) -> table -> "
                           f"weighted sum -> argmax): median {np.median(tt[1:]):.1f} (events, {a.torch_reps} runs after one warm-up); {share:.6f} of its pixels "
                           "equal the filter's (it gives a tie to the smallest class, also against the own value)")
                del tmap
                torch.cuda.empty_cache()

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
            say(f"  ({k:5s}) {what[k]:86s} median {med[k]:10.2f}   p10 {p10[k]:10.2f}   p90 {p90[k]:10.2f}")
        for k, (_, r, _) in spec.items():
            if k not in med:
                continue
            s = f"  ({k}) = {med[k]:.2f} (its own p10 .. p90 spans {p90[k] - p10[k]:.2f})"
            if f"m{r}" in med:
                b, span = med[f"m{r}"], p90[f"m{r}"] - p10[f"m{r}"]
                s += (f": {med[k] / b:.2f} x (m{r}) = {b:.2f} (its p10 .. p90 spans {span:.2f}; the difference of {med[k] - b:+.2f} lies "
                      f"{'inside' if abs(med[k] - b) <= span else 'beyond'} that span)")
            if "e" in med:
                s += f"; {med[k] / med['e']:.2f} x the floor (e) = {med['e']:.2f} (spans {p90['e'] - p10['e']:.2f})"
            say(s)
        for line in alt:
            say(line)
        del pred, conf, lab, frame, gray, real, noise25, noise200, out, support, support16
        torch.cuda.empty_cache()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
