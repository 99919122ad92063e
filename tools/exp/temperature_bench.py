"""Timing of temperature scaling for profiles/temperature.txt: each `_t` kernel against its untempered sibling, and the sweep kernel
(csrc/temperature.hip, mmsa_temperature_sweep_nchw) at J = 1 against the three launches it stands for and at J = 8 and 16.  Legs interleaved in ONE
process, every repetition timing each leg once (order rotated), `--inner` launches per timing between two events on the launch stream:
  (a) mmsa_slide_argmax_conf            (b) mmsa_slide_argmax_conf_t            the frame-size class map + confidence, T = 2.5
  (c) mmsa_slide_argmax_resized_conf    (d) mmsa_slide_argmax_resized_conf_t    the same at a rescaled size (from a canvas of half the size per axis)
  (e) mmsa_softmax_flip_accum_nchw      (f) mmsa_softmax_flip_accum_nchw_t      the canvas softmax
  (g) canvas softmax + mmsa_argmax_max_nchw + mmsa_eval_calibration: what one temperature costs without the sweep (the map's mmsa_argmax_nchw not counted)
  (h) the sweep at J = 1    (i) at J = 8    (j) at J = 16
25 classes (`--classes`: above 64 the frame-size kernels recompute, and the shape is two 1000 x 1000 maps); two 1024 x 1024 maps (one window per image)
and the 1080 x 1920 frame under six 1024 x 1024 windows; synthetic head-resolution logits
(randn * 6: the cost of these kernels does not depend on the values but for the sweep's bin rounds, so labels come in 32 x 32 patches with 5 % ignored and
the logits are what they are).  Before anything is timed, (b), (d), (f) at T = 1 are checked against (a), (c), (e) bit for bit and (h) against (g)."""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "multimodal-sam-adapter_amd"))
sys.path.insert(0, ROOT)


def patch_labels(B, H, W, C, g):
    coarse = torch.randint(0, C, (B, (H + 31) // 32, (W + 31) // 32), generator=g)
    lab = coarse.repeat_interleave(32, 1).repeat_interleave(32, 2)[:, :H, :W].to(torch.uint8)
    lab[torch.rand(B, H, W, generator=g) < 0.05] = 255
    return lab.contiguous()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--inner", type=int, default=10)
    ap.add_argument("--bins", type=int, default=15)
    ap.add_argument("--temperature", type=float, default=2.5)
    ap.add_argument("--classes", type=int, default=25, help="above 64 the frame-size legs (a), (b) take the recomputing form; two 1000 x 1000 maps then")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.reps < 30:
        raise SystemExit("temperature_bench: at least 30 repetitions (medians and percentiles are reported)")
    if not torch.cuda.is_available():
        raise SystemExit("temperature_bench: no GPU (a timing needs one)")
    import mmsa
    import mmsa.inference as inf
    from mmsa.evaluate import LabelPrep, calibration, geometric_grid, temperature_sweep
    dev = torch.device("cuda", 0)
    C, K, T = a.classes, a.bins, a.temperature
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    say(f"device {torch.cuda.get_device_name(0)}; reps {a.reps}, {a.inner} launches per timing; times in microseconds per launch (leg (g): per three launches); "
        f"{C} classes, {K} bins, T = {T}")
    geos = (("2 x 1024 x 1024, one window per image", inf.MapPlan.whole(2, 1024, 1024), inf.MapPlan.whole(2, 512, 512, ori_shape=(1024, 1024))),
            ("1 x 1080 x 1920, six 1024 x 1024 windows", inf.MapPlan.slide(1, 1080, 1920, (1024, 1024), (768, 768)),
             inf.MapPlan.slide(1, 540, 960, (512, 512), (384, 384), ori_shape=(1080, 1920))))
    if C > 64:      # 1000 rows: the canvas legs' resize launch takes classes x rows <= 65535
        geos = (("2 x 1000 x 1000, one window per image", inf.MapPlan.whole(2, 1000, 1000), inf.MapPlan.whole(2, 500, 500, ori_shape=(1000, 1000))),)
    for name, plan, rplan in geos:
        g = torch.Generator().manual_seed(5)
        B, H, W = plan.B, plan.H, plan.W
        lg = (torch.randn(plan.n, C, plan.hc // 4, plan.wc // 4, generator=g) * 6).to(dev)
        rlg = (torch.randn(rplan.n, C, rplan.hc // 4, rplan.wc // 4, generator=g) * 6).to(dev)
        unc = torch.zeros(1, dtype=torch.int32, device=dev)
        y = inf._canvas_logits(plan, lg, unc).contiguous()
        lab = patch_labels(B, H, W, C, g).to(dev)
        lp = LabelPrep(C)
        out, conf = torch.empty(B, H, W, dtype=torch.uint8, device=dev), torch.empty(B, H, W, device=dev)
        out2, conf2 = torch.empty_like(out), torch.empty_like(conf)
        prob, prob2 = torch.empty_like(y), torch.empty_like(y)
        cal = torch.zeros(B, 3, K, dtype=torch.int64, device=dev)
        sweeps = {J: torch.zeros(B, J, 4, K, dtype=torch.int64, device=dev) for J in (1, 8, 16)}
        grids = {1: [T], 8: geometric_grid(0.5, 4, 8), 16: geometric_grid(0.25, 8, 16)}

        def three():
            inf._softmax_accum(y, prob, it=mmsa.evaluate.inv_temperature(T))
            inf._argmax_max_into(prob, out2, conf2)
            calibration(out2, conf2, lab, lp, cal=cal)

        legs = dict(a=lambda: plan.class_map(lg, out, unc, conf=conf), b=lambda: plan.class_map(lg, out, unc, conf=conf, temperature=T),
                    c=lambda: rplan.class_map(rlg, out, unc, conf=conf, one_pass=True),
                    d=lambda: rplan.class_map(rlg, out, unc, conf=conf, one_pass=True, temperature=T),
                    e=lambda: inf._softmax_accum(y, prob), f=lambda: inf._softmax_accum(y, prob, it=mmsa.evaluate.inv_temperature(T)), g=three,
                    h=lambda: temperature_sweep(y, lab, lp, grids[1], out=sweeps[1]), i=lambda: temperature_sweep(y, lab, lp, grids[8], out=sweeps[8]),
                    j=lambda: temperature_sweep(y, lab, lp, grids[16], out=sweeps[16]))
        # checks: T = 1 is the sibling; the sweep at J = 1 is the three launches
        for p, l, kw in ((plan, lg, {}), (rplan, rlg, dict(one_pass=True))):
            p.class_map(l, out, unc, conf=conf, **kw)
            p.class_map(l, out2, unc, conf=conf2, temperature=1.0, **kw)
            assert torch.equal(out, out2) and torch.equal(conf, conf2), name
        inf._softmax_accum(y, prob)
        inf._softmax_accum(y, prob2, it=1.0)
        assert torch.equal(prob, prob2), name
        del prob2
        three()
        legs["h"]()
        torch.cuda.synchronize()
        assert int(unc.item()) == 0 and torch.equal(sweeps[1][:, 0, :3], cal), name
        for k in legs:          # warm-up
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
        say(f"{name}: {B * H * W} pixels, canvas {tuple(y.shape)}; rescaled legs: {rplan.n} windows of {rplan.hc} x {rplan.wc} on {rplan.H} x {rplan.W} -> "
            f"{rplan.Ho} x {rplan.Wo}; T = 1 equals the sibling bit for bit (three pairs); the sweep at J = 1 equals softmax_t + argmax_max + eval_calibration")
        med = {}
        for k, what in (("a", "slide_argmax_conf"), ("b", "slide_argmax_conf_t"), ("c", "slide_argmax_resized_conf"), ("d", "slide_argmax_resized_conf_t"),
                        ("e", "softmax_flip_accum_nchw"), ("f", "softmax_flip_accum_nchw_t"), ("g", "softmax_t + argmax_max + eval_calibration"),
                        ("h", "temperature_sweep J = 1"), ("i", "temperature_sweep J = 8"), ("j", "temperature_sweep J = 16")):
            t = np.array(times[k])
            med[k] = float(np.median(t))
            say(f"  ({k}) {what:44s} median {med[k]:9.2f}   p10 {np.percentile(t, 10):9.2f}   p90 {np.percentile(t, 90):9.2f}   spread "
                f"{np.percentile(t, 90) - np.percentile(t, 10):7.2f}")
        say(f"  (b) - (a) = {med['b'] - med['a']:.2f} us, (d) - (c) = {med['d'] - med['c']:.2f} us, (f) - (e) = {med['f'] - med['e']:.2f} us; "
            f"(h) / (g) = {med['h'] / med['g']:.2f}; per temperature: J = 8 {med['i'] / 8:.2f} us, J = 16 {med['j'] / 16:.2f} us, against (g) {med['g']:.2f} us")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
