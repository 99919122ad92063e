"""Timing of the rescaled class map for profiles/rescale_class_map.txt.  Legs interleaved in ONE process, every repetition timing each leg once (order
rotated), `--inner` calls per timing between two events on the launch stream, from the same seeded head-resolution logits:
  (c) the canvas path -- what the parent commit runs: canvas (bilinear_accum per window, div_count), second canvas (bilinear_accum, write), argmax_nchw,
      as mmsa.inference._rescaled_map_canvas issues them (its two memsets and its count check included: they are part of that path);
  (o) mmsa_slide_argmax_resized, one launch;
  (y) mmsa_slide_argmax at the frame's own size -- the yardstick for the spread: one launch of the sibling kernel, no rescale.
Shapes: the six-window 1080 x 1920 frame at 25 classes rescaled up to (1200, 2133) and down to (810, 1440); two 1024 x 1024 whole frames to (1042, 1042).
Every (o) map is checked against (c) bit for bit first."""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "multimodal-sam-adapter_amd"))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=40)
    ap.add_argument("--inner", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("rescale_class_map_bench: no GPU (a timing needs one)")
    import mmsa.inference as inf
    from mmsa import lib, ops
    dev = torch.device("cuda", 0)
    C = 25
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    say(f"device {torch.cuda.get_device_name(0)}; reps {a.reps}, {a.inner} calls per timing; times in microseconds per call")
    slide = lambda ori: inf.MapPlan.slide(1, 1080, 1920, (1024, 1024), (640, 640), ori_shape=ori)
    cases = [("slide 1080 x 1920, six 1024 x 1024 windows", slide((1200, 2133))), ("slide 1080 x 1920, six 1024 x 1024 windows", slide((810, 1440))),
             ("whole 2 x 1024 x 1024", inf.MapPlan.whole(2, 1024, 1024, ori_shape=(1042, 1042)))]
    for name, plan in cases:
        B, H, W, Hd, Wd, n, tab = plan.B, plan.H, plan.W, plan.Hd, plan.Wd, plan.n, plan.tab
        g = torch.Generator().manual_seed(7)
        coarse = torch.randn(n, C, 32, 32, generator=g)
        lg = (torch.nn.functional.interpolate(coarse, size=(256, 256), mode="bilinear") + 0.05 * torch.randn(n, C, 256, 256, generator=g)).to(dev)
        out = {k: torch.empty(B, Hd, Wd, dtype=torch.uint8, device=dev) for k in "co"}
        same = torch.empty(B, H, W, dtype=torch.uint8, device=dev)
        unc = torch.zeros(1, dtype=torch.int32, device=dev)
        legs = dict(c=lambda: inf._rescaled_map_canvas(plan, lg, out["c"], unc),
                    o=lambda: lib.call("mmsa_slide_argmax_resized", lg.data_ptr(), n, C, 256, 256, tab, out["o"].data_ptr(), B, H, W, 1024, 1024, Hd, Wd, Hd, Wd,
                                       unc.data_ptr(), ops._stream()),
                    y=lambda: lib.call("mmsa_slide_argmax", lg.data_ptr(), n, C, 256, 256, tab, same.data_ptr(), B, H, W, 1024, 1024, unc.data_ptr(), ops._stream()))
        for _ in range(2):
            for k in legs:
                legs[k]()
        torch.cuda.synchronize()
        assert int(unc.item()) == 0 and torch.equal(out["c"], out["o"]), "the one-pass map differs from the canvas path"
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
        say(f"{name} -> ({Hd}, {Wd}), {C} classes, {B * Hd * Wd} output pixels; the one-pass map equals the canvas path bit for bit")
        for k, what in (("c", "canvas path (parent): canvas, second canvas, argmax"), ("o", "mmsa_slide_argmax_resized, one launch"),
                        ("y", "mmsa_slide_argmax at the frame's size (yardstick)")):
            t = np.array(times[k])
            say(f"  ({k}) {what:52s} median {np.median(t):9.2f}   p10 {np.percentile(t, 10):9.2f}   p90 {np.percentile(t, 90):9.2f}")
        say(f"  canvas path / one pass = {np.median(times['c']) / np.median(times['o']):.2f}")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
