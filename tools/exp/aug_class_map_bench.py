"""Timing of the augmented class map (aug_test) for profiles/aug_class_map.txt.  Legs interleaved in ONE process, every repetition timing each leg once
(order rotated), `--inner` calls per timing between two events on the launch stream, from the same seeded head-resolution logits of every view:
  (c) the canvas path -- per view: canvas (bilinear_accum per window, div_count), second canvas where the view has another size, softmax / un-flip /
      accumulate (mmsa_softmax_flip_accum_nchw); then argmax_nchw: as mmsa.inference.AugPlan.mean_probabilities + argmax_map issue them (their memsets and
      count checks included: they are part of that path);
  (o) mmsa_aug_argmax, one launch.
Shapes: the six-window 1080 x 1920 frame at 25 classes, ori_shape (1080, 1920); views {1.0, 1.0 flipped} and {1.0, 1.25} x {plain, flipped} (the 1.25 x
view is 1350 x 2400: eight 1024 x 1024 windows, up to six on a pixel).  A third case runs the two 1.0 views under four windows (stride (56, 896)), where no pixel has more than four windows on a tap: the
kernel's register-slot form alone, without the scanning form of taps under 5 .. 8 windows.  Every (o) map is checked against (c) bit for bit first.  The default
(mmsa.inference.ONE_PASS_AUG_DEFAULT) is one pass only where the medians differ by more than the p10 .. p90 spread of the canvas path in its favour."""
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
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--inner", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("aug_class_map_bench: no GPU (a timing needs one)")
    import mmsa.inference as inf
    dev = torch.device("cuda", 0)
    C, ori = 25, (1080, 1920)
    tc = dict(mode="slide", crop_size=(1024, 1024), stride=(640, 640))
    tc4 = dict(tc, stride=(56, 896))      # the same frame under four windows: at most 4 on a pixel, so no pixel takes the kernel's scanning form
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    say(f"device {torch.cuda.get_device_name(0)}; reps {a.reps}, {a.inner} calls per timing; times in microseconds per call")
    small, large = (1, 1080, 1920), (1, 1350, 2400)
    cases = [("views 1.0, 1.0 flipped", tc, [small, small], [None, "horizontal"]),
             ("views 1.0, 1.0 flipped, 1.25, 1.25 flipped", tc, [small, small, large, large], [None, "horizontal", None, "horizontal"]),
             ("views 1.0, 1.0 flipped, stride (56, 896): no pixel under more than 4 windows", tc4, [small, small], [None, "horizontal"])]
    for name, cfg, shapes, flips in cases:
        plan = inf.AugPlan.make(cfg, shapes, flips, ori_shape=ori)
        g = torch.Generator().manual_seed(7)
        lgs = []
        for p in plan.plans:
            coarse = torch.randn(p.n, C, 32, 32, generator=g)
            lgs.append((torch.nn.functional.interpolate(coarse, size=(256, 256), mode="bilinear") + 0.05 * torch.randn(p.n, C, 256, 256, generator=g)).to(dev))
        B, Ho, Wo = plan.size
        out = {k: torch.empty(B, Ho, Wo, dtype=torch.uint8, device=dev) for k in "co"}
        unc = torch.zeros(1, dtype=torch.int32, device=dev)
        legs = dict(c=lambda: out["c"].copy_(inf.argmax_map(plan.mean_probabilities(lgs, unc))), o=lambda: plan.class_map(lgs, out["o"], unc, one_pass=True))
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
        say(f"{name}: {[p.n for p in plan.plans]} windows -> {ori}, {C} classes, {B * Ho * Wo} output pixels; the one-pass map equals the canvas path bit for bit")
        for k, what in (("c", "canvas path: per view canvas, resize, softmax + add; argmax"), ("o", "mmsa_aug_argmax, one launch")):
            t = np.array(times[k])
            say(f"  ({k}) {what:58s} median {np.median(t):10.2f}   p10 {np.percentile(t, 10):10.2f}   p90 {np.percentile(t, 90):10.2f}")
        tc_, to_ = np.array(times["c"]), np.array(times["o"])
        spread = np.percentile(tc_, 90) - np.percentile(tc_, 10)
        say(f"  canvas path / one pass = {np.median(tc_) / np.median(to_):.2f}; medians differ by {np.median(tc_) - np.median(to_):.2f}, spread of the canvas path {spread:.2f}")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
