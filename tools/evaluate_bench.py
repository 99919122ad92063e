"""Timing of the evaluation kernels against the class-map kernel they extend (profiles/evaluate.txt).  Four legs, interleaved in ONE process, every
repetition timing each leg once (order rotated), `--inner` launches per timing between two events on the launch stream:
  (a) mmsa_slide_argmax alone -- the yardstick: its kernel is the one that was there before the evaluation entries;
  (b) mmsa_slide_argmax, then mmsa_eval_confusion_u8 on the stored map;
  (c) mmsa_slide_argmax_eval writing the map;
  (d) mmsa_slide_argmax_eval with out == NULL;
  (s) mmsa_eval_confusion_u8 alone (bytes moved = 2 per pixel: one class map byte, one label byte).
Workloads: logits [2, 25, 256, 256] -> two 1024 x 1024 maps (whole-image inference), and the six 1024 x 1024 windows (stride 640) of a 1080 x 1920 frame.
Prints medians, the 10th / 90th percentiles, and the standalone kernel's achieved TB/s; checks first that (b), (c), (d) give the same counts."""
import argparse
import ctypes
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "multimodal-sam-adapter_amd"))


def smooth_logits(n, C, hs, ws, g):
    import torch.nn.functional as F
    low = torch.randn(n, C, hs // 8, ws // 8, generator=g)
    return (F.interpolate(low, size=(hs, ws), mode="bilinear", align_corners=False) + 0.05 * torch.randn(n, C, hs, ws, generator=g)).contiguous()


def patch_labels(B, H, W, C, g):
    coarse = torch.randint(0, C, (B, (H + 31) // 32, (W + 31) // 32), generator=g)
    lab = coarse.repeat_interleave(32, 1).repeat_interleave(32, 2)[:, :H, :W].to(torch.uint8)
    lab[torch.rand(B, H, W, generator=g) < 0.05] = 255
    return lab.contiguous()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=40)
    ap.add_argument("--inner", type=int, default=20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("evaluate_bench: no GPU (a timing needs one)")
    from mmsa import lib, ops
    from mmsa.evaluate import LabelPrep, confusion, slide_argmax_eval
    import mmsa.inference as inf
    dev = torch.device("cuda", 0)
    C = 25
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    say(f"device {torch.cuda.get_device_name(0)}; reps {a.reps}, {a.inner} launches per timing; times in microseconds per launch (or pair of launches)")
    for name, B, H, W, jobs in (("2 x 1024 x 1024, one window per image", 2, 1024, 1024, [(b, 0, 0) for b in range(2)]),
                                ("1080 x 1920, six 1024 x 1024 windows, stride 640", 1, 1080, 1920,
                                 [(0, y1, x1) for (y1, x1, _, _) in inf.crop_boxes(1080, 1920, (1024, 1024), (640, 640))])):
        g = torch.Generator().manual_seed(5)
        n = len(jobs)
        lg = smooth_logits(n, C, 256, 256, g).to(dev)
        lab = patch_labels(B, H, W, C, g).to(dev)
        tab = (ctypes.c_int * (3 * n))(*[v for j in jobs for v in j])
        lp = LabelPrep(C)
        out = torch.empty(B, H, W, dtype=torch.uint8, device=dev)
        unc = torch.zeros(1, dtype=torch.int32, device=dev)
        cnt = {k: torch.zeros(B, C + 1, C + 1, dtype=torch.int64, device=dev) for k in "bcds"}

        def plain():
            lib.call("mmsa_slide_argmax", lg.data_ptr(), n, C, 256, 256, tab, out.data_ptr(), B, H, W, 1024, 1024, unc.data_ptr(), ops._stream())
        legs = dict(a=plain,
                    b=lambda: (plain(), confusion(out, lab, lp, counts=cnt["b"])),
                    c=lambda: slide_argmax_eval(lg, n, tab, out, B, H, W, 1024, 1024, unc, lab, lp, cnt["c"]),
                    d=lambda: slide_argmax_eval(lg, n, tab, None, B, H, W, 1024, 1024, unc, lab, lp, cnt["d"]),
                    s=lambda: confusion(out, lab, lp, counts=cnt["s"]))
        for k in "abcds":       # warm-up, and the legs agree
            legs[k]()
        torch.cuda.synchronize()
        assert int(unc.item()) == 0
        assert torch.equal(cnt["b"], cnt["c"]) and torch.equal(cnt["b"], cnt["d"]) and torch.equal(cnt["b"], cnt["s"]) and int(cnt["b"].sum()) > 0
        nz = int((cnt["b"] != 0).sum())
        times = {k: [] for k in legs}
        order = list(legs)
        for r in range(a.reps):
            for k in order[r % len(order):] + order[:r % len(order)]:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(a.inner):
                    legs[k]()
                e1.record()
                e1.synchronize()
                times[k].append(e0.elapsed_time(e1) * 1e3 / a.inner)
        say()
        say(f"{name}: {B * H * W} pixels, {n} windows, {nz} non-zero count bins")
        med = {}
        for k, what in (("a", "slide_argmax alone (yardstick)"), ("b", "slide_argmax + eval_confusion_u8"), ("c", "slide_argmax_eval with the map"),
                        ("d", "slide_argmax_eval, out == NULL"), ("s", "eval_confusion_u8 alone")):
            t = np.array(times[k])
            med[k] = float(np.median(t))
            say(f"  ({k}) {what:36s} median {med[k]:9.2f}   p10 {np.percentile(t, 10):9.2f}   p90 {np.percentile(t, 90):9.2f}")
        ta = np.array(times["a"])
        spread = float(np.percentile(ta, 90) - np.percentile(ta, 10))
        say(f"  spread of the yardstick (p90 - p10): {spread:.2f} us = {100 * spread / med['a']:.1f} % of its median")
        say(f"  (b) - (a) = {med['b'] - med['a']:.2f} us, (c) - (a) = {med['c'] - med['a']:.2f} us, (d) - (a) = {med['d'] - med['a']:.2f} us; (b) - (c) = {med['b'] - med['c']:.2f} us")
        say(f"  eval_confusion_u8 alone: {2 * B * H * W} bytes read -> {2 * B * H * W / (med['s'] * 1e-6) / 1e12:.3f} TB/s (launch included)")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
