"""Timing of the uncertainty maps for profiles/uncertainty.txt.  Legs interleaved in ONE process, every repetition timing each leg once (order rotated),
`--inner` calls per timing between two events on the launch stream, all from the same seeded head-resolution logits:
  (c)  the `confidence=True` class-map launch (mmsa_slide_argmax_conf / mmsa_slide_argmax_resized_conf): the parent's code, unchanged in this build -- the yardstick;
  (k1) the `_score` launch writing the top-2 margin, (k2) the same launch writing the entropy score (mmsa_slide_argmax_score / mmsa_slide_argmax_resized_score);
  (m1) / (m2) the canvas alternative for the same score: the probabilities on canvases (the launches of `probabilities` after the head), then
       mmsa_argmax_score_nchw.
Shapes, 25 classes: two 1024 x 1024 maps (whole mode, one window each) and the six-window 1080 x 1920 frame (1024 x 1024 windows, stride 640), each at its
own size (the per-lane LDS column) and rescaled (the recomputing form); then two 1000 x 1000 maps at 65 classes, where the frame-size launch recomputes as well
(1000 rows: the canvas leg's resize launch takes classes x rows <= 65535).
Every score of a one-pass leg is checked against the canvas leg's bit for bit first, every map against the argmax of the canvas logits.  No threshold: the
medians and p10 .. p90 spreads are the record; the default of `one_pass=` for a score follows from (k) against (m) beyond the spread of (c)."""
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
        raise SystemExit("uncertainty_bench: no GPU (a timing needs one)")
    import mmsa.inference as inf
    dev = torch.device("cuda", 0)
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    def logits(n, C, g):
        coarse = torch.randn(n, C, 32, 32, generator=g)
        return (torch.nn.functional.interpolate(coarse, size=(256, 256), mode="bilinear") + 0.05 * torch.randn(n, C, 256, 256, generator=g)).to(dev)

    what = dict(c="confidence launch (the yardstick)", k1="score launch, margin", k2="score launch, entropy",
                m1="canvases + mmsa_argmax_score_nchw, margin", m2="canvases + mmsa_argmax_score_nchw, entropy")

    def measure(name, legs, check):
        for _ in range(2):
            for k in legs:
                legs[k]()
        torch.cuda.synchronize()
        check()
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
        say(f"{name}; map and score of every one-pass leg equal the canvas leg's bit for bit")
        for k in legs:
            t = np.array(times[k])
            say(f"  ({k:2s}) {what[k]:46s} median {np.median(t):10.2f}   p10 {np.percentile(t, 10):10.2f}   p90 {np.percentile(t, 90):10.2f}")
        med = {k: float(np.median(times[k])) for k in legs}
        spread = float(np.percentile(times["c"], 90) - np.percentile(times["c"], 10))
        say(f"  (k1) - (c) = {med['k1'] - med['c']:+.2f}; (k2) - (c) = {med['k2'] - med['c']:+.2f}; (m1) - (k1) = {med['m1'] - med['k1']:+.2f}; "
            f"(m2) - (k2) = {med['m2'] - med['k2']:+.2f}; p10 .. p90 of (c) spans {spread:.2f}")

    say(f"device {torch.cuda.get_device_name(0)}; reps {a.reps}, {a.inner} calls per timing; times in microseconds per call")
    g = torch.Generator().manual_seed(7)
    frame_cfg = ((1024, 1024), (640, 640))
    for C, name, plan in ((25, "two 1024 x 1024 maps", inf.MapPlan.whole(2, 1024, 1024)),
                          (25, "1080 x 1920 frame, six windows", inf.MapPlan.slide(1, 1080, 1920, *frame_cfg)),
                          (25, "two 1024 x 1024 maps -> (1200, 1200)", inf.MapPlan.whole(2, 1024, 1024, ori_shape=(1200, 1200))),
                          (25, "1080 x 1920 frame, six windows -> (720, 1280)", inf.MapPlan.slide(1, 1080, 1920, *frame_cfg, (720, 1280))),
                          (65, "two 1000 x 1000 maps, the recomputing form", inf.MapPlan.whole(2, 1000, 1000))):
        lg = logits(plan.n, C, g)
        size = (plan.B, plan.Ho, plan.Wo)
        keys = ("c", "k1", "k2", "m1", "m2")
        out = {k: torch.empty(size, dtype=torch.uint8, device=dev) for k in keys}
        conf = {k: torch.empty(size, dtype=torch.float32, device=dev) for k in keys}
        unc = torch.zeros(1, dtype=torch.int32, device=dev)
        op = dict(one_pass=True) if plan.rescaled else {}
        kept = {}

        def canvas(k, kind, plan=plan, lg=lg, out=out, conf=conf, unc=unc, kept=kept):
            y = inf._canvas_logits(plan, lg, unc)[:, :, :plan.Ho, :plan.Wo].contiguous()
            p = torch.empty_like(y)
            inf._softmax_accum(y, p)
            inf._argmax_score_into(p, out[k], conf[k], kind)
            kept["y"] = y

        legs = dict(c=lambda plan=plan, lg=lg, out=out, conf=conf, unc=unc, op=op: plan.class_map(lg, out["c"], unc, conf=conf["c"], **op),
                    k1=lambda plan=plan, lg=lg, out=out, conf=conf, unc=unc, op=op: plan.class_map(lg, out["k1"], unc, conf=conf["k1"], score="margin", **op),
                    k2=lambda plan=plan, lg=lg, out=out, conf=conf, unc=unc, op=op: plan.class_map(lg, out["k2"], unc, conf=conf["k2"], score="entropy", **op),
                    m1=lambda canvas=canvas: canvas("m1", 1), m2=lambda canvas=canvas: canvas("m2", 2))

        def check(out=out, conf=conf, kept=kept, name=name):
            want = inf.argmax_map(kept["y"])
            for k in ("c", "k1", "k2"):
                assert torch.equal(out[k], want), f"{name}: the map of leg ({k}) differs from the canvas path"
            assert torch.equal(conf["k1"], conf["m1"]) and torch.equal(conf["k2"], conf["m2"]), f"{name}: a one-pass score differs from the canvas leg's"

        measure(f"{name}: {C} classes, {plan.n} windows, {plan.B * plan.Ho * plan.Wo} output pixels", legs, check)
        assert int(unc.item()) == 0
        del lg, out, conf, kept
        torch.cuda.empty_cache()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
