"""Timing of the top-k maps for profiles/topk.txt.  Legs interleaved in ONE process, every repetition timing each leg once (order rotated), `--inner` calls
per timing between two events on the launch stream, all from the same seeded head-resolution logits:
  (c)  the `confidence=True` class-map launch (mmsa_slide_argmax_conf / mmsa_slide_argmax_resized_conf): the parent's code, unchanged in this build -- the yardstick;
  (k2) / (k8) the top-k launch of the plan for K = 2 / K = 8: mmsa_slide_argmax_topk at the frame's size, the canvas path + mmsa_argmax_topk_nchw at a rescaled size;
  (t2) / (t8) the canvas alternative a user has without it: the probabilities on canvases (the launches of `probabilities` after the head), then torch.topk.
Shapes, 25 classes: two 1024 x 1024 maps (whole mode, one window each) and the six-window 1080 x 1920 frame (1024 x 1024 windows, stride 640), each at its
own size (the per-lane LDS column) and at the rescaled targets of profiles/uncertainty.txt (the canvas path, the only one built); then two 1000 x 1000 maps at
65 classes, where the frame-size launch recomputes in three passes.  Then the evaluation pass: mmsa_eval_topk_u8 on the K = 2 / K = 8 class planes against
mmsa_eval_confusion_u8 on plane 0 (the yardstick), on the frame-size maps.
Every plane of a (k) leg is checked first: plane 0 of the classes against the map of (c), plane 0 of the probabilities against its confidence, bit for bit, and
the probabilities against torch.topk's values (equal as sets of values per pixel: the same float32 numbers, whatever the order of ties).  No threshold: the
medians and p10 .. p90 spreads are the record."""
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
        raise SystemExit("topk_bench: no GPU (a timing needs one)")
    import mmsa
    import mmsa.inference as inf
    from mmsa.evaluate import LabelPrep
    dev = torch.device("cuda", 0)
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    def logits(n, C, g):
        coarse = torch.randn(n, C, 32, 32, generator=g)
        return (torch.nn.functional.interpolate(coarse, size=(256, 256), mode="bilinear") + 0.05 * torch.randn(n, C, 256, 256, generator=g)).to(dev)

    def measure(name, legs, what, check, yard):
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
        say(name)
        for k in legs:
            t = np.array(times[k])
            say(f"  ({k:2s}) {what[k]:52s} median {np.median(t):10.2f}   p10 {np.percentile(t, 10):10.2f}   p90 {np.percentile(t, 90):10.2f}")
        med = {k: float(np.median(times[k])) for k in legs}
        spread = float(np.percentile(times[yard], 90) - np.percentile(times[yard], 10))
        say("  " + "; ".join(f"({k}) - ({yard}) = {med[k] - med[yard]:+.2f}" for k in legs if k != yard) + f"; p10 .. p90 of ({yard}) spans {spread:.2f}")

    say(f"device {torch.cuda.get_device_name(0)}; reps {a.reps}, {a.inner} calls per timing; times in microseconds per call")
    g = torch.Generator().manual_seed(7)
    frame_cfg = ((1024, 1024), (640, 640))
    what = dict(c="confidence launch (the yardstick)", k2="top-k launch of the plan, K = 2", k8="top-k launch of the plan, K = 8",
                t2="canvases + torch.topk, K = 2", t8="canvases + torch.topk, K = 8")
    planes = {}
    for C, name, plan in ((25, "two 1024 x 1024 maps", inf.MapPlan.whole(2, 1024, 1024)),
                          (25, "1080 x 1920 frame, six windows", inf.MapPlan.slide(1, 1080, 1920, *frame_cfg)),
                          (25, "two 1024 x 1024 maps -> (1200, 1200)", inf.MapPlan.whole(2, 1024, 1024, ori_shape=(1200, 1200))),
                          (25, "1080 x 1920 frame, six windows -> (720, 1280)", inf.MapPlan.slide(1, 1080, 1920, *frame_cfg, (720, 1280))),
                          (65, "two 1000 x 1000 maps, the recomputing form", inf.MapPlan.whole(2, 1000, 1000))):
        lg = logits(plan.n, C, g)
        size = (plan.B, plan.Ho, plan.Wo)
        out = torch.empty(size, dtype=torch.uint8, device=dev)
        conf = torch.empty(size, dtype=torch.float32, device=dev)
        tk = {K: inf.TopK(torch.empty((K,) + size, dtype=torch.uint8, device=dev), torch.empty((K,) + size, dtype=torch.float32, device=dev)) for K in (2, 8)}
        unc = torch.zeros(1, dtype=torch.int32, device=dev)
        op = dict(one_pass=True) if plan.rescaled else {}
        kept = {}

        def canvas(K, plan=plan, lg=lg, unc=unc, kept=kept):
            y = inf._canvas_logits(plan, lg, unc)[:, :, :plan.Ho, :plan.Wo].contiguous()
            p = torch.empty_like(y)
            inf._softmax_accum(y, p)
            kept[K] = torch.topk(p, K, dim=1)

        legs = dict(c=lambda plan=plan, lg=lg, out=out, conf=conf, unc=unc, op=op: plan.class_map(lg, out, unc, conf=conf, **op),
                    k2=lambda plan=plan, lg=lg, tk=tk, unc=unc: plan.class_map(lg, tk[2].classes[0], unc, topk=tk[2]),
                    k8=lambda plan=plan, lg=lg, tk=tk, unc=unc: plan.class_map(lg, tk[8].classes[0], unc, topk=tk[8]),
                    t2=lambda canvas=canvas: canvas(2), t8=lambda canvas=canvas: canvas(8))

        def check(out=out, conf=conf, tk=tk, kept=kept, name=name):
            for K in (2, 8):
                assert torch.equal(tk[K].classes[0], out) and torch.equal(tk[K].probs[0], conf), f"{name}: plane 0 of K = {K} is not the map / the confidence of (c)"
                assert torch.equal(tk[K].probs.permute(1, 0, 2, 3), kept[K].values), f"{name}: the probabilities of K = {K} are not torch.topk's values"

        path = "the canvas path + mmsa_argmax_topk_nchw" if plan.rescaled else "mmsa_slide_argmax_topk, " + ("LDS column" if C <= 64 else "three recomputing passes")
        measure(f"{name}: {C} classes, {plan.n} windows, {plan.B * plan.Ho * plan.Wo} output pixels; (k) = {path}; plane 0 equals (c), the values equal torch.topk's",
                legs, what, check, "c")
        assert int(unc.item()) == 0
        if C == 25 and not plan.rescaled:
            planes[name] = (tk[2].classes.clone(), tk[8].classes.clone())
        del lg, out, conf, tk, kept
        torch.cuda.empty_cache()
    # the evaluation pass against the confusion pass on the same maps
    ewhat = dict(e="mmsa_eval_confusion_u8 on plane 0 (the yardstick)", r2="mmsa_eval_topk_u8, K = 2", r8="mmsa_eval_topk_u8, K = 8")
    lp = LabelPrep(25)
    for name, (c2, c8) in planes.items():
        B = c2.shape[1]
        lab = torch.randint(0, 25, tuple(c2.shape[1:]), generator=g, dtype=torch.uint8).to(dev)
        lab = torch.where(torch.rand(lab.shape, device=dev) < 0.6, c2[0], lab)                      # mostly right, as a trained model is
        bufs = dict(e=torch.zeros(B, 26, 26, dtype=torch.int64, device=dev), r2=torch.zeros(B, 25, 3, dtype=torch.int64, device=dev),
                    r8=torch.zeros(B, 25, 9, dtype=torch.int64, device=dev))
        legs = dict(e=lambda c2=c2, lab=lab, bufs=bufs: mmsa.confusion(c2[0], lab, lp, counts=bufs["e"]),
                    r2=lambda c2=c2, lab=lab, bufs=bufs: mmsa.topk_counts(c2, lab, lp, counts=bufs["r2"]),
                    r8=lambda c8=c8, lab=lab, bufs=bufs: mmsa.topk_counts(c8, lab, lp, counts=bufs["r8"]))

        def check(c2=c2, c8=c8, lab=lab):
            e = mmsa.confusion(c2[0], lab, lp)
            for c in (c2, c8):
                r = mmsa.topk_counts(c, lab, lp)
                assert torch.equal(r[:, :, 0], torch.diagonal(e, dim1=1, dim2=2)[:, :25]) and torch.equal(r.sum(2), e.sum(2)[:, :25])

        measure(f"evaluation, {name}: column 0 and the row sums equal the confusion pass's", legs, ewhat, check, "e")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
