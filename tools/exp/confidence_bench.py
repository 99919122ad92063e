"""Timing of the confidence maps for profiles/confidence.txt.  Legs interleaved in ONE process, every repetition timing each leg once (order rotated),
`--inner` calls per timing between two events on the launch stream, all from the same seeded head-resolution logits:
  (p) the plain class-map launch (mmsa_slide_argmax / mmsa_slide_argmax_resized / mmsa_aug_argmax): the parent's code, unchanged in this build;
  (k) its `_conf` sibling, which also writes the confidence map (at the frame's size and 25 classes: the LDS-column form);
  (s) frame size only: the second-pass form of the `_conf` kernel for every C, from a -DMMSA_CONF_SECOND_PASS build of segment.hip
      (tools/build_variant.sh tools/exp/bin/libmmsa_conf_pass2.so segment.hip -DMMSA_CONF_SECOND_PASS); skipped when that library is not there;
  (t) what a caller does today: the probabilities on canvases (the launches of `probabilities` / `aug_inference` after the head), then torch's .max(1);
  (m) the canvas path of this build: the same canvases, then mmsa_argmax_max_nchw.
Shapes, 25 classes: two 1024 x 1024 maps (whole mode, one window each) and the six-window 1080 x 1920 frame (1024 x 1024 windows, stride 640), each at its
own size and rescaled; the frame's two views (plain, flipped) for the augmented launch.  Every confidence map is checked against (t)'s bit for bit first, every one-view
class map against the argmax of the canvas logits, the augmented ones against the argmax of the mean probabilities.  No threshold: the medians and p10 .. p90 spreads are the record."""
import argparse
import ctypes
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "multimodal-sam-adapter_amd"))
sys.path.insert(0, ROOT)
PASS2_LIB = os.path.join(ROOT, "tools", "exp", "bin", "libmmsa_conf_pass2.so")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--inner", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("confidence_bench: no GPU (a timing needs one)")
    import mmsa.inference as inf
    from mmsa import lib, ops
    dev = torch.device("cuda", 0)
    C = 25
    pass2 = None
    if os.path.exists(PASS2_LIB):
        pass2 = ctypes.CDLL(PASS2_LIB).mmsa_slide_argmax_conf
        pass2.argtypes, pass2.restype = lib.SIGNATURES["mmsa_slide_argmax_conf"], ctypes.c_int
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    def logits(n, g):
        coarse = torch.randn(n, C, 32, 32, generator=g)
        return (torch.nn.functional.interpolate(coarse, size=(256, 256), mode="bilinear") + 0.05 * torch.randn(n, C, 256, 256, generator=g)).to(dev)

    def measure(name, legs, results):
        for _ in range(2):
            for k in legs:
                legs[k]()
        torch.cuda.synchronize()
        want_map, want_conf = results["t"]()
        for k in legs:
            if k == "t":
                continue
            got_map, got_conf = results[k]()
            assert got_map is None or torch.equal(got_map, want_map), f"{name}: the map of leg ({k}) differs from the canvas path"
            assert k == "p" or torch.equal(got_conf, want_conf), f"{name}: the confidence of leg ({k}) differs from the canvas path"
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
        say(f"{name}; map and confidence of every leg equal the canvas path bit for bit")
        what = dict(p="plain class-map launch", k="_conf launch", s="_conf launch, second-pass form (measurement build)",
                    t="today: probabilities on canvases, torch .max(1)", m="canvases, mmsa_argmax_max_nchw")
        for k in legs:
            t = np.array(times[k])
            say(f"  ({k}) {what[k]:52s} median {np.median(t):10.2f}   p10 {np.percentile(t, 10):10.2f}   p90 {np.percentile(t, 90):10.2f}")
        med = {k: float(np.median(times[k])) for k in legs}
        extra = f"; (s) - (k) = {med['s'] - med['k']:+.2f}" if "s" in med else ""
        say(f"  (k) - (p) = {med['k'] - med['p']:+.2f}; (t) / (k) = {med['t'] / med['k']:.2f}; (t) - (m) = {med['t'] - med['m']:+.2f}{extra}")

    say(f"device {torch.cuda.get_device_name(0)}; reps {a.reps}, {a.inner} calls per timing; times in microseconds per call; {C} classes")
    g = torch.Generator().manual_seed(7)
    frame_cfg = ((1024, 1024), (640, 640))
    for name, plan in (("two 1024 x 1024 maps", inf.MapPlan.whole(2, 1024, 1024)),
                       ("1080 x 1920 frame, six windows", inf.MapPlan.slide(1, 1080, 1920, *frame_cfg)),
                       ("two 1024 x 1024 maps -> (1200, 1200)", inf.MapPlan.whole(2, 1024, 1024, ori_shape=(1200, 1200))),
                       ("1080 x 1920 frame, six windows -> (720, 1280)", inf.MapPlan.slide(1, 1080, 1920, *frame_cfg, (720, 1280)))):
        lg = logits(plan.n, g)
        size = (plan.B, plan.Ho, plan.Wo)
        out = {k: torch.empty(size, dtype=torch.uint8, device=dev) for k in "pksm"}
        conf = {k: torch.empty(size, dtype=torch.float32, device=dev) for k in "ksm"}
        unc = torch.zeros(1, dtype=torch.int32, device=dev)
        today = {}
        op = dict(one_pass=True) if plan.rescaled else {}

        def leg_t(plan=plan, lg=lg, today=today, unc=unc):
            y = inf._canvas_logits(plan, lg, unc)
            p = torch.empty_like(y)
            inf._softmax_accum(y, p)
            today["y"], today["r"] = y, p.max(1)

        legs = dict(p=lambda plan=plan, lg=lg, out=out, unc=unc, op=op: plan.class_map(lg, out["p"], unc, **op),
                    k=lambda plan=plan, lg=lg, out=out, conf=conf, unc=unc, op=op: plan.class_map(lg, out["k"], unc, conf=conf["k"], **op))
        if pass2 is not None and not plan.rescaled:
            legs["s"] = lambda plan=plan, lg=lg, out=out, conf=conf, unc=unc: pass2(*plan._args(lg, out["s"], conf["s"]), unc.data_ptr(), ops._stream())
        legs["t"] = leg_t
        if plan.rescaled:
            legs["m"] = lambda plan=plan, lg=lg, out=out, conf=conf, unc=unc: plan.class_map(lg, out["m"], unc, conf=conf["m"], one_pass=False)
        else:
            def leg_m(plan=plan, lg=lg, out=out, conf=conf, unc=unc):
                y = inf._canvas_logits(plan, lg, unc)
                p = torch.empty_like(y)
                inf._softmax_accum(y, p)
                inf._argmax_max_into(p, out["m"], conf["m"])
            legs["m"] = leg_m
        results = {k: (lambda k=k, out=out, conf=conf: (out[k], conf.get(k))) for k in "pksm"}
        if not plan.rescaled:
            results["m"] = lambda conf=conf: (None, conf["m"])      # this leg's map is the argmax of the PROBABILITIES, which may merge two near-equal logits
        results["t"] = lambda today=today: (inf.argmax_map(today["y"]), today["r"].values)
        measure(f"{name}: {plan.n} windows, {plan.B * plan.Ho * plan.Wo} output pixels", legs, results)
        assert int(unc.item()) == 0

    # the augmented launch: the frame's two views, plain and flipped
    tc = dict(mode="slide", crop_size=(1024, 1024), stride=(640, 640))
    plan = inf.AugPlan.make(tc, [(1, 1080, 1920)] * 2, [None, "horizontal"], ori_shape=(1080, 1920))
    lgs = [logits(p.n, g) for p in plan.plans]
    out = {k: torch.empty(plan.size, dtype=torch.uint8, device=dev) for k in "pkm"}
    conf = {k: torch.empty(plan.size, dtype=torch.float32, device=dev) for k in "km"}
    unc = torch.zeros(1, dtype=torch.int32, device=dev)
    today = {}

    def aug_t():
        today["p"] = plan.mean_probabilities(lgs, unc)
        today["r"] = today["p"].max(1)

    legs = dict(p=lambda: plan.class_map(lgs, out["p"], unc, one_pass=True), k=lambda: plan.class_map(lgs, out["k"], unc, one_pass=True, conf=conf["k"]),
                t=aug_t, m=lambda: plan.class_map(lgs, out["m"], unc, one_pass=False, conf=conf["m"]))
    results = {k: (lambda k=k: (out[k], conf.get(k))) for k in "pkm"}
    results["t"] = lambda: (inf.argmax_map(today["p"]), today["r"].values)
    measure(f"augmented, views 1.0 and 1.0 flipped of the 1080 x 1920 frame: {[p.n for p in plan.plans]} windows, {plan.size[1] * plan.size[2]} output pixels", legs, results)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
