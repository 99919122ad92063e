"""Timing of the selective-evaluation kernel (csrc/selective.hip, mmsa_eval_selective) and of mmsa_abstain_u8 for profiles/selective.txt.  Legs interleaved
in ONE process, every repetition timing each leg once (order rotated), `--inner` launches per timing between two events on the launch stream:
  (s) mmsa_eval_confusion_u8 alone -- the first yardstick: its kernel is the parent's (profiles/selective_isa.txt), 2 bytes per pixel;
  (k) mmsa_eval_calibration on the same maps with the model's confidences -- the second yardstick, its kernel the parent's too, 6 bytes per pixel;
  (v) mmsa_eval_selective on the same maps with the model's confidences, 25 classes and 15 bins: one bin group, 6 bytes per pixel;
  (u) the same launch with confidences uniform in [0, 1): no two neighbouring pixels share a cell, the worst case of the same-cell merging;
  (g) the same maps counted with 63 classes and 16 bins: six bin groups, each of which reads the 6 bytes per pixel (36 in all);
  (a) mmsa_abstain_u8 at min_bin = bins - 1 on the model's confidences: 1 + 4 bytes read and 1 written per pixel.
Maps: the sizes of the evaluation profile -- two 1024 x 1024 maps and one 1080 x 1920 frame, 25 classes -- as class map and confidence map of a real
forward: the seeded tiny backbone (tests/configs.py 'tiny256') with a seeded 25-class SegformerHead, whole-image inference rescaled to the map size.
Labels in 32 x 32 patches with 5 % ignored.  Legs (v), (u), (g) and (a) are checked against the numpy restatement (tests/selective_ref.py) before
anything is timed.  `--tag` names the build in the output: the same-cell merging forms are builds of their own (tools/build_variant.sh with -DSEL_MERGE,
loaded through MMSA_LIB), each timed against the yardsticks of its own run."""
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
    ap.add_argument("--reps", type=int, default=40)
    ap.add_argument("--inner", type=int, default=20)
    ap.add_argument("--bins", type=int, default=15)
    ap.add_argument("--tag", default="the library as built (SEL_MERGE and SEL_CHUNK of csrc/selective.hip)")
    ap.add_argument("--out", default=None)
    ap.add_argument("--append", action="store_true")
    a = ap.parse_args()
    if a.reps < 30:
        raise SystemExit("selective_bench: at least 30 repetitions (medians and percentiles are reported)")
    if not torch.cuda.is_available():
        raise SystemExit("selective_bench: no GPU (a timing needs one)")
    import mmsa
    import mmsa.inference as inf
    from mmsa.evaluate import LabelPrep, abstain, calibration, confusion, selective, selective_metrics_of
    from tests import selective_ref as SR
    from tests.configs import CONFIGS, HEAD_CONFIGS, make_input
    from tests.weights import seeded_state_dict
    dev = torch.device("cuda", 0)
    C, K, C2, K2 = 25, a.bins, 63, 16
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    cfg, hcfg = CONFIGS["tiny256"], HEAD_CONFIGS["head_tiny"]
    m = mmsa.build_backbone(dict(type="SAMAdapterbimodalMixModNewInTwinConvNEW", **cfg["kwargs"]))
    m.load_state_dict(seeded_state_dict(m, seed=cfg["seed"]))
    h = mmsa.build_head(dict(type="SegformerHead", **dict(hcfg["kwargs"], num_classes=C)))
    h.load_state_dict(seeded_state_dict(h, seed=hcfg["seed"]))
    h = h.to(dev)
    say(f"build: {a.tag}")
    say(f"device {torch.cuda.get_device_name(0)}; reps {a.reps}, {a.inner} launches per timing; times in microseconds per launch; {C} classes, {K} bins")
    for name, B, H, W in (("2 x 1024 x 1024", 2, 1024, 1024), ("1 x 1080 x 1920", 1, 1080, 1920)):
        g = torch.Generator().manual_seed(5)
        x = make_input(cfg, batch=B, seed=17).to(dev)
        pred, conf = inf.whole_class_map(m, h, x, ori_shape=(H, W), confidence=True)
        lab = patch_labels(B, H, W, C, g).to(dev)
        uni = torch.rand(B, H, W, generator=g).to(dev)
        lp, lp2 = LabelPrep(C), LabelPrep(C2)
        cnt = torch.zeros(B, C + 1, C + 1, dtype=torch.int64, device=dev)
        cal = torch.zeros(B, 3, K, dtype=torch.int64, device=dev)
        sel = {k: torch.zeros(B, K, C + 1, C + 1, dtype=torch.int64, device=dev) for k in "vu"}
        sel["g"] = torch.zeros(B, K2, C2 + 1, C2 + 1, dtype=torch.int64, device=dev)
        gated = torch.empty_like(pred)
        legs = dict(s=lambda: confusion(pred, lab, lp, counts=cnt), k=lambda: calibration(pred, conf, lab, lp, cal=cal),
                    v=lambda: selective(pred, conf, lab, lp, counts=sel["v"]), u=lambda: selective(pred, uni, lab, lp, counts=sel["u"]),
                    g=lambda: selective(pred, conf, lab, lp2, counts=sel["g"]), a=lambda: abstain(pred, conf, K, K - 1, out=gated))
        for k in legs:          # warm-up, and the counts are the restatement's
            legs[k]()
        torch.cuda.synchronize()
        p_h, l_h, c_h = pred.cpu().numpy(), lab.cpu().numpy(), conf.cpu().numpy()
        for k, c, cc, kk in (("v", c_h, C, K), ("u", uni.cpu().numpy(), C, K), ("g", c_h, C2, K2)):
            assert np.array_equal(sel[k].cpu().numpy(), SR.counts_of_batch(p_h, c, l_h, cc, kk)), k
        assert np.array_equal(gated.cpu().numpy(), SR.abstain_of(p_h, c_h, K, K - 1))
        first = sel["v"].cpu().numpy().sum(0)
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
        per_bin = first.sum((1, 2))
        curve = selective_metrics_of(first)
        say()
        say(f"{name}: {B * H * W} pixels; counts and thresholded map equal the numpy restatement bit for bit; the model's confidences fill "
            f"{int((per_bin > 0).sum())} of {K} bins, {100.0 * per_bin.max() / max(per_bin.sum(), 1):.1f} % of the pixels in the fullest, "
            f"{int((first > 0).sum())} of {first.size} cells in use; mIoU {100 * curve['mIoU'][0]:.2f} % at coverage 1, "
            f"{100 * curve['mIoU'][K - 1]:.2f} % at coverage {curve['coverage'][K - 1]:.3f} (the top bin alone)")
        med, spread = {}, {}
        for k, what, bpp in (("s", "eval_confusion_u8 alone (yardstick)", 2), ("k", "eval_calibration, model confidences (yardstick)", 6),
                             ("v", "eval_selective, model confidences", 6), ("u", "eval_selective, uniform confidences", 6),
                             ("g", f"eval_selective, {C2} classes x {K2} bins: 6 groups", 36), ("a", "abstain_u8, min_bin = bins - 1", 6)):
            t = np.array(times[k])
            med[k], spread[k] = float(np.median(t)), float(np.percentile(t, 90) - np.percentile(t, 10))
            say(f"  ({k}) {what:48s} median {med[k]:8.2f}   p10 {np.percentile(t, 10):8.2f}   p90 {np.percentile(t, 90):8.2f}   spread {spread[k]:6.2f}   "
                f"{bpp} B/pixel = {bpp * B * H * W} bytes -> {bpp * B * H * W / (med[k] * 1e-6) / 1e12:.3f} TB/s (launch included)")
        say(f"  (v) - (s) = {med['v'] - med['s']:.2f} us, (v) - (k) = {med['v'] - med['k']:.2f} us, (u) - (v) = {med['u'] - med['v']:.2f} us; spread of the "
            f"yardsticks (p90 - p10) {spread['s']:.2f} / {spread['k']:.2f} us")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "a" if a.append else "w").write("\n".join(lines) + "\n\n")


if __name__ == "__main__":
    main()
