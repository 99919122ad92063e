"""Timing of the calibration kernel (csrc/calibrate.hip, mmsa_eval_calibration) for profiles/calibration.txt.  Legs interleaved in ONE process, every
repetition timing each leg once (order rotated), `--inner` launches per timing between two events on the launch stream:
  (s) mmsa_eval_confusion_u8 alone -- the yardstick: its kernel is the parent's, launch-bound at this size (profiles/evaluate.txt), 2 bytes per pixel;
  (k) mmsa_eval_calibration on the same maps with the model's confidences, 15 bins (1 + 4 + 1 = 6 bytes per pixel);
  (u) the same launch with confidences uniform in [0, 1): every wave meets all 15 bins, the worst case of the bin-by-bin wave reduction.
Maps: the sizes of the evaluation profile -- two 1024 x 1024 maps and one 1080 x 1920 frame, 25 classes -- as class map and confidence map of a real
forward: the seeded tiny backbone (tests/configs.py 'tiny256') with a seeded 25-class SegformerHead, whole-image inference rescaled to the map size
(mmsa_slide_argmax_resized_conf).  Labels in 32 x 32 patches with 5 % ignored.  Legs (k) and (u) are checked against the numpy restatement
(tests/calibration_ref.py) before anything is timed."""
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
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.reps < 30:
        raise SystemExit("calibration_bench: at least 30 repetitions (medians and percentiles are reported)")
    if not torch.cuda.is_available():
        raise SystemExit("calibration_bench: no GPU (a timing needs one)")
    import mmsa
    import mmsa.inference as inf
    from mmsa.evaluate import LabelPrep, calibration, confusion, ece_of, reliability_of
    from tests import calibration_ref as CR
    from tests.configs import CONFIGS, HEAD_CONFIGS, make_input
    from tests.weights import seeded_state_dict
    dev = torch.device("cuda", 0)
    C, K = 25, a.bins
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
    say(f"device {torch.cuda.get_device_name(0)}; reps {a.reps}, {a.inner} launches per timing; times in microseconds per launch; {C} classes, {K} bins")
    for name, B, H, W in (("2 x 1024 x 1024", 2, 1024, 1024), ("1 x 1080 x 1920", 1, 1080, 1920)):
        g = torch.Generator().manual_seed(5)
        x = make_input(cfg, batch=B, seed=17).to(dev)
        pred, conf = inf.whole_class_map(m, h, x, ori_shape=(H, W), confidence=True)
        lab = patch_labels(B, H, W, C, g).to(dev)
        uni = torch.rand(B, H, W, generator=g).to(dev)
        lp = LabelPrep(C)
        cnt = torch.zeros(B, C + 1, C + 1, dtype=torch.int64, device=dev)
        cal = {k: torch.zeros(B, 3, K, dtype=torch.int64, device=dev) for k in "ku"}
        legs = dict(s=lambda: confusion(pred, lab, lp, counts=cnt), k=lambda: calibration(pred, conf, lab, lp, cal=cal["k"]),
                    u=lambda: calibration(pred, uni, lab, lp, cal=cal["u"]))
        for k in legs:          # warm-up, and the bins are the restatement's
            legs[k]()
        torch.cuda.synchronize()
        p_h, l_h = pred.cpu().numpy(), lab.cpu().numpy()
        for k, c in (("k", conf), ("u", uni)):
            assert np.array_equal(cal[k].cpu().numpy(), CR.bins_of_batch(p_h, c.cpu().numpy(), l_h, C, K)), k
        first = cal["k"].cpu().numpy().sum(0)
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
        say(f"{name}: {B * H * W} pixels; bins equal the numpy restatement bit for bit; the model's confidences fill {int((first[0] > 0).sum())} of {K} bins, "
            f"{100.0 * first[0].max() / max(first[0].sum(), 1):.1f} % of the pixels in the fullest; ECE {100 * ece_of(first):.2f} %, mean confidence "
            f"{100 * np.nansum(reliability_of(first)['confidence'] * first[0]) / max(first[0].sum(), 1):.2f} %")
        med, spread = {}, {}
        for k, what, bpp in (("s", "eval_confusion_u8 alone (yardstick)", 2), ("k", "eval_calibration, model confidences", 6),
                             ("u", "eval_calibration, uniform confidences", 6)):
            t = np.array(times[k])
            med[k], spread[k] = float(np.median(t)), float(np.percentile(t, 90) - np.percentile(t, 10))
            say(f"  ({k}) {what:38s} median {med[k]:8.2f}   p10 {np.percentile(t, 10):8.2f}   p90 {np.percentile(t, 90):8.2f}   spread {spread[k]:6.2f}   "
                f"{bpp} B/pixel = {bpp * B * H * W} bytes -> {bpp * B * H * W / (med[k] * 1e-6) / 1e12:.3f} TB/s (launch included)")
        say(f"  (k) - (s) = {med['k'] - med['s']:.2f} us, (u) - (s) = {med['u'] - med['s']:.2f} us; spread of the yardstick (p90 - p10) {spread['s']:.2f} us")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
