"""Timing of the boundary counts for profiles/boundary.txt.  Legs interleaved in ONE process, every repetition timing each leg once (order rotated), `--inner`
calls per timing between two events on the launch stream, all on the same stored maps:
  (e)        mmsa_eval_confusion_u8 on the same maps: the floor -- the same 2 bytes per pixel without the stencil;
  (b1) .. (b32)  mmsa_eval_boundary_u8 at radius 1, 3, 8, 32;
  (t1) .. (t32)  what a user has without it, in device torch: max_pool2d (separable: a row pool, then a column pool, stride 1, -inf padding) of +x and -x
             on the float class map and on the LUT-ed label map for "window min != window max", then one bincount over zone * (C + 1)^2 + cell on the
             pixels whose label is not ignored.  (The one-hot canvases [B, C, H, W] a dilation per class would need are not timed.)
Workloads, 25 classes: two 1024 x 1024 maps and the 1080 x 1920 frame.  The class map is the argmax launch's on seeded head-resolution logits (smooth blobs, as
a model's map); the label map is that map with its contours moved by (3, 2) pixels, 16 x 16 patches of other classes on 4 % of the blocks and ignored patches
on 3 %.  Every (b) result is checked first against the (t) result of its radius, cell for cell, and its zone sum against (e).  No threshold: the medians and
p10 .. p90 spreads are the record; the LDS bytes and the workgroups per CU they allow (160 KiB of LDS per CU) are printed per radius."""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "multimodal-sam-adapter_amd"))
sys.path.insert(0, ROOT)

RADII = (1, 3, 8, 32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--inner", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("boundary_bench: no GPU (a timing needs one)")
    import mmsa
    import mmsa.inference as inf
    from mmsa.evaluate import LabelPrep, boundary_launch_shape
    import torch.nn.functional as F
    dev = torch.device("cuda", 0)
    lines = []
    C = 25
    nb = (C + 1) * (C + 1)

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    def logits(n, g):
        coarse = torch.randn(n, C, 32, 32, generator=g)
        return (F.interpolate(coarse, size=(256, 256), mode="bilinear") + 0.05 * torch.randn(n, C, 256, 256, generator=g)).to(dev)

    def near(x, d):
        """bool [B, H, W]: the (2 d + 1)^2 window of the float map x is not uniform; max_pool2d pads with -inf, so pixels outside the image do not exist."""
        x = x.unsqueeze(1)

        def pool(v):
            return F.max_pool2d(F.max_pool2d(v, (1, 2 * d + 1), 1, (0, d)), (2 * d + 1, 1), 1, (d, 0))
        return ((pool(x) != x) | (pool(-x) != -x)).squeeze(1)

    def torch_counts(pred, lab, lut, d):
        L = lut[lab.long()]
        Lc = torch.where(L == 255, L, L.clamp(max=C))
        P = pred.clamp(max=C)
        zone = 2 * near(Lc.float(), d).long() + near(P.float(), d).long()
        idx = (zone * nb + Lc.clamp(max=C).long() * (C + 1) + P.long()) + torch.arange(pred.shape[0], device=pred.device).view(-1, 1, 1) * (4 * nb)
        return torch.bincount(idx[L != 255], minlength=pred.shape[0] * 4 * nb).view(pred.shape[0], 4, C + 1, C + 1)

    say(f"device {torch.cuda.get_device_name(0)}; reps {a.reps}, {a.inner} calls per timing; times in microseconds per call; {C} classes")
    say("launch shape per radius (mmsa.evaluate.boundary_launch_shape): " + "; ".join(
        f"d = {d}: tile {boundary_launch_shape(C, d)[3]} x {boundary_launch_shape(C, d)[2]}, {boundary_launch_shape(C, d)[0]} zone group(s), "
        f"{boundary_launch_shape(C, d)[1]} B of LDS -> at most {163840 // boundary_launch_shape(C, d)[1]} workgroups per CU by LDS" for d in RADII))
    g = torch.Generator().manual_seed(7)
    lp = LabelPrep(C)
    for name, plan in (("two 1024 x 1024 maps", inf.MapPlan.whole(2, 1024, 1024)),
                       ("1080 x 1920 frame, six windows", inf.MapPlan.slide(1, 1080, 1920, (1024, 1024), (640, 640)))):
        lg = logits(plan.n, g)
        B, H, W = plan.B, plan.Ho, plan.Wo
        pred = torch.empty(B, H, W, dtype=torch.uint8, device=dev)
        unc = torch.zeros(1, dtype=torch.int32, device=dev)
        plan.class_map(lg, pred, unc)
        assert int(unc.item()) == 0
        del lg
        lab = torch.roll(pred, (3, 2), (1, 2)).cpu()
        r = torch.rand(B, (H + 15) // 16, (W + 15) // 16, generator=g).repeat_interleave(16, 1).repeat_interleave(16, 2)[:, :H, :W]
        other = torch.randint(0, C, (B, (H + 15) // 16, (W + 15) // 16), generator=g, dtype=torch.uint8).repeat_interleave(16, 1).repeat_interleave(16, 2)[:, :H, :W]
        lab = torch.where(r < 0.04, other, lab)
        lab[(r >= 0.04) & (r < 0.07)] = 255
        lab = lab.contiguous().to(dev)
        lut = torch.from_numpy(lp.lut).to(dev)
        npx = B * H * W
        bufs = {d: torch.zeros(B, 4, C + 1, C + 1, dtype=torch.int64, device=dev) for d in RADII}
        ebuf = torch.zeros(B, C + 1, C + 1, dtype=torch.int64, device=dev)
        legs = dict(e=lambda: mmsa.confusion(pred, lab, lp, counts=ebuf))
        what = dict(e="mmsa_eval_confusion_u8 (the floor)")
        for d in RADII:
            legs[f"b{d}"] = lambda d=d: mmsa.boundary_counts(pred, lab, lp, d, counts=bufs[d])
            what[f"b{d}"] = f"mmsa_eval_boundary_u8, radius {d}"
        for d in RADII:
            legs[f"t{d}"] = lambda d=d: torch_counts(pred, lab, lut, d)
            what[f"t{d}"] = f"torch: separable max_pool2d x 4 + bincount, radius {d}"
        for _ in range(2):
            for k in legs:
                legs[k]()
        torch.cuda.synchronize()
        e = mmsa.confusion(pred, lab, lp)
        band = {}
        for d in RADII:
            got = mmsa.boundary_counts(pred, lab, lp, d)
            assert torch.equal(got, torch_counts(pred, lab, lut, d)), f"{name}: radius {d}: the kernel's counts are not the torch path's"
            assert torch.equal(got.sum(1), e), f"{name}: radius {d}: the zone sum is not the confusion matrix"
            band[d] = float(got[:, 2:].sum()) / float(got.sum())
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
        say(f"{name}: {npx} pixels; every (b) equals its (t) cell for cell and sums to (e) over the zones; share of the counted pixels in the label band: "
            + ", ".join(f"d = {d}: {band[d]:.3f}" for d in RADII))
        med = {}
        for k in legs:
            t = np.array(times[k])
            med[k] = float(np.median(t))
            say(f"  ({k:3s}) {what[k]:58s} median {med[k]:10.2f}   p10 {np.percentile(t, 10):10.2f}   p90 {np.percentile(t, 90):10.2f}"
                f"   {2.0 * npx / med[k] * 1e-6:7.3f} TB/s on 2 B per pixel")
        spread = float(np.percentile(times["e"], 90) - np.percentile(times["e"], 10))
        say("  " + "; ".join(f"(b{d}) - (e) = {med[f'b{d}'] - med['e']:+.2f}, (t{d}) / (b{d}) = {med[f't{d}'] / med[f'b{d}']:.1f} x" for d in RADII)
            + f"; p10 .. p90 of (e) spans {spread:.2f}")
        del pred, lab, bufs
        torch.cuda.empty_cache()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
