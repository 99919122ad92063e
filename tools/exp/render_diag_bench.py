"""Timing of the diagnostic pictures for profiles/render_diag.txt.  Legs interleaved in ONE process, every repetition timing each leg once (order rotated),
`--inner` calls per timing between two events on the launch stream, all on the same stored maps and the same raw uint8 source:
  (y)            the yardstick: mmsa_render_u8, `Renderer.__call__` over the raw frame -- the launch that existed; the new code is never its own yardstick;
  (L) (E) (H) (A)  labels / errors / heat / abstained, each ONE launch;
  (a2)           what (A) replaces: mmsa.abstain, then `__call__` on its map (two launches, the map written and read back);
  (b1) .. (b32)  band at radius 1, 3, 8, 32 (where="both": both maps staged, both passes made);
  (e1) .. (e32)  mmsa_eval_boundary_u8 on the same maps: the band's integer work without the picture;
  (t1) .. (t32)  the band picture in device torch: separable max_pool2d of +x and -x on both float maps, a compare, a palette gather, the float64 blend and
                 torch.where.  Checked to be the (b) picture byte for byte before anything is timed.
Workloads, 25 classes: two 1024 x 1024 maps and one 1080 x 1920 frame.  Maps as in tools/exp/boundary_bench.py (the argmax of smooth seeded logits; the label
map is that map with its contours moved, patches of other classes and ignored patches); the confidence is uniform noise.
Two tables per workload: the eager call as a user makes it (Python, checks and the launch: at these sizes mostly the host), and the device time per call from
a replayed graph of `--graph` calls (every leg but the torch ones, which allocate).  Bytes per pixel are the compulsory
ones (maps read once, the source read, the picture written; the band's halo re-reads are not counted).  No threshold: medians and p10 .. p90 are the record."""
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
    ap.add_argument("--graph", type=int, default=20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("render_diag_bench: no GPU (a timing needs one)")
    import mmsa
    import mmsa.inference as inf
    from mmsa.evaluate import LabelPrep
    from mmsa.render import HEAT, Renderer
    import torch.nn.functional as F
    dev = torch.device("cuda", 0)
    lines = []
    C, OP = 25, 0.5

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    def logits(n, g):
        coarse = torch.randn(n, C, 32, 32, generator=g)
        return (F.interpolate(coarse, size=(256, 256), mode="bilinear") + 0.05 * torch.randn(n, C, 256, 256, generator=g)).to(dev)

    def near(x, d):
        x = x.unsqueeze(1)

        def pool(v):
            return F.max_pool2d(F.max_pool2d(v, (1, 2 * d + 1), 1, (0, d)), (2 * d + 1, 1), 1, (d, 0))
        return ((pool(x) != x) | (pool(-x) != -x)).squeeze(1)

    g = torch.Generator().manual_seed(7)
    palette = np.array([((37 * i + 11) % 256, (91 * i + 5) % 256, (53 * i + 200) % 256) for i in range(C)])
    pal_t = torch.zeros(256, 3, dtype=torch.uint8)
    pal_t[:C] = torch.from_numpy(palette[:, ::-1].copy()).to(torch.uint8)          # bgr=True: the picture's channel order
    pal_t = pal_t.to(dev)
    white = torch.full((3,), 255, dtype=torch.uint8, device=dev)
    lp = LabelPrep(C)
    lut = torch.from_numpy(lp.lut).to(dev)
    r = Renderer(palette, opacity=OP)

    def torch_band(pred, lab, src, d):
        L = lut[lab.long()]
        Lc = torch.where(L == 255, L, L.clamp(max=C))
        P = pred.clamp(max=C)
        marked = (near(Lc.float(), d) | near(P.float(), d)) & (L != 255)
        blend = (src.double() * (1 - OP) + pal_t[P.long()].double() * OP).to(torch.uint8)
        return torch.where(marked.unsqueeze(-1), white, blend)

    say(f"device {torch.cuda.get_device_name(0)}; reps {a.reps}, {a.inner} calls per timing; times in microseconds per call; {C} classes; opacity {OP}; raw uint8 source")
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
        rr = torch.rand(B, (H + 15) // 16, (W + 15) // 16, generator=g).repeat_interleave(16, 1).repeat_interleave(16, 2)[:, :H, :W]
        other = torch.randint(0, C, (B, (H + 15) // 16, (W + 15) // 16), generator=g, dtype=torch.uint8).repeat_interleave(16, 1).repeat_interleave(16, 2)[:, :H, :W]
        lab = torch.where(rr < 0.04, other, lab)
        lab[(rr >= 0.04) & (rr < 0.07)] = 255
        lab = lab.contiguous().to(dev)
        conf = torch.rand(B, H, W, generator=g).to(dev)
        src = torch.randint(0, 256, (B, H, W, 3), generator=g, dtype=torch.uint8).to(dev)
        npx = B * H * W
        out = torch.empty(B, H, W, 3, dtype=torch.uint8, device=dev)
        amap = torch.empty_like(pred)
        bufs = {d: torch.zeros(B, 4, C + 1, C + 1, dtype=torch.int64, device=dev) for d in RADII}

        def two_launches():
            mmsa.abstain(pred, conf, 15, 6, out=amap)
            r(amap, src, out=out)

        legs = dict(y=lambda: r(pred, src, out=out), L=lambda: r.labels(lab, lp, source=src, out=out), E=lambda: r.errors(pred, lab, lp, source=src, out=out),
                    H=lambda: r.heat(conf, HEAT, source=src, out=out), A=lambda: r.abstained(pred, conf, 15, min_bin=6, source=src, out=out), a2=two_launches)
        what = dict(y="mmsa_render_u8 over the raw frame (the yardstick)", L="labels", E="errors", H="heat, 256-entry colormap", A="abstained, 15 bins",
                    a2="mmsa.abstain + __call__ (what (A) replaces)")
        nbytes = dict(y=7, L=7, E=8, H=10, A=11, a2=11)
        for d in RADII:
            legs[f"b{d}"] = lambda d=d: r.band(pred, lab, lp, radius=d, where="both", source=src, out=out)
            what[f"b{d}"] = f"band, radius {d}, both maps"
            nbytes[f"b{d}"] = 8
        for d in RADII:
            legs[f"e{d}"] = lambda d=d: mmsa.boundary_counts(pred, lab, lp, d, counts=bufs[d])
            what[f"e{d}"] = f"mmsa_eval_boundary_u8, radius {d} (no picture)"
            nbytes[f"e{d}"] = 2
        for d in RADII:
            legs[f"t{d}"] = lambda d=d: torch_band(pred, lab, src, d)
            what[f"t{d}"] = f"torch: max_pool2d x 8, compare, gather, blend, where; radius {d}"
            nbytes[f"t{d}"] = 8
        for d in RADII:
            assert torch.equal(r.band(pred, lab, lp, radius=d, where="both", source=src), torch_band(pred, lab, src, d)), f"{name}: radius {d}: (b) is not (t)"
        assert torch.equal(r.abstained(pred, conf, 15, min_bin=6, source=src, colour=(0, 0, 0), mark_opacity=OP), r(mmsa.abstain(pred, conf, 15, 6), src))
        for _ in range(2):
            for k in legs:
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
        # device time: `--graph` calls of a leg captured into one graph and replayed (the launches back to back, no host work between them); the legs
        # that allocate (torch) are left out.  Interleaved like the eager timings.
        graphs, gtimes = {}, {}
        side = torch.cuda.Stream()
        for k in legs:
            if k.startswith("t"):
                continue
            gr = torch.cuda.CUDAGraph()
            with torch.cuda.graph(gr, stream=side):
                for _ in range(a.graph):
                    legs[k]()
            graphs[k], gtimes[k] = gr, []
            gr.replay()
        torch.cuda.synchronize()
        gorder = list(graphs)
        for rep in range(a.reps):
            for k in gorder[rep % len(gorder):] + gorder[:rep % len(gorder)]:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                graphs[k].replay()
                e1.record()
                e1.synchronize()
                gtimes[k].append(e0.elapsed_time(e1) * 1e3 / a.graph)
        say()
        say(f"{name}: {npx} pixels; every (b) equals its (t) byte for byte; (A) at mark_opacity = opacity equals (a2)'s picture")
        med = {}
        for k in legs:
            t = np.array(times[k])
            med[k] = float(np.median(t))
            say(f"  ({k:3s}) {what[k]:70s} median {med[k]:10.2f}   p10 {np.percentile(t, 10):10.2f}   p90 {np.percentile(t, 90):10.2f}"
                f"   {nbytes[k]:2d} B per pixel {nbytes[k] * npx / med[k] * 1e-6:7.3f} TB/s   {med[k] / med['y']:6.2f} x (y)")
        spread = float(np.percentile(times["y"], 90) - np.percentile(times["y"], 10))
        say(f"  p10 .. p90 of (y) spans {spread:.2f}; (a2) / (A) = {med['a2'] / med['A']:.2f} x; "
            + "; ".join(f"(b{d}) / (e{d}) = {med[f'b{d}'] / med[f'e{d}']:.2f} x, (t{d}) / (b{d}) = {med[f't{d}'] / med[f'b{d}']:.1f} x" for d in RADII))
        say(f"  device time per call, a graph of {a.graph} calls replayed (no host work between the launches):")
        gmed = {}
        for k in graphs:
            t = np.array(gtimes[k])
            gmed[k] = float(np.median(t))
            say(f"  ({k:3s}) {what[k]:70s} median {gmed[k]:10.2f}   p10 {np.percentile(t, 10):10.2f}   p90 {np.percentile(t, 90):10.2f}"
                f"   {nbytes[k]:2d} B per pixel {nbytes[k] * npx / gmed[k] * 1e-6:7.3f} TB/s   {gmed[k] / gmed['y']:6.2f} x (y)")
        gspread = float(np.percentile(gtimes["y"], 90) - np.percentile(gtimes["y"], 10))
        say(f"  p10 .. p90 of (y) spans {gspread:.2f}; (a2) / (A) = {gmed['a2'] / gmed['A']:.2f} x; "
            + "; ".join(f"(b{d}) / (e{d}) = {gmed[f'b{d}'] / gmed[f'e{d}']:.2f} x" for d in RADII))
        del graphs, pred, lab, conf, src, out, bufs
        torch.cuda.empty_cache()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
