"""Measurements of mmsa.preprocess on the GPU box -> profiles/preprocess.txt (or --out):

1. kernel time and achieved bytes/s of mmsa_preprocess_nhwc (1024 x 1024 whole frame) and mmsa_preprocess_crops (1080 x 1920 frame, the six
   1024 x 1024 windows of crop 1024 / stride 640) per source dtype pair, against the yardstick mmsa_crop_batch_nchw cutting the same windows from
   a float32 NCHW frame (48 B per output pixel).  Compulsory bytes of the new kernels = source bytes read + 24 B per output pixel.  Every figure
   is the median over --reps repetitions (>= 20), the candidates INTERLEAVED within each repetition; a repetition times --inner launches between
   two device events.  The spread given is (max - min) / median of the yardstick over the repetitions of the same job.
2. frames/s of a SlideRunner frame with HOST input: the parent path (numpy normalise on the host, float32 upload, SlideRunner) against
   FrameFeeder + SlideRunner(preprocess=), ViT-L 1024, one 1080 x 1920 frame per step; the host normalise alone is timed as well.

Usage: python tools/preprocess_bench.py [--reps 30] [--inner 10] [--frames 12] [--skip-model] [--out profiles/preprocess.txt]"""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "multimodal-sam-adapter_amd"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import mmsa  # noqa: E402
import mmsa.inference as inf  # noqa: E402
from mmsa.preprocess import FrameFeeder, Preprocess  # noqa: E402
from tests import preprocess_ref as PR  # noqa: E402
from tests.configs import CONFIGS, HEAD_CONFIGS  # noqa: E402

DEV = torch.device("cuda:0")
DT = {"u8": np.uint8, "f32": np.float32}


def timed(fn, inner):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(inner):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / inner       # us per launch


def interleaved(cands, reps, inner):
    for fn in cands.values():
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    ts = {k: [] for k in cands}
    for _ in range(reps):
        for k, fn in cands.items():
            ts[k].append(timed(fn, inner))
    return ts


def line(name, us, nbytes, ts):
    return f"  {name:<34s} {us:9.1f} us  {nbytes / 1e6:8.1f} MB  {nbytes / us / 1e6:6.2f} TB/s   (min {min(ts):.1f}, max {max(ts):.1f} us)"


def sources(g, shape, kind):
    if kind == "u8":
        return g.integers(0, 256, shape, dtype=np.uint8)
    return (g.random(shape) * 255).astype(np.float32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--inner", type=int, default=10)
    ap.add_argument("--frames", type=int, default=12)
    ap.add_argument("--skip-model", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "preprocess.txt"))
    args = ap.parse_args()
    assert args.reps >= 20
    cfg = PR.load_cfgs()["muses_rgb_lidar"]
    pp = Preprocess.from_pipeline(PR.pipeline_of(cfg))
    g = np.random.default_rng(1)
    rows = [f"tools/preprocess_bench.py --reps {args.reps} --inner {args.inner} --frames {args.frames}   ({torch.cuda.get_device_name(0)}, kernel sources {digest()})",
            "settings: MUSES RGB+LiDAR (Normalize_multimodal_Muses, norm_by_max, to_rgb [True, False]); medians over the repetitions, candidates interleaved", ""]

    # ---- 1a. windows of a 1080 x 1920 frame ----
    Hs, Ws, crop = 1080, 1920, (1024, 1024)
    jobs = [(0, box) for box in inf.crop_boxes(Hs, Ws, crop, (640, 640))]
    n = len(jobs)
    opix = n * crop[0] * crop[1]
    src = {k: torch.from_numpy(sources(g, (1, Hs, Ws, 3), k)).to(DEV) for k in DT}
    frame32 = pp(src["u8"], src["u8"])
    out = torch.empty(n, 6, *crop, device=DEV)
    cands = {"yardstick crop_batch_nchw (f32 NCHW)": lambda: inf._crops(frame32, jobs, crop, out=out)}
    nbytes = {"yardstick crop_batch_nchw (f32 NCHW)": 48 * opix}
    covered = sum((y2 - y1) * (x2 - x1) for _, (y1, x1, y2, x2) in jobs)       # source pixels read, counted once per window that covers them
    for a, b in (("u8", "u8"), ("u8", "f32"), ("f32", "f32")):
        name = f"preprocess_crops {a}/{b}"
        cands[name] = (lambda a=a, b=b: pp.crops(src[a], src[b], jobs, crop, out=out))
        nbytes[name] = covered * 3 * (np.dtype(DT[a]).itemsize + np.dtype(DT[b]).itemsize) + 24 * opix
    ts = interleaved(cands, args.reps, args.inner)
    med = {k: statistics.median(v) for k, v in ts.items()}
    yk = "yardstick crop_batch_nchw (f32 NCHW)"
    spread = (max(ts[yk]) - min(ts[yk])) / med[yk]
    rows.append(f"1a. slide: 1080 x 1920 frame -> {n} windows of 1024 x 1024 (us per launch; bytes = compulsory traffic, every window's reads counted)")
    rows += [line(k, med[k], nbytes[k], ts[k]) for k in cands]
    rows.append("  (back-to-back repetitions on the same buffers: rates above the HBM peak mean part of the traffic is served by the caches, for the yardstick and the new kernels alike -- compare times)")
    rows.append(f"  yardstick run-to-run spread (max - min) / median: {100 * spread:.1f} %")
    for k in cands:
        if k != yk:
            verdict = "no longer than the yardstick" if med[k] <= med[yk] * (1 + spread) else "SLOWER than the yardstick"
            rows.append(f"  {k}: {med[k] / med[yk]:.2f} x the yardstick's time -> {verdict}")
    rows.append("")

    # ---- 1b. whole 1024 x 1024 frame ----
    Hs = Ws = 1024
    src = {k: torch.from_numpy(sources(g, (1, Hs, Ws, 3), k)).to(DEV) for k in DT}
    whole = torch.empty(1, 6, Hs, Ws, device=DEV)
    cands, nbytes = {}, {}
    for a, b in (("u8", "u8"), ("u8", "f32"), ("f32", "f32")):
        name = f"preprocess_nhwc {a}/{b}"
        cands[name] = (lambda a=a, b=b: pp(src[a], src[b], out=whole))
        nbytes[name] = Hs * Ws * (3 * (np.dtype(DT[a]).itemsize + np.dtype(DT[b]).itemsize) + 24)
    ts = interleaved(cands, args.reps, args.inner)
    rows.append("1b. whole: 1024 x 1024 frame -> [1, 6, 1024, 1024] (no yardstick kernel exists for this form: the parent takes the normalised tensor)")
    rows += [line(k, statistics.median(ts[k]), nbytes[k], ts[k]) for k in cands]
    wm = [statistics.median(ts[k]) for k in cands]
    if max(wm) <= 1.1 * min(wm):
        rows.append("  (the same time for 31 to 50 MB: at this size the launch is not bandwidth-bound -- what bounds it, the eager enqueue rate of the caller or the "
                    "kernel's 1024 one-row workgroups, is not separated here)")
    rows.append("")

    # ---- 2. a SlideRunner frame with host input ----
    if not args.skip_model:
        rows += frames_per_s(pp, cfg, g, args.frames)
    text = "\n".join(rows) + "\n"
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    open(args.out, "w").write(text)


def digest():
    sys.path.insert(0, os.path.join(ROOT, "multimodal-sam-adapter_amd"))
    import build as _b
    return _b.source_digest()[:12]


def frames_per_s(pp, cfg, g, frames):
    from tests.weights import seeded_state_dict
    m = mmsa.build_backbone(dict(type="SAMAdapterbimodalMixModNewInTwinConvNEW", **CONFIGS["vitl1024"]["kwargs"]))
    m.load_state_dict(seeded_state_dict(m, seed=CONFIGS["vitl1024"]["seed"]))
    h = mmsa.build_head(dict(type="SegformerHead", **HEAD_CONFIGS["head_vitl"]["kwargs"])).to(DEV)
    h.load_state_dict(seeded_state_dict(h, seed=HEAD_CONFIGS["head_vitl"]["seed"]))
    shape = (1, 1080, 1920, 3)
    rgb = g.integers(0, 256, shape, dtype=np.uint8)
    aux = (g.integers(0, 256, shape) * (g.random(shape) < 0.05)).astype(np.uint8)
    norm = lambda: PR.normalize_ref(rgb, aux, cfg["mean"], cfg["std"], cfg["to_rgb"], cfg["modalities_name"], cfg["norm_by_max"], "muses")

    # parent path: numpy normalise -> float32 upload (pinned, as a careful caller would) -> SlideRunner on its static float frame
    frame = torch.empty(1, 6, 1080, 1920, device=DEV)
    pinned = torch.empty(1, 6, 1080, 1920).pin_memory()
    sr_ref = inf.SlideRunner(m, h, frame, (1024, 1024), (640, 640), chains=2)

    def parent_step():
        pinned.numpy()[:] = norm()
        frame.copy_(pinned, non_blocking=True)
        return sr_ref.run().outputs()[0]

    sr_raw = inf.SlideRunner(m, h, (torch.from_numpy(rgb).to(DEV), torch.from_numpy(aux).to(DEV)), (1024, 1024), (640, 640), chains=2, preprocess=pp)
    feeder = FrameFeeder(pp, shape[:3], slots=2)

    def raw_step():
        return sr_raw.run(frame=feeder.feed(rgb, aux)).outputs()[0]

    def device_only():
        return sr_raw.run().outputs()[0]

    res = {}
    for name, step in (("parent: numpy normalise + f32 upload + SlideRunner", parent_step), ("FrameFeeder + SlideRunner(preprocess=)", raw_step),
                       ("device only (resident raw frame)", device_only)):
        for _ in range(2):
            cm = step()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(frames):
            cm = step()
        torch.cuda.synchronize()
        res[name] = ((time.perf_counter() - t0) / frames, cm.clone())
    assert torch.equal(res["parent: numpy normalise + f32 upload + SlideRunner"][1], res["FrameFeeder + SlideRunner(preprocess=)"][1]), "the two paths disagree on the class map"
    t0 = time.perf_counter()
    for _ in range(3):
        norm()
    t_norm = (time.perf_counter() - t0) / 3
    rows = [f"2. SlideRunner, ViT-L 1024, one 1080 x 1920 frame per step from HOST arrays (uint8 RGB + uint8 LiDAR map), {frames} frames, same class map on both paths"]
    for name, (dt, _) in res.items():
        rows.append(f"  {name:<52s} {dt * 1e3:8.1f} ms/frame  {1 / dt:6.2f} frames/s")
    dev_t = res["device only (resident raw frame)"][0]
    rows.append(f"  host numpy normalise alone (measured, {os.cpu_count()} CPUs visible): {t_norm * 1e3:.1f} ms/frame; upload sizes: 49.8 MB float32 vs 12.4 MB uint8")
    for name in list(res)[:2]:
        dt = res[name][0]
        rows.append(f"  {name}: {'device-bound (within 5 % of the device-only time)' if dt <= 1.05 * dev_t else f'host-bound ({dt / dev_t:.2f} x the device-only time)'}")
    return rows


if __name__ == "__main__":
    main()
