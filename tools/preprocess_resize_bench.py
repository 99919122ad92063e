"""Measurement of the resizing launch of mmsa.preprocess on the GPU box -> profiles/preprocess_resize.txt (or --out).

Same method as tools/preprocess_bench.py: every figure is the median over --reps repetitions (>= 20), the candidates INTERLEAVED within each
repetition; a repetition times --inner launches between two device events; the spread is (max - min) / median of the yardstick.

Candidates, batch 2, uint8 RGB + uint8 auxiliary map, DELIVER's settings:
  yardstick   mmsa_preprocess_nhwc          1024 x 1024 frames -> [2, 6, 1024, 1024]   (what a caller who resized on the host launches)
  resize      mmsa_preprocess_resize_nhwc   1042 x 1042 frames -> [2, 6, 1024, 1024]   (DELIVER's native size; 8-bit fixed-point bilinear)
  and, for the record, the float32 path (uint8 + float32 sources) and the 1080 x 1920 -> 576 x 1024 geometry.
Compulsory bytes = source bytes read once + 24 B per output pixel.  Both write the same bytes; the resizing launch reads 3.6 % more.

Usage: python tools/preprocess_resize_bench.py [--reps 30] [--inner 10] [--out profiles/preprocess_resize.txt]"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "multimodal-sam-adapter_amd"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from mmsa.preprocess import Preprocess  # noqa: E402
from tests import preprocess_resize_ref as RR  # noqa: E402
from tools.preprocess_bench import DEV, digest, interleaved, line  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--inner", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "preprocess_resize.txt"))
    args = ap.parse_args()
    assert args.reps >= 20
    cfg = RR.load_cfgs()["deliver_rgb_lidar"]
    pp = Preprocess.from_pipeline(RR.pipeline_of(cfg), resize="device")
    g = np.random.default_rng(1)
    B = 2

    def u8(h, w):
        return torch.from_numpy(g.integers(0, 256, (B, h, w, 3), dtype=np.uint8)).to(DEV)

    def f32(h, w):
        return torch.from_numpy((g.random((B, h, w, 3)) * 255).astype(np.float32)).to(DEV)

    rows = [f"tools/preprocess_resize_bench.py --reps {args.reps} --inner {args.inner}   ({torch.cuda.get_device_name(0)}, kernel sources {digest()})",
            f"settings: DELIVER RGB+LiDAR (Normalize_multimodal, norm_by_max, to_rgb [True, True]), batch {B}; medians over the repetitions, candidates interleaved", ""]
    out = torch.empty(B, 6, 1024, 1024, device=DEV)
    a1024, b1024, a1042, b1042, c1042 = u8(1024, 1024), u8(1024, 1024), u8(1042, 1042), u8(1042, 1042), f32(1042, 1042)
    yk = "yardstick preprocess_nhwc u8/u8 1024^2"
    cands = {yk: lambda: pp(a1024, b1024, out=out),
             "preprocess_resize_nhwc u8/u8 1042^2": lambda: pp(a1042, b1042, out=out),
             "preprocess_resize_nhwc u8/f32 1042^2": lambda: pp(a1042, c1042, out=out)}
    opix = B * 1024 * 1024
    nbytes = {yk: B * 1024 * 1024 * 6 + 24 * opix, "preprocess_resize_nhwc u8/u8 1042^2": B * 1042 * 1042 * 6 + 24 * opix,
              "preprocess_resize_nhwc u8/f32 1042^2": B * 1042 * 1042 * 15 + 24 * opix}
    assert pp.canvas(1042, 1042) == (1024, 1024)
    ts = interleaved(cands, args.reps, args.inner)
    med = {k: statistics.median(v) for k, v in ts.items()}
    spread = (max(ts[yk]) - min(ts[yk])) / med[yk]
    rows.append(f"1. whole frame, batch {B} -> [{B}, 6, 1024, 1024] (us per launch; bytes = compulsory traffic)")
    rows += [line(k, med[k], nbytes[k], ts[k]) for k in cands]
    rows.append("  (back-to-back repetitions on the same buffers: part of the traffic is served by the caches, for the yardstick and the new kernel alike -- compare times)")
    rows.append(f"  yardstick run-to-run spread (max - min) / median: {100 * spread:.1f} %")
    for k in list(cands)[1:]:
        r = med[k] / med[yk]
        rows.append(f"  {k}: {r:.2f} x the yardstick's time -> {'within' if r <= 2 else 'BEYOND'} the 2 x accepted for a launch that reads two source rows per output row")
    rows.append("")

    # a strong downscale: the uint8 span (1920 pixels per workgroup) is staged, 576 x 1024 out
    out2 = torch.empty(B, 6, 576, 1024, device=DEV)
    m_rgb, m_aux = u8(1080, 1920), u8(1080, 1920)
    assert pp.canvas(1080, 1920) == (576, 1024)
    ts2 = interleaved({"preprocess_resize_nhwc u8/u8 1080x1920 -> 576x1024": lambda: pp(m_rgb, m_aux, out=out2)}, args.reps, args.inner)
    k2 = next(iter(ts2))
    rows.append(f"2. keep_ratio downscale, batch {B} (bytes = the source read once + 24 B per output pixel)")
    rows.append(line(k2, statistics.median(ts2[k2]), B * 1080 * 1920 * 6 + 24 * B * 576 * 1024, ts2[k2]))
    rows.append("")
    # results must not change while they are timed: the timed launches against the numpy restatement
    rgb, aux = a1042.cpu().numpy(), b1042.cpu().numpy()
    want = torch.from_numpy(RR.pipeline_ref(rgb, aux, pp.resize, cfg["mean"], cfg["std"], cfg["to_rgb"], cfg["modalities_name"], cfg["norm_by_max"], "multimodal"))
    assert torch.equal(pp(a1042, b1042, out=out).cpu(), want), "the timed launch differs from the restatement"
    rows.append("the timed 1042^2 uint8 launch equals tests/preprocess_resize_ref.py bit for bit")
    text = "\n".join(rows) + "\n"
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    open(args.out, "w").write(text)


if __name__ == "__main__":
    main()
