"""fp8 (e4m3) ViT-block weights (`model.fp8_weights`) against the default h8c planes, on one box:

    python tools/fp8_weights_bench.py [--rounds 3] [--steps 20] [--warmup 5] [--out profiles/fp8_weights_ab.txt]

  * step A/B: bench.py's replayed batch-2 step with the decode head (ViT-L 1024^2 and ViT-H 1024^2), fp8 on / off INTERLEAVED for `--rounds` rounds
    (the order alternates per round), each leg a fresh bench.py process (`--set fp8_weights=True`, `--no-verify`: the golden probes are fp32-weight
    probes, which fp8 weights do not meet -- their drift is reported below instead);
  * per-site GEMM microseconds (qkv, proj, lin1, lin2) of one eager ViT-L batch-2 forward from ops.GEMM_PROFILE (device events around every launch);
  * packed ViT-block weight bytes (the four sites of every block);
  * drift of fp8 f1..f4 against the committed fp32-weight reference probes of vitl1024 / vith1024 (rel-L2, max-rel: what fp8 costs on those seeded weights).
The record is stamped with the kernel-source digest (build.source_digest())."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "multimodal-sam-adapter_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)
SITES = ("qkv", "proj", "lin1", "lin2")


def bench_leg(config, fp8, steps, warmup):
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(steps), "--warmup", str(warmup), "--config", config,
           "--no-verify", "--no-cpu-baseline", "--no-roofline"] + (["--set", "fp8_weights=True"] if fp8 else [])
    r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=900)
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    if r.returncode != 0 or not lines:
        raise RuntimeError(f"bench.py failed ({r.returncode}): {r.stderr[-2000:]}")
    return json.loads(lines[-1])["ms_per_step"]


def model(name, fp8):
    import mmsa
    from tests.configs import CONFIGS
    from tests.weights import seeded_state_dict
    cfg = CONFIGS[name]
    m = mmsa.build_backbone(dict(type="SAMAdapterbimodalMixModNewInTwinConvNEW", **cfg["kwargs"]))
    m.load_state_dict(seeded_state_dict(m, seed=cfg["seed"]), strict=True)
    m.fp8_weights = fp8
    return cfg, m


def site_of(m, n, k):
    D, heads = m.cfg["embed_dim"], m.cfg["num_heads"]
    Da = heads * ((D // heads + 31) // 32 * 32)
    hidden = int(D * m.cfg["mlp_ratio"])
    return {(3 * Da, D): "qkv", (D, Da): "proj", (hidden, D): "lin1", (D, hidden): "lin2"}.get((n, k))


def per_site_us(fp8):
    import torch
    from mmsa import ops
    from tests.configs import make_input
    cfg, m = model("vitl1024", fp8)
    x = make_input(cfg, batch=2, seed=1234).to("cuda:0")
    m(x)
    torch.cuda.synchronize()
    prof, shapes = [], []
    ops.GEMM_PROFILE, ops.GEMM_SHAPES = prof, shapes
    try:
        m(x)
        torch.cuda.synchronize()
    finally:
        ops.GEMM_PROFILE, ops.GEMM_SHAPES = None, None
    ops.collect_gemm_profile(prof)
    acc = {s: [] for s in SITES}
    for (f, by, ms), sh in zip(ops.collect_gemm_profile.launches, shapes):
        s = site_of(m, sh[1], sh[2])
        if s is not None and sh[0] == 2 * 64 * 64:
            acc[s].append(ms * 1e3)
    nbytes = sum(bp[s].p.numel() * bp[s].p.element_size() for bp in m._packed["blocks"] for s in SITES)
    return {s: (statistics.median(v), len(v)) for s, v in acc.items() if v}, nbytes


def drift(name):
    import numpy as np
    import torch
    from tests.configs import make_input, probe_index
    from tests.util import max_rel, rel_l2
    cfg, m = model(name, True)
    fs = m(make_input(cfg).to("cuda:0"))[0]
    g = np.load(os.path.join(ROOT, "tests", "golden", f"model_{name}.npz"))
    out = []
    for i, f in enumerate(fs):
        pi = probe_index(f.numel(), 2048, seed=100 + i)
        got, ref = f.flatten()[pi.to(f.device)].cpu(), torch.from_numpy(g[f"f{i+1}_probe"])
        out.append((rel_l2(got, ref), max_rel(got, ref)))
    nbytes = sum(bp[s].p.numel() * bp[s].p.element_size() for bp in m._packed["blocks"] for s in SITES)
    _, m0 = model(name, False)
    m0(make_input(cfg).to("cuda:0"))
    nbytes0 = sum(bp[s].p.numel() * bp[s].p.element_size() for bp in m0._packed["blocks"] for s in SITES)
    return out, nbytes, nbytes0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--configs", default="vitl1024,vith1024")
    ap.add_argument("--skip-ab", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fp8_weights_ab.txt"))
    a = ap.parse_args()
    import build
    lines = [f"# tools/fp8_weights_bench.py -- source digest {build.source_digest()} -- {time.strftime('%Y-%m-%d %H:%M:%S')}"]

    def emit(s):
        print(s, flush=True)
        lines.append(s)
    if not a.skip_ab:
        for config in a.configs.split(","):
            res = {False: [], True: []}
            for r in range(a.rounds):
                for fp8 in ((False, True) if r % 2 == 0 else (True, False)):
                    res[fp8].append(bench_leg(config, fp8, a.steps, a.warmup))
            for fp8 in (False, True):
                v = res[fp8]
                emit(f"{config} batch 2 + head, replayed, fp8_weights={fp8}: ms/step {' '.join(f'{t:.3f}' for t in v)}  median {statistics.median(v):.3f}  "
                     f"spread {max(v) - min(v):.3f}")
            emit(f"{config} fp8 / default (medians): {statistics.median(res[True]) / statistics.median(res[False]):.4f}")
    s0, b0 = per_site_us(False)
    s1, b1 = per_site_us(True)
    emit("ViT-L 1024^2 batch 2, eager, per-site GEMM us (median over the 24 blocks): site  default(h8c)  fp8(W8)  ratio")
    for s in SITES:
        emit(f"  {s:5s} {s0[s][0]:9.1f} {s1[s][0]:9.1f}  {s1[s][0] / s0[s][0]:.3f}   ({s1[s][1]} launches)")
    for name in ("vitl1024", "vith1024"):
        d, nb, nb0 = drift(name)
        emit(f"{name}: packed ViT-block weight bytes fp8 {nb / 1e6:.1f} MB vs default {nb0 / 1e6:.1f} MB ({nb / nb0:.3f})")
        emit(f"{name}: fp8 drift against the fp32-weight reference probes: " + "  ".join(f"f{i+1} rel_l2 {r:.3e} max_rel {mr:.3e}" for i, (r, mr) in enumerate(d)))
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
