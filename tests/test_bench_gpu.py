"""bench.py itself on the GPU box, on a small configuration: the eager (`--no-graph`) path verifies the outputs it has just computed
(it probed stale tensors and failed spuriously; the counter-pass scripts tools/pmc_*.sh run exactly this mode)."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu


def _bench(*args, full=True):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--config", "vitb512", "--steps", "2", "--warmup", "1"]
                       + (["--full", "--no-cpu-baseline", "--no-roofline"] if full else []) + list(args), capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1]
    return json.loads(line)


def test_bench_no_graph_verifies_the_eager_outputs():
    d = _bench("--no-graph", "--chains", "1")
    assert d["config"]["hip_graph"] is False
    assert d["metric"].endswith("ViT-B") and "NOT the BASELINE headline" in d["config"]["workload"]
    assert d["verified"]["replayed_graph_vs_reference_golden_probes_max_rel"] <= 1e-3
    assert d["value"] > 0 and d["vs_baseline"] is None


def test_bench_graph_and_chains_verify_bitwise():
    d = _bench()
    assert d["config"]["hip_graph"] is True
    assert d["verified"]["graph_replay_equals_eager_bitwise"] is True
    assert d["verified"]["replayed_graph_vs_reference_golden_probes_max_rel"] <= 1e-3
    assert d["config"]["attention_blocks"]["f16"] + d["config"]["attention_blocks"]["b3"] == 12
    assert d["config"]["attention_blocks"]["interactions_on_pairs"] == [] and d["config"]["attention_blocks"]["wide_range_state"] is False


def test_bench_roofline_families_and_pipelined_gather_fields():
    """Round 6: the GEMM roofline is reported in two families -- launches that can be matrix-bound (`roofline.frac`) and launches below 100 FLOP per compulsory
    byte scored against HBM (`roofline.hbm_gemms`) -- and `roofline.all_gemm_launches` keeps the definition of rounds 1-5; their launch counts, FLOPs and kernel
    times add up.  Single rank: no collective, no overlap record."""
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--config", "vitb512", "--steps", "2", "--warmup", "1", "--full", "--no-cpu-baseline",
                        "--no-extras"],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    d = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])
    rf = d["roofline"]
    assert rf["bound"] == "mfma" and rf["hbm_gemms"]["bound"] == "hbm" and rf["hbm_gemms"]["peak"] == 8000.0
    al = rf["all_gemm_launches"]
    assert rf["launches_per_step"] + rf["hbm_gemms"]["launches_per_step"] == al["launches_per_step"] and rf["hbm_gemms"]["launches_per_step"] > 0
    assert abs(rf["algorithmic_gflop_per_step"] + rf["hbm_gemms"]["algorithmic_gflop_per_step"] - al["algorithmic_gflop_per_step"]) <= 0.3
    assert abs(rf["kernel_ms_per_step"] + rf["hbm_gemms"]["kernel_ms_per_step"] - al["kernel_ms_per_step"]) <= 0.01
    assert rf["frac"] >= al["frac"] and 0.0 < rf["hbm_gemms"]["frac"] < 1.0
    assert d["config"]["collective_overlap"] is None and d["config"]["host_threads_per_rank"] is None


def test_bench_plain_run_dumps_the_logits_of_its_last_timed_step(tmp_path):
    """Without --full the benchmark times the step and computes nothing else; --dump-outputs writes the logits the last timed step returned.  The
    replayed graph and the eager launch sequence write the same logits bit for bit."""
    import numpy as np
    runs = {"graph": _bench("--dump-outputs", str(tmp_path / "graph"), full=False),
            "eager": _bench("--no-graph", "--chains", "1", "--dump-outputs", str(tmp_path / "eager"), full=False)}
    for d in runs.values():
        assert d["steps"] == 2 and d["ms_per_step"] > 0 and abs(d["value"] - 2 / (d["ms_per_step"] * 1e-3)) < 1e-2 * d["value"]
        assert all(d[k] is None for k in ("verified", "encoder_only", "replay_ms", "attention_guard", "roofline", "hbm_kernels", "cpu_baseline",
                                          "worst_case_precision", "eager_plugin_api", "config4_frame", "vith1024"))
    assert runs["graph"]["config"]["hip_graph"] is True and runs["eager"]["config"]["hip_graph"] is False
    g, e = np.load(tmp_path / "graph" / "logits.npy"), np.load(tmp_path / "eager" / "logits.npy")
    assert g.shape == (2, 25, 128, 128) and g.dtype == np.float32 and np.isfinite(g).all() and g.std() > 0
    assert np.array_equal(g, e)


def _gather_cuda_worker(rk, ws, port, q):
    import torch
    import torch.distributed as dist
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    sys.path.insert(0, os.path.join(ROOT, "multimodal-sam-adapter_amd"))
    torch.cuda.set_device(0)
    dist.init_process_group("gloo", rank=rk, world_size=ws)
    from mmsa.dist import LogitsGather
    dev = torch.device("cuda", 0)
    g = LogitsGather()
    local = torch.zeros(2, 25, 64, 64, device=dev)
    big = torch.zeros(64 << 20, device=dev)             # something for the launch stream to be busy with
    ok, err = True, ""
    try:
        hs = []
        for k in range(5):
            big.add_(1.0)                                # "replay k" ...
            local.fill_(100.0 * k + rk)                  # ... writes the step's logits
            hs.append(g.submit(local))
            local.fill_(-1.0)                            # the NEXT replay overwrites the buffer at once: ordered behind the staging copy only
            if k >= 1:
                r_ = hs[k - 1].result()
                want = [100.0 * (k - 1) + r for r in range(ws) for _ in range(2)]
                got = r_[:, 0, 0, 0].tolist()
                ok = ok and got == want and bool((r_ == r_[:, :1, :1, :1]).all())
        r_ = hs[-1].result()
        ok = ok and r_[:, 0, 0, 0].tolist() == [400.0 + r for r in range(ws) for _ in range(2)]
        ok = ok and g.stream is not None and g.stream != torch.cuda.current_stream(dev)
    except RuntimeError as e:                            # gloo without CUDA all-gather support on this build
        ok, err = False, str(e)
    q.put((rk, ok, err))
    dist.destroy_process_group()


def test_logits_gather_cuda_side_stream_gloo_world2():
    """mmsa.dist.LogitsGather on DEVICE tensors (two ranks sharing the one GPU of the box, gloo as the transport): the staging copy runs on the gather's own
    stream behind the step that wrote the logits, the launch stream waits for that copy only, so a next step that overwrites the logits buffer immediately
    does not disturb the gathered tensor -- the property the N > 1 bench relies on when it enqueues replay k + 1 before gather k has completed."""
    import torch.multiprocessing as mp
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = 29650 + os.getpid() % 300
    procs = [ctx.Process(target=_gather_cuda_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = [q.get(timeout=300) for _ in procs]
    for p in procs:
        p.join(60)
    if any("not supported" in err or "unsupported" in err.lower() for _, _, err in res):
        pytest.skip("gloo cannot all-gather device tensors in this build: " + res[0][2][:200])
    for rk, ok, err in res:
        assert ok, f"rank {rk}: {err}"
