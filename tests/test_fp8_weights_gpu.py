"""Opt-in fp8 (e4m3) weights of the ViT-block GEMMs (`model.fp8_weights`, csrc/gemm_h8c_w8.hip) on the MI355X: the kernel against float64 and
against the h8c kernel on the same effective weights, the model against the oracle loaded with `effective_state_dict()`, the guards, determinism,
packed checkpoints and the pack-time refusals."""
import os

import numpy as np
import pytest
import torch

from oracle import ref_encoder as R
from tests.configs import CONFIGS, make_input, probe_index
from tests.weights import large_magnitude, peaky_attention, seeded_state_dict
from tests.util import assert_close, max_rel, rel_l2

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

# a model whose block GEMMs qualify for h8c / W8 (every contraction >= 512): tiny256 with embed 512, 8 heads (64 wide), 32-wide MSDA heads as at ViT-L
KW512 = dict(CONFIGS["tiny256"]["kwargs"], embed_dim=512, num_heads=8, deform_num_heads=8)
SITES = ("qkv", "proj", "lin1", "lin2")


def _gemm_case(M, N, K, seed):
    g = torch.Generator().manual_seed(seed)
    a = torch.randn(M, K, generator=g).to(DEV)
    w = (torch.randn(N, K, generator=g) * torch.exp2(torch.randint(-3, 3, (N, 1), generator=g).float()) / K ** 0.5).to(DEV)
    return a, w


def _run_both(a, w, **kw):
    """(W8 kernel output, h8c kernel output on the same A planes and W_eff as h8c planes, float64 reference on the fp32 A and W_eff)"""
    from mmsa import ops
    ap = ops.split_planes(a, fmt=ops.FMT_H8C)
    w8 = ops.w8_planes(w)
    weff = ops.planes_to_float(w8)
    wh = ops.split_planes(weff, fmt=ops.FMT_H8C)
    return ap, w8, wh, weff


@pytest.mark.parametrize("M", [1000, 8192])
@pytest.mark.parametrize("NK", [(2304, 768), (3072, 1024), (4096, 1024), (1024, 4096), (4608, 1280), (1280, 1536), (5120, 1280), (1280, 5120)])
def test_w8_kernel_against_float64(M, NK):
    """fp32 output, bias: error against A W_eff^T in float64 within 1.25 x that of the h8c kernel on the same A planes with W_eff packed as h8c planes;
    bit-identical over two runs."""
    from mmsa import ops
    N, K = NK
    a, w = _gemm_case(M, N, K, seed=M + N + K)
    ap, w8, wh, weff = _run_both(a, w)
    bias = torch.randn(N, device=DEV) * 0.1
    ref = (a.double() @ weff.double().t() + bias.double())
    out8 = ops.gemm(ap, w8, torch.empty(M, N, device=DEV), bias=bias, m=M)
    out8b = ops.gemm(ap, w8, torch.empty(M, N, device=DEV), bias=bias, m=M)
    outh = ops.gemm(ap, wh, torch.empty(M, N, device=DEV), bias=bias, m=M)
    torch.cuda.synchronize()
    assert torch.equal(out8, out8b), "two runs differ"
    e8, eh = rel_l2(out8, ref), rel_l2(outh, ref)
    assert e8 <= 1.25 * eh, f"M={M} N={N} K={K}: W8 {e8:.3e} vs h8c {eh:.3e}"
    assert max_rel(out8, ref) <= 1.25 * max_rel(outh, ref) + 1e-6


@pytest.mark.parametrize("M", [1000, 8192])
def test_w8_kernel_epilogues(M):
    """Every epilogue the four ViT sites use, on W8 weights against the h8c kernel on W_eff (same A planes) and float64: GELU into h8c planes (lin1),
    colscale x alpha + residual (gamma and residual: proj / lin2), LayerNorm-fold producer (rowstats_out + stream planes) and consumer (row_norm,
    planes out), qkv's f3 | h8 v-split planes output."""
    from mmsa import ops
    N, K = 2048, 1024
    a, w = _gemm_case(M, N, K, seed=7 + M)
    ap, w8, wh, weff = _run_both(a, w)
    bias = torch.randn(N, device=DEV) * 0.1
    lin = a.double() @ weff.double().t() + bias.double()

    def both(fn):
        r8, rh = fn(w8), fn(wh)
        torch.cuda.synchronize()
        return r8, rh

    def check(r8, rh, ref, what):
        e8, eh = rel_l2(r8, ref), rel_l2(rh, ref)
        assert e8 <= 1.25 * eh + 1e-7, f"{what}: W8 {e8:.3e} vs h8c {eh:.3e}"
        assert rel_l2(r8, rh) <= 1e-4, what
    # GELU -> h8c planes (lin1)
    r8, rh = both(lambda ww: ops.planes_to_float(ops.gemm(ap, ww, bias=bias, act="gelu", m=M, out_planes=ops.alloc_planes(M, N, DEV, fmt=ops.FMT_H8C))))
    check(r8, rh, torch.nn.functional.gelu(lin), "gelu -> h8c planes")
    # colscale (gamma) x alpha + beta residual, fp32 out (proj / lin2 with layer scale)
    gam = torch.rand(N, device=DEV) + 0.5
    res = torch.randn(M, N, device=DEV)
    r8, rh = both(lambda ww: ops.gemm(ap, ww, torch.empty(M, N, device=DEV), bias=bias, colscale=gam, alpha=0.75, resid=res, beta=1.0, m=M))
    check(r8, rh, res.double() + 0.75 * gam.double() * lin, "gamma + residual")
    # LayerNorm-fold producer: fp32 + residual + stream planes + row strip sums
    if M % 256 == 0:
        rs8, rsh = torch.zeros(M, N // 64, 2, device=DEV), torch.zeros(M, N // 64, 2, device=DEV)
        o8 = ops.gemm(ap, w8, torch.empty(M, N, device=DEV), bias=bias, resid=res, m=M, out_planes=ops.alloc_planes(M, N, DEV, fmt=ops.FMT_H8C), rowstats_out=rs8)
        oh = ops.gemm(ap, wh, torch.empty(M, N, device=DEV), bias=bias, resid=res, m=M, out_planes=ops.alloc_planes(M, N, DEV, fmt=ops.FMT_H8C), rowstats_out=rsh)
        torch.cuda.synchronize()
        check(o8, oh, res.double() + lin, "producer fp32")
        assert rel_l2(rs8, rsh) <= 1e-4
    # LayerNorm-fold consumer: row_norm with column sums, planes out (qkv / lin1 form)
    mr = torch.stack([torch.randn(M, device=DEV) * 0.1, torch.rand(M, device=DEV) + 0.5], 1).contiguous()
    cs = weff.double().sum(1).float().contiguous()
    r8, rh = both(lambda ww: ops.planes_to_float(ops.gemm(ap, ww, bias=bias, m=M, out_planes=ops.alloc_planes(M, N, DEV, fmt=ops.FMT_H8C), row_norm=(mr, cs))))
    refn = mr[:, 1:2].double() * (a.double() @ weff.double().t() - mr[:, 0:1].double() * cs.double()) + bias.double()
    check(r8, rh, refn, "row_norm -> planes")
    # qkv: f3 planes with the v third as h8 planes
    r8, rh = both(lambda ww: ops.planes_to_float(ops.gemm(ap, ww, bias=bias, m=M, out_planes=ops.alloc_planes(M, N, DEV, fmt=ops.FMT_F3, split=2 * N // 3 // 32 * 32))))
    check(r8, rh, lin, "f3 | h8 split planes")


def _models(sd_mod=None, seed=61):
    import mmsa
    torch.manual_seed(0)
    orc = R.OracleEncoder(**KW512)
    sd = seeded_state_dict(orc, seed=seed)
    if sd_mod is not None:
        sd = sd_mod(sd)
    m = mmsa.build_backbone(dict(type="SAMAdapterbimodalMixModNewInTwinConvNEW", **KW512))
    m.load_state_dict(sd, strict=True)
    return orc, sd, m


def _block_bytes(m):
    return sum(m._packed["blocks"][i][s].p.numel() * m._packed["blocks"][i][s].p.element_size() for i in range(len(m._packed["blocks"])) for s in SITES)


def test_fp8_model_against_the_oracle_on_effective_weights():
    """fp8_weights = True: f1..f4 within the gate of the oracle loaded with m.effective_state_dict(); every block runs W8 on all four sites; packed
    block weights <= 0.36 x the default pack's; the outputs differ from the default model's (the fp8 path ran).  Fails without the feature."""
    import mmsa
    from mmsa import ops
    orc, sd, m = _models()
    x = make_input(dict(kwargs=KW512, in_seed=62), batch=1)
    m0 = mmsa.build_backbone(dict(type="SAMAdapterbimodalMixModNewInTwinConvNEW", **KW512))
    m0.load_state_dict(sd, strict=True)
    f0 = [f.clone() for f in m0(x.to(DEV))[0]]
    m.fp8_weights = True
    fs, _ = m(x.to(DEV))
    assert all(bp[s].fmt == ops.FMT_W8 for bp in m._packed["blocks"] for s in SITES)
    assert _block_bytes(m) <= 0.36 * _block_bytes(m0), (_block_bytes(m), _block_bytes(m0))
    eff = m.effective_state_dict()
    assert list(eff.keys()) == list(m.state_dict().keys())
    orc.load_state_dict(eff)
    ref, _ = orc(x)
    for i, (f, r) in enumerate(zip(fs, ref)):
        assert_close(f, r, what=f"fp8 weights f{i+1} vs oracle on the effective weights")
    assert not all(torch.equal(a_, b_) for a_, b_ in zip(fs, f0))


def test_fp8_guards_move_blocks_and_go_wide():
    """The attention logit guard (q / k rows x 3: blocks move to f3 pairs, repacked from the effective weights) and the wide-range state (a post-LayerNorm
    channel of ~1e5, a GELU hidden of 6e4: bf16 pairs) keep computing with the effective weights: both against the oracle on effective_state_dict()."""
    from mmsa import ops
    x = make_input(dict(kwargs=KW512, in_seed=63), batch=1)
    orc, sd, m = _models(lambda s: peaky_attention(s, 512, 3.0))
    m.fp8_weights = True
    fs, _ = m(x.to(DEV))
    moved = [bp["index"] for bp in m._packed["blocks"] if bp["qkv"].fmt == ops.FMT_F3]
    assert moved, "no block moved to pairs"
    assert all(bp["qkv"].fmt in (ops.FMT_F3, ops.FMT_W8) for bp in m._packed["blocks"])
    orc.load_state_dict(m.effective_state_dict())
    for i, (f, r) in enumerate(zip(fs, orc(x)[0])):
        assert_close(f, r, what=f"fp8 peaky (moved {moved}) f{i+1} vs oracle")
    orc, sd, m = _models(lambda s: large_magnitude(s, dict(ln2=(1, 5), ln1=(2, 9), gelu=(3, 17))))
    m.fp8_weights = True
    fs, _ = m(x.to(DEV))
    assert m._wide() and all(bp["qkv"].fmt == ops.FMT_B3 for bp in m._packed["blocks"])
    orc.load_state_dict(m.effective_state_dict())
    for i, (f, r) in enumerate(zip(fs, orc(x)[0])):
        assert_close(f, r, what=f"fp8 wide-range state f{i+1} vs oracle")


def test_fp8_packed_checkpoint_round_trip_and_refusals(tmp_path):
    import mmsa
    from mmsa import checkpoint as C
    orc, sd, m = _models()
    del orc
    m.fp8_weights = True
    x = make_input(dict(kwargs=KW512, in_seed=64), batch=2).to(DEV)
    ref = [f.clone() for f in m(x)[0]]
    path = str(tmp_path / "fp8.packed.pth")
    C.save_packed(m, path, device=DEV)
    assert torch.load(path, map_location="cpu")["settings"]["fp8_weights"] is True
    m2 = mmsa.build_backbone(dict(type="SAMAdapterbimodalMixModNewInTwinConvNEW", **KW512))
    m2.fp8_weights = True
    C.load_packed(m2, path, device=DEV)

    def boom(dev):
        raise AssertionError("_pack must not run after load_packed")
    m2._pack = boom
    for a_, b_ in zip(m2(x)[0], ref):
        assert torch.equal(a_, b_)
    m3 = mmsa.build_backbone(dict(type="SAMAdapterbimodalMixModNewInTwinConvNEW", **KW512))
    with pytest.raises(RuntimeError, match="repack"):
        C.load_packed(m3, path, device=DEV)            # an fp8 pack into a model without the switch
    m3.load_state_dict(sd, strict=True)
    dpath = str(tmp_path / "default.packed.pth")
    C.save_packed(m3, dpath, device=DEV)
    assert "fp8_weights" not in torch.load(dpath, map_location="cpu")["settings"]
    m4 = mmsa.build_backbone(dict(type="SAMAdapterbimodalMixModNewInTwinConvNEW", **KW512))
    m4.fp8_weights = True
    with pytest.raises(RuntimeError, match="repack"):
        C.load_packed(m4, dpath, device=DEV)           # a default pack into an fp8 model


def test_fp8_pack_refuses_unsupported_configurations():
    """The switch is never ignored: where the ViT-block GEMMs would not run on h8c planes the pack raises."""
    import mmsa
    cfg = CONFIGS["tiny256"]
    x = make_input(cfg).to(DEV)
    m = mmsa.build_backbone(dict(type="SAMAdapterbimodalMixModNewInTwinConvNEW", **cfg["kwargs"]))
    m.load_state_dict(seeded_state_dict(m, seed=cfg["seed"]), strict=True)
    m.fp8_weights = True
    with pytest.raises(ValueError, match="shorter than 512"):
        m(x)
    orc, sd, m = _models()
    del orc
    xx = make_input(dict(kwargs=KW512, in_seed=65), batch=1).to(DEV)
    m.fp8_weights, m.h8c = True, False
    with pytest.raises(ValueError, match="h8c is off"):
        m(xx)
    m.h8c, m.h8_sites = True, ("inter", "up", "attnv")
    m.invalidate()
    with pytest.raises(ValueError, match="'vit' is not among"):
        m(xx)


# rel-L2 drift of fp8 f1..f4 against the committed fp32-weight reference probes (image 0), as measured on the MI355X (tools/fp8_weights_bench.py,
# profiles/fp8_weights_ab.txt): what e4m3 weights (3 mantissa bits) cost on the seeded weights.  The test holds it below twice that value.
DRIFT = {"vitl1024": (3.063e-2, 4.472e-2, 4.749e-2, 5.105e-2), "vith1024": (3.596e-2, 5.531e-2, 5.592e-2, 6.061e-2)}


@pytest.mark.parametrize("name", ["vitl1024", "vith1024"])
def test_fp8_vit_l_and_h_eager_replayed_and_deterministic(golden_dir, name):
    """ViT-L / ViT-H at 1024^2 with fp8 weights: eager and graph-replayed forwards finite and bit-identical; batch 1 vs batch 2 bit-identical per image;
    two Chains equal one chain; rel-L2 drift against the reference probes (fp32 weights) below 2 x the measured value (DRIFT: ViT-L 3.1 / 4.5 / 4.7 /
    5.1 %, ViT-H 3.6 / 5.5 / 5.6 / 6.1 % on f1 .. f4)."""
    import mmsa
    cfg = CONFIGS[name]
    m = mmsa.build_backbone(dict(type="SAMAdapterbimodalMixModNewInTwinConvNEW", **cfg["kwargs"]))
    m.load_state_dict(seeded_state_dict(m, seed=cfg["seed"]), strict=True)
    m.fp8_weights = True
    x = make_input(cfg, batch=2, seed=1234).to(DEV)
    x[0].copy_(make_input(cfg)[0].to(DEV))
    eager = [f.clone() for f in m(x)[0]]
    assert all(torch.isfinite(f).all() for f in eager)
    one = m(x[1:2])[0]
    for a_, b_ in zip(eager, one):
        assert torch.equal(a_[1:2], b_), "batch 1 vs batch 2"
    holder = {}
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        m(x)
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        holder["fs"] = m(x)[0]
    for t in holder["fs"]:
        t.fill_(float("nan"))
    graph.replay()
    torch.cuda.synchronize()
    for a_, b_ in zip(holder["fs"], eager):
        assert torch.equal(a_, b_), "replay vs eager"
    del graph, holder
    if name == "vitl1024":
        x4 = torch.cat([x, x.flip(0)], 0)
        ch = mmsa.Chains(m, None, n=2).capture(x4)
        feats = ch.replay().outputs()
        torch.cuda.synchronize()
        for c in range(2):
            fs = m(x4[2 * c:2 * c + 2])[0]
            for k in range(4):
                assert torch.equal(feats[c][k], fs[k]), "two chains vs one"
    g = np.load(os.path.join(golden_dir, f"model_{name}.npz"))
    for i, f in enumerate(eager):
        pi = probe_index(f[0].numel(), 2048, seed=100 + i)
        got, ref = f[0].flatten()[pi.to(DEV)].cpu(), torch.from_numpy(g[f"f{i+1}_probe"])
        d = rel_l2(got, ref)
        print(f"{name} fp8 f{i+1} drift rel_l2 {d:.3e} max_rel {max_rel(got, ref):.3e}")
        assert d < 2 * DRIFT[name][i], (name, i, d)
