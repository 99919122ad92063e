"""Keeps the bound of tests/variant_ref.py honest, on the CPU, for every case of the table in tests/test_kernel_variants_gpu.py: torch's own fp32
evaluation of the same statement stays inside the bound (the float64 reference and the bound are consistent with plain fp32 arithmetic), and a
result with ONE border element moved by 8x its bound is rejected (the check is per element, nothing is averaged away).  The MSDA restatement is
checked once against the oracle's msda_core, the MSDA backward restatement against float64 autograd through the forward restatement and through msda_core,
and deliberately wrong restatements of LayerNorm and MSDA (forward and backward) must land outside the bound: the width of the bound is a checked
property too."""
import pytest
import torch

from tests import variant_ref as V
from tests.test_kernel_variants_gpu import CASES, RAISES


@pytest.mark.parametrize("cid,op,p", CASES, ids=[c[0] for c in CASES])
def test_bound_admits_fp32_and_rejects_one_bad_element(cid, op, p):
    i, r, bnd = V.case_data(cid, op, p)
    assert r.dtype == torch.float64 and bnd.dtype == torch.float64 and r.shape == bnd.shape
    assert bool(torch.isfinite(r).all()) and bool(torch.isfinite(bnd).all()) and bool((bnd >= 0).all())
    y = V.fp32_eval(op, i, p)
    assert y.dtype == torch.float32 or op in ("colstats", "gram") or p.get("dtype") == "f64"      # (results the device itself returns as double)
    V.assert_inside(y, r, bnd, cid + " (torch fp32 on the CPU)")
    # the first and the last element are border elements of every layout here (corner pixel, first / last channel); take the ones with a bound > 0
    flat_b = bnd.flatten()
    cand = [k for k in (0, flat_b.numel() - 1) if float(flat_b[k]) > 0] or [int(torch.argmax(flat_b))]
    assert float(flat_b[cand[0]]) > 0, "a case whose every bound is zero cannot be checked this way"
    for k in cand:
        bad = r.clone().flatten()
        bad[k] += 8 * flat_b[k]
        assert int(V.violations(bad.view_as(r), r, bnd).sum()) == 1
        with pytest.raises(AssertionError):
            V.assert_inside(bad.view_as(r), r, bnd, cid)


def test_table_is_complete():
    ops_used = {c[1] for c in CASES}
    assert ops_used == set(V.OPS), sorted(set(V.OPS) - ops_used)
    assert all(p["B"] == 2 for _, _, p in CASES + RAISES)


def test_nan_is_outside_the_bound():
    r = torch.zeros(4, dtype=torch.float64)
    y = r.clone()
    y[2] = float("nan")
    assert int(V.violations(y, r, torch.ones(4, dtype=torch.float64)).sum()) == 1


def _fused_as_forward(i, p):
    """The fused case's locations and weights, formed in float64 as the restatement says: loc = ref + off / (W_l, H_l), softmax over L * P."""
    levels, _, S = V.msda_geometry(p)
    Bn, M, D, Lq, P, L = p["B"], p["M"], p["D"], p["Lq"], p["P"], len(levels)
    raw = i["raw"].double()
    off = raw[:, :M * L * P * 2].reshape(Bn, Lq, M, L, P, 2)
    wgt = torch.softmax(raw[:, M * L * P * 2:].reshape(Bn, Lq, M, L * P), -1).view(Bn, Lq, M, L, P)
    size = torch.tensor([[w, h] for h, w in levels], dtype=torch.float64).view(1, 1, 1, L, 1, 2)
    return i["value"].double().view(Bn, S, M, D), i["ref"].double().view(1, Lq, 1, 1, 1, 2) + off / size, wgt


@pytest.mark.parametrize("cid", ["msda-d32-q33", "msdaf-m3d12"])
def test_msda_restatement_agrees_with_the_oracle(cid):
    """The direct gather of variant_ref against oracle.ref_encoder.msda_core (grid_sample based) in float64, to 1e-12 relative."""
    from oracle.ref_encoder import msda_core
    _, op, p = next(c for c in CASES if c[0] == cid)
    i, r, _ = V.case_data(cid, op, p)
    value, loc, wgt = _fused_as_forward(i, p) if op == "msda_fused" else (i["value"].double(), i["loc"].double(), i["aw"].double())
    want = msda_core(value, torch.tensor(p["levels"]), loc, wgt).reshape(r.shape)
    assert float((want - r).abs().max()) <= 1e-12 * float(want.abs().max())


@pytest.mark.parametrize("cid", ["msdab-f32-shfl-m3d8-q33", "msdab-f32-atom-m4d40-q26"])
def test_msda_backward_restatement_agrees_with_autograd(cid):
    """The direct statement of the three gradients against float64 autograd through variant_ref._gather (floor-based taps, like the statement) and through
    oracle.ref_encoder.msda_core (grid_sample based), to 1e-12 relative per gradient."""
    from oracle.ref_encoder import msda_core
    _, op, p = next(c for c in CASES if c[0] == cid)
    i, r, _ = V.case_data(cid, op, p)
    levels, starts, _ = V.msda_geometry(p)
    parts = V.msda_bwd_slices(p)
    for fwd in (lambda v, lo, a: V._gather(v, levels, starts, lo, a)[0], lambda v, lo, a: msda_core(v, torch.tensor(levels), lo, a).view(i["gout"].shape)):
        v, lo, a = (i[k].double().requires_grad_(True) for k in ("value", "loc", "aw"))
        (fwd(v, lo, a) * i["gout"].double()).sum().backward()
        for name, got in (("gvalue", v.grad), ("gloc", lo.grad), ("gaw", a.grad)):
            assert float((got.reshape(-1) - r[parts[name]]).abs().max()) <= 1e-12 * float(got.abs().max()), name


MUTANTS = {"layernorm_rows": ("mean_drop4", "var_cm1", "eps", "group0"), "msda": ("nohalf", "swap", "start"), "msda_fused": ("nohalf", "swap", "start", "softmaxP"),
           "msda_bwd": ("swapWH", "noaw", "awaw", "dhsign", "start")}


@pytest.mark.parametrize("op,mut", [(op, m) for op, ms in MUTANTS.items() for m in ms])
def test_bound_rejects_wrong_statements(op, mut):
    """A float64 restatement that is wrong in one respect -- LayerNorm: the mean without the row's last four channels, the variance over C - 1, the other
    eps, every group given group 0's weights; MSDA: no -0.5, H and W exchanged in the normalisation, the second level's start index one row too late, the
    softmax over P instead of L * P; MSDA backward: W and H exchanged in the scale of grad_sampling_loc, grad_sampling_loc without the attention weight,
    grad_attn_weight times the attention weight, the sign of one tap's dh flipped, the second level's start index one row too late -- lands outside the bound in at least one element of at least one case of the family."""
    caught = 0
    for cid, cop, p in CASES:
        if cop != op or p.get("rows", 0) > 1000 or caught >= 3:
            continue
        i, r, bnd = V.case_data(cid, cop, p)
        wrong = V.OPS[cop][1](V.cast(i, torch.float64), p, mut=mut)[0]
        caught += int(V.violations(wrong, r, bnd).any())
    assert caught, f"no {op} case rejects the mutant '{mut}': the table lacks a case"
