"""Keeps the bound of tests/gemm_ref.py honest, on the CPU, for every case of the table in tests/test_gemm_variants_gpu.py: the reference and the bound are
finite float64 of one shape; torch's own fp32 evaluation of the same restatement (three fp32 matmuls and the epilogue in fp32) stays inside the bound -- and
EQUALS the reference where the case is exact-grid, whose exactness condition is checked here too; the reference with its first or last element moved by 8 x
its bound (one fp32 ulp where the bound is 0) is rejected.  Deliberately wrong restatements must land outside the bound in at least one case of their family:
the width of the bound is a checked property."""
import pytest
import torch

from tests import gemm_ref as G
from tests.test_gemm_variants_gpu import CASES, RAISES
from tests.variant_ref import assert_inside


@pytest.mark.parametrize("cid,op,p", CASES, ids=[c[0] for c in CASES])
def test_bound_admits_fp32_and_rejects_one_bad_element(cid, op, p):
    i, r, bnd = G.case_data(cid, op, p)
    assert r.dtype == torch.float64 and bnd.dtype == torch.float64 and r.shape == bnd.shape
    assert bool(torch.isfinite(r).all()) and bool(torch.isfinite(bnd).all()) and bool((bnd >= 0).all())
    y = G.fp32_eval(op, i, p)
    assert y.dtype == torch.float32
    assert_inside(y, r, bnd, cid + " (torch fp32 on the CPU)")
    exact = p.get("exact") or op == "mlp_fused"
    if exact:      # every partial sum is exact in fp32 in any order
        worst, limit = G.mlp_exact_margin(i, p) if op == "mlp_fused" else G.exact_margin(i, p)
        assert worst < limit, f"sum |terms| + |bias| + |resid| = {worst} is not below 2^24 x the grid step = {limit}"
        assert p["K"] > 128 if op != "mlp_fused" else True
    else:
        assert p["K"] <= 128, "random data is used at K <= 128 only"
    if p.get("exact") and p.get("act", "none") in ("none", "relu") and not p.get("colscale") and p.get("alpha", 1.0) == 1.0 and p.get("beta", 1.0) == 1.0:
        assert bool((bnd == 0).all()) and torch.equal(y.double(), r), "an exact-grid case with a linear epilogue is held bit for bit"
    flat_b = bnd.flatten()
    for k in (0, flat_b.numel() - 1):
        bad = r.clone().flatten()
        step = 8 * float(flat_b[k])
        if step == 0.0:      # bound 0: one fp32 ulp of the value
            v = bad[k].float()
            step = float(torch.nextafter(v, v + 1) - v)
        bad[k] += step
        assert int(G.violations(bad.view_as(r), r, bnd).sum()) == 1
        with pytest.raises(AssertionError):
            assert_inside(bad.view_as(r), r, bnd, cid)


def test_table_is_complete():
    assert {c[1] for c in CASES} == set(G.OPS), sorted(set(G.OPS) ^ {c[1] for c in CASES})
    assert len(RAISES) >= 20


# mutant -> (families it is tried on, which cases of a family can show it)
_LDS = ("v2_b3w4", "v2_b3w8", "v2_h8", "v2_f3", "h8c", "w8")
MUTANTS = {
    "lohi8": (("split3", "v2_b3w4", "v2_b3w8", "v2_h8", "v2_f3", "h8c", "h8c4", "stream"), lambda p: True),      # the lo . hi term dropped for the last 8 columns of K
    "ktile128": (("split3", "stream", "h8c4") + _LDS, lambda p: p["M"] > 128),                                      # the last k-tile skipped for rows >= 128
    "bias_col": (("tiny", "split3", "stream", "h8c4") + _LDS, lambda p: p.get("bias", True)),                       # bias taken from column min(n, N - 2)
    "colscale_b0": (("tiny", "split3") + _LDS[:-1], lambda p: p.get("batch", 1) > 1 and p.get("colscale")),          # batch 1 given batch 0's colscale
    "ps_swap": (("split3",) + _LDS, lambda p: p.get("ps")),                                                         # the pixel-shuffle quadrant bits exchanged
    "rmod_src": (("split3",) + _LDS, lambda p: p.get("ps") and p.get("resid_mod")),                                 # resid_mod row from the source row, not the destination row
    "no_rn": (_LDS[1:], lambda p: p.get("rn")),                                                                     # row-normalisation left out
    "colsum_b0": (_LDS[1:-1], lambda p: p.get("rn") and p.get("batch", 1) > 1),                                      # colsum of the wrong batch
    "h8c_round": (("h8c", "h8c4"), lambda p: True),                                                                # h8c: q(hi) rounded instead of truncated
    "w8_code": (("w8",), lambda p: True),                                                                          # W8: the e4m3 code as the lo-term operand
    "b2_outside": (("mlp_fused",), lambda p: True),                                                                # mlp_fused: b2 added outside gamma
}


@pytest.mark.parametrize("mut,op", [(m, op) for m, (fams, _) in MUTANTS.items() for op in fams])
def test_bound_rejects_wrong_statements(mut, op):
    caught = tried = 0
    for cid, cop, p in CASES:
        if cop != op or not MUTANTS[mut][1](p) or caught:
            continue
        i, r, bnd = G.case_data(cid, cop, p)
        wrong = G.OPS[cop][1](i, p, mut=mut)[0]
        tried += 1
        caught += int(G.violations(wrong, r, bnd).any())
    assert caught, f"no {op} case of {tried} rejects the mutant '{mut}': the table lacks a case"


def test_tiny_weight_sum_is_exact_in_fp32():
    """gemm_tiny_kernel adds a weight's bf16 hi and lo parts in fp32 before the product: 8 + 8 significant bits, exact (its comment says so)."""
    w = torch.randn(64, 256, generator=G.gen_for("tiny-wsum")) * 3
    o = G.split(w, "b3")
    assert bool(((o["hi"] + o["lo"]).double() == o["hi"].double() + o["lo"].double()).all())
    assert bool(((o["hi"] + o["lo"] - w).abs() <= w.abs() * 2.0 ** -16).all())


def test_planes_words_layouts():
    """The five layouts of csrc/common.h, spelt out once without the device: where element (r, c) of a 3 x 70 matrix lies."""
    x = torch.arange(1, 211).float().view(3, 70) + 2.0 ** -12
    for fmt, weight in G.SPLIT_KINDS:
        o = G.split(x, fmt)
        w = G.planes_words(o, weight=weight)
        by = w.contiguous().view(torch.uint8)
        r, c = 2, 37
        if fmt in ("b3", "f3"):
            assert w.shape == (3, 192)
            hi, lo = w[r, 64 + 5], w[r, 64 + 32 + 5]
            dec = (lambda t: (t.to(torch.int32) << 16).view(torch.float32)) if fmt == "b3" else (lambda t: t.view(torch.float16).float())
            assert float(dec(hi.reshape(1))) == float(o["hi"][r, c]) and float(dec(lo.reshape(1))) == float(o["lo"][r, c])
        elif fmt == "h8":
            assert w.shape == (3, 192)
            blk = by[r, 128:256]
            assert float(blk[10:12].view(torch.float16).float()) == float(o["hi"][r, c])
            lo_at, qh_at = (64 + 8, 64) if weight else (64, 64 + 8)      # chunk g = 0 of the block, k = 5
            assert blk[lo_at + 5] == o["ql8"].view(torch.uint8)[r, c] and blk[qh_at + 5] == o["qh8"].view(torch.uint8)[r, c]
        else:
            assert w.shape == (2, 384)      # two row pairs of 3 x 128 words
            pair = by[1]
            assert float(pair[2 * 37:2 * 37 + 2].view(torch.float16).float()) == float(o["hi"][r, c])      # row 2 = first row of pair 1
            assert pair[4 * 128 + 0 * 128 + 0 * 64 + 0 * 16 + 1 * 8 + 5] == o["ql8"].view(torch.uint8)[r, c]      # chunk 0, row 0 of the pair, group 0, second k-tile, byte 5
            assert bool((by[1, 2 * 128:4 * 128] == 0).all()), "the missing partner of an odd last row is zero"
