"""Keeps the bound of tests/variant_ref.py honest, on the CPU, for every case of the table in tests/test_kernel_variants_gpu.py: torch's own fp32
evaluation of the same statement stays inside the bound (the float64 reference and the bound are consistent with plain fp32 arithmetic), and a
result with ONE border element moved by 8x its bound is rejected (the check is per element, nothing is averaged away)."""
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
    assert y.dtype == torch.float32 or op in ("colstats", "gram")       # (results the device itself returns as double)
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
