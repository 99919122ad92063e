"""CPU companion of tests/test_persistent_walks_gpu.py: what that file relies on before anything reaches a GPU.

  * the shape helpers return, at 64, 104, 256 and 304 CUs, batches that meet every trip count the GPU tests claim (each GPU test asserts the same on its device);
  * for every bounded case at n = 256, torch's own fp32 evaluation stays inside the float64 bound and ONE border element moved by 8x its bound is rejected
    (the pattern of tests/test_kernel_variants_cpu.py: the bound is consistent with plain fp32 arithmetic, and nothing is averaged away);
  * the im2col restatement is the unfold it claims to be;
  * for the attention seeds and geometries at n = 256, the float64 max |logit| is at least 4 in EVERY image -- check_leaf's precondition -- on the fp32 operands
    and on their fp16 roundings (what the all-fp16 form of the kernel reads)."""
import pytest
import torch
import torch.nn.functional as F

from tests import test_attention_gpu as A
from tests import test_persistent_walks_gpu as P
from tests import variant_ref as V

CUS = (64, 104, 256, 304)
N = 256          # the MI355X


@pytest.mark.parametrize("n", CUS)
def test_window_batches_meet_their_trip_counts(n):
    for geom, (H, W, ws, heads, _) in P.WATTN.items():
        B, items = P.walk_shape(geom, n)
        per = P.wattn_windows(H, W, ws)[0] * heads
        assert items == per * B
        for grid in P.wattn_grids(items, n):
            trips = P.walk_of(geom, B, grid)[0]
            assert grid <= n and sum(t * c for t, c in trips.items()) == items
            assert max(trips) >= (2 if geom == "ws7_mixed" else 3)
        if geom == "ws7_mixed":
            assert n < items < 2 * n and per * (B - 1) <= n
        elif geom == "ws7_h3":
            assert items >= 2 * n + 1 and B - P.cdiv(2 * n + 1, per) < 8
        else:
            assert items >= 2 * n + 1 > per * (B - 1), "not the smallest batch"
    assert (P.wattn_windows(23, 31, 7), P.wattn_windows(30, 30, 14)) == ((20, 12), (9, 4))


def test_window_batches_on_256_cus():
    """The figures the issue names: B = 13 (520 items) and B = 29 (522 items), at most 26 100 token rows; and what a workgroup's list mixes on that part."""
    assert [P.wattn_batch(g, N) for g in ("ws7", "ws14", "ws7_h3", "ws7_mixed")] == [13, 29, 10, 5]
    assert max(P.wattn_batch(g, N) * H * W for g, (H, W, _, _, _) in P.WATTN.items()) == 26100
    facts = {g: P.walk_facts(g, N) for g in P.WATTN}
    # the restated cost model's pick: 174 workgroups (three trips each, two of them two) for ws7, 200 for its three-head form, one per CU for the other two
    assert [facts[g][2] for g in ("ws7", "ws14", "ws7_h3", "ws7_mixed")] == [174, 256, 200, 256]
    assert facts["ws7_mixed"][3] == {1: 212, 2: 44}
    # two heads and even grids: the head never changes inside a workgroup's list -- what the three-head cases are for
    assert facts["ws7"][4]["head_changes"] == 0 and facts["ws14"][4]["head_changes"] == 0
    for g in ("ws7_h3", "ws7_mixed"):
        assert facts[g][4]["head_changes"] > 0 and facts[g][4]["image_changes"] > 0
    B, items = P.walk_shape("ws7_h3", N)
    assert (B, items, P.wattn_grids(items, N)) == (10, 600, (200, 256))
    for grid in P.wattn_grids(items, N):          # every workgroup changes head on every trip, whichever grid runs
        trips, mix = P.walk_of("ws7_h3", B, grid)
        assert mix["head_changes"] == items - grid


@pytest.mark.parametrize("n", CUS)
def test_dwconv7_batches_meet_their_trip_counts(n):
    B = P.dw7_batch(n)
    for ipg in (0, B // 2):
        Bn, nt, grid, trips, sub = P.dw7_facts(n, ipg)
        assert Bn == B and nt == 6 * B and grid == 2 * n and sum(t * c for t, c in trips.items()) == nt
        assert B % 2 == 0 and nt >= 4 * n + 1 and nt % 8 and max(trips) >= 3 and sub == (2 * n) // 6
    smaller = [b for b in range(2, B, 2) if 6 * b >= 4 * n + 1 and (6 * b) % 8]
    assert not smaller, "not the smallest even batch past twice the grid with a tile count that is no multiple of 8"
    if n == N:
        assert B == 174 and B * 96 * 32 * 16 * 4 < 50e6


def test_xcd_order_restatement_is_a_permutation():
    for total in (1, 7, 8, 9, 276, 1044):
        assert sorted(P.xcd_order(i, total) for i in range(total)) == list(range(total))
    assert [P.xcd_order(i, 17) for i in (0, 1, 8, 15, 16)] == [0, 2, 1, 15, 16]


def test_grid_stride_shapes_pass_their_caps():
    for op in P.STRIDE:
        rest = P.stride_facts(op, 4 if op == "gelu_gate" else 2)
        assert 0 < rest < P.STRIDE[op][2] * 256
    p = P.IM2COL
    assert p["Kpad"] > p["Cin"] * p["p"] ** 2 and P.STRIDE["im2col"][3] > 4194304


_CASES = P.bounded_cases(N)


@pytest.mark.parametrize("cid,op,p", _CASES, ids=[c[0] for c in _CASES])
def test_bound_admits_fp32_and_rejects_one_bad_element(cid, op, p):
    make, ref = V.OPS[op]
    i = make(p, V.gen_for(cid))
    r, bnd = ref(V.cast(i, torch.float64), p)
    bnd = bnd.double()
    assert r.dtype == torch.float64 and r.shape == bnd.shape
    assert bool(torch.isfinite(r).all()) and bool(torch.isfinite(bnd).all()) and bool((bnd >= 0).all())
    y = V.fp32_eval(op, i, p)
    assert y.dtype == torch.float32
    V.assert_inside(y, r, bnd, cid + " (torch fp32 on the CPU)")
    del y
    flat_b = bnd.flatten()
    cand = [k for k in (0, flat_b.numel() - 1) if float(flat_b[k]) > 0]
    assert cand, "no border element with a bound > 0"
    for k in cand:
        bad = r.clone().flatten()
        bad[k] += 8 * flat_b[k]
        assert int(V.violations(bad.view_as(r), r, bnd).sum()) == 1
        with pytest.raises(AssertionError):
            V.assert_inside(bad.view_as(r), r, bnd, cid)


def test_im2col_restatement_is_unfold():
    p = dict(B=2, Ctot=4, c0=1, Cin=3, H=12, W=8, p=4, Kpad=64)
    x = torch.randn(p["B"], p["Ctot"], p["H"], p["W"], generator=V.gen_for("im2col-small"))
    want = F.unfold(x[:, 1:4], kernel_size=4, stride=4).transpose(1, 2).reshape(-1, 48)       # [B, C k k, L] -> [(b, ph, pw), (c, kh, kw)]
    got = P.im2col_ref(x, p)
    assert torch.equal(got[:, :48], want) and bool((got[:, 48:] == 0).all()) and got.shape == (12, 64)


@pytest.mark.parametrize("geom", list(P.WATTN))
def test_every_image_has_a_peaked_softmax(geom, monkeypatch):
    """check_leaf refuses a problem whose max |logit| is below 4 (a near-uniform softmax cannot see a scale or rel-pos error).  If a seed fails here, change the
    seed in WATTN, not the threshold."""
    monkeypatch.setattr(A, "DEV", "cpu")                       # ref_attention evaluates where test_attention_gpu.DEV says
    H, W, ws, heads, seed = P.WATTN[geom]
    B, T = P.wattn_batch(geom, N), H * W
    qkv, bias, rph, rpw = A.make_problem(B, H, W, heads, P.HD, ws, seed)
    f16 = lambda t: t.half().double()                          # noqa: E731
    low = []
    for b in range(B):
        q = qkv[b * T:(b + 1) * T]
        a32 = A.ref_attention(q.double(), bias.double(), rph.double(), rpw.double(), 1, H, W, heads, P.HD, ws, P.HD ** -0.5)[1]
        a16 = A.ref_attention(f16(q), f16(bias), f16(rph), f16(rpw), 1, H, W, heads, P.HD, ws, P.HD ** -0.5)[1]
        low.append(min(a32, a16))
    print(f"{geom}: max |logit| per image {min(low):.2f} .. {max(low):.2f}")
    assert min(low) >= 4.0, f"{geom}: image {low.index(min(low))} has max |logit| {min(low):.2f} < 4"
