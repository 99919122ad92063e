"""mmsa_gfe_qkv_conv (csrc/gfe_qkv.hip): the GFE's grouped 1x1 and 3x3 qkv convs as one grouped 3x3 conv with weights folded at pack time, against
the SEQUENTIAL two convs in float64 on the CPU.  Bound per element: 64 * 2^-24 * (|x| conv |W_eff|) -- one rounding of W_eff to fp32 plus the fp32
accumulation of the products, with slack for the matrix pipe's summation order -- and never more than twice the error of the two-launch path."""
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
G = 32


@pytest.fixture(scope="module")
def ops():
    import mmsa
    return mmsa.ops


_CASES = {}


def _case(c, B, H, W):
    """Inputs, module weights, the float64 reference and the bound's denominator: computed once per shape, shared, never written to."""
    key = (c, B, H, W)
    if key not in _CASES:
        gen = torch.Generator().manual_seed(1000 + c + 7 * H + W)
        x = torch.randn(B, c, H, W, generator=gen)
        q1 = torch.randn(3 * c, c // G, 1, 1, generator=gen) / (c // G) ** 0.5
        q2 = torch.randn(3 * c, 3 * c // G, 3, 3, generator=gen) / (27 * c // G) ** 0.5
        xd, q1d, q2d = x.double(), q1.double(), q2.double()
        ref = F.conv2d(F.conv2d(xd, q1d, groups=G), q2d, padding=1, groups=G)
        co, ci = 3 * c // G, c // G
        weff = torch.einsum("gmi,gomhw->goihw", q1d.reshape(G, co, ci), q2d.reshape(G, co, co, 3, 3)).reshape(3 * c, ci, 3, 3)
        mag = F.conv2d(xd.abs(), weff.abs(), padding=1, groups=G)
        nhwc = lambda t: t.permute(0, 2, 3, 1).reshape(B * H * W, -1).contiguous()   # noqa: E731
        _CASES[key] = dict(x=nhwc(x), q1=q1, q2=q2, ref=nhwc(ref), mag=nhwc(mag))
    return _CASES[key]


def _packed(case, c):
    from mmsa.backbone import fold_gfe_qkv
    co, ci = 3 * c // G, c // G
    q1p = case["q1"].reshape(G, co, ci, 1).permute(0, 3, 2, 1).contiguous().to(DEV)     # as backbone._pack lays them out
    q2p = case["q2"].reshape(G, co, co, 9).permute(0, 3, 2, 1).contiguous().to(DEV)
    return q1p, q2p, fold_gfe_qkv(case["q1"], case["q2"]).to(DEV)


def _two_launch(ops, x, q1p, q2p, out, B, H, W, c):
    mid = torch.empty(B * H * W, 3 * c, device=DEV)
    ops.gconv(x, q1p, None, mid, B, H, W, G, c // G, 3 * c // G, 1)
    ops.gconv(mid, q2p, None, out, B, H, W, G, 3 * c // G, 3 * c // G, 3)


def _check(ops, c, B, H, W, ldx=None, ldy=None, covered=True):
    case = _case(c, B, H, W)
    q1p, q2p, w12 = _packed(case, c)
    P = B * H * W
    ldx, ldy = ldx or c, ldy or 3 * c
    xbuf = torch.full((P, ldx), float("nan"), device=DEV)
    x = xbuf[:, ldx - c:]
    x.copy_(case["x"])
    outs = []
    for _ in range(2):
        ybuf = torch.full((P, ldy), -7.0, device=DEV)
        y = ybuf[:, (ldy - 3 * c) // 2:(ldy - 3 * c) // 2 + 3 * c]
        done = ops.gfe_qkv(x, w12, y, B, H, W, G, c // G, 3 * c // G)
        assert done == covered
        if not done:   # not covered: nothing was launched, the caller keeps the two launches
            torch.cuda.synchronize()
            assert bool((ybuf == -7.0).all())
            _two_launch(ops, x, q1p, q2p, y, B, H, W, c)
        torch.cuda.synchronize()
        rest = ybuf.clone()
        rest[:, (ldy - 3 * c) // 2:(ldy - 3 * c) // 2 + 3 * c] = -7.0
        assert bool((rest == -7.0).all()), "wrote outside its columns"
        outs.append(y.cpu())
    assert torch.equal(outs[0], outs[1]), "two runs differ"
    two = torch.empty(P, 3 * c, device=DEV)
    _two_launch(ops, x, q1p, q2p, two, B, H, W, c)
    err = (outs[0].double() - case["ref"]).abs()
    err2 = (two.cpu().double() - case["ref"]).abs()
    bound = 64 * 2.0 ** -24 * case["mag"]
    worst = float((err / bound.clamp_min(1e-300)).max())
    print(f"gfe_qkv c={c} {B}x{H}x{W} ld {ldx}/{ldy}: max err {float(err.max()):.3e} (two launches {float(err2.max()):.3e}), worst err / bound {worst:.3f}")
    assert torch.isfinite(outs[0]).all()
    assert bool((err <= bound).all()), f"worst err / bound {worst:.3f}"
    assert float(err.max()) <= 2 * float(err2.max())


@pytest.mark.parametrize("c", [96, 192, 384, 768])
def test_ragged_tiles_and_borders(ops, c):
    """cin_g -> cout_g = 3 -> 9, 6 -> 18, 12 -> 36, 24 -> 72; 20 x 18: two tile rows and columns, both ragged, every border."""
    _check(ops, c, 2, 20, 18)


def test_one_full_tile(ops):
    _check(ops, 96, 1, 16, 16)


def test_column_slices_of_wider_buffers(ops):
    """ldx > c and ldy > 3c: input and output are column slices (at odd offsets) of wider buffers, whose other columns stay as they were."""
    _check(ops, 192, 2, 20, 18, ldx=192 + 37, ldy=576 + 50)


@pytest.mark.parametrize("B", [2, 4])
def test_chunk_runs_equal_single_chunks_bitwise(ops, B):
    """Only a launch of >= 1024 workgroups lets a workgroup walk a run of 2 (B = 2) or 4 (B = 4) 24-channel chunks: the 1/4-resolution level of the
    1024^2 models, c = 96 on 256 x 256.  A chunk's arithmetic does not depend on the run it is in, so the launch must equal, bit for bit, four
    launches over one chunk each (8 of the 32 groups, as column slices): the path the tests above hold against float64."""
    from mmsa.backbone import fold_gfe_qkv
    c, H, W = 96, 256, 256
    gen = torch.Generator().manual_seed(77)
    q1 = torch.randn(3 * c, c // G, 1, 1, generator=gen)
    q2 = torch.randn(3 * c, 3 * c // G, 3, 3, generator=gen) / 9
    w12 = fold_gfe_qkv(q1, q2).to(DEV)
    x = torch.randn(B * H * W, c, device=DEV, generator=torch.Generator(DEV).manual_seed(78))
    whole = torch.full((B * H * W, 3 * c), float("nan"), device=DEV)
    parts = torch.full((B * H * W, 3 * c), float("nan"), device=DEV)
    assert ops.gfe_qkv(x, w12, whole, B, H, W, G, 3, 9)
    for j in range(4):
        assert ops.gfe_qkv(x[:, 24 * j:24 * j + 24], w12[8 * j:8 * j + 8], parts[:, 72 * j:72 * j + 72], B, H, W, 8, 3, 9)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(whole).all()) and torch.equal(whole, parts)


def test_uncovered_width_keeps_the_two_launches(ops):
    """c = 32 (one channel per group, the tiny test models): the entry reports 'not covered', launches nothing, and the two-launch path is right."""
    _check(ops, 32, 2, 20, 18, covered=False)
