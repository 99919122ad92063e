"""The GFE's qkv2(qkv1(x)) folded into one grouped 3x3 conv (mmsa.backbone.fold_gfe_qkv): the fold itself, in float64 on the CPU."""
import pytest
import torch
import torch.nn.functional as F

G = 32


def _weights(c, seed):
    gen = torch.Generator().manual_seed(seed)
    q1 = torch.randn(3 * c, c // G, 1, 1, generator=gen, dtype=torch.float64)
    q2 = torch.randn(3 * c, 3 * c // G, 3, 3, generator=gen, dtype=torch.float64)
    x = torch.randn(2, c, 5, 7, generator=gen, dtype=torch.float64)
    return q1, q2, x


def _fold64(q1, q2):
    """W_eff in the module's own layout [3c, c/G, 3, 3], float64, written independently of the packed form."""
    co, ci = q1.shape[0] // G, q1.shape[1]
    a = q1.reshape(G, co, ci)              # [g][m][ci]
    b = q2.reshape(G, co, co, 3, 3)        # [g][co][m][kh][kw]
    return torch.einsum("gmi,gomhw->goihw", a, b).reshape(G * co, ci, 3, 3)


@pytest.mark.parametrize("c", [96, 768])
def test_composition_is_a_grouped_3x3_conv(c):
    """conv2d(x, W_eff, padding=1, groups=32) == conv2d(conv2d(x, q1, groups=32), q2, padding=1, groups=32) to 1e-12 relative, borders included."""
    q1, q2, x = _weights(c, 5 + c)
    ref = F.conv2d(F.conv2d(x, q1, groups=G), q2, padding=1, groups=G)
    got = F.conv2d(x, _fold64(q1, q2), padding=1, groups=G)
    assert got.shape == ref.shape == (2, 3 * c, 5, 7)
    err = (got - ref).abs()
    assert float((err / ref.abs().max()).max()) <= 1e-12
    border = torch.ones(5, 7, dtype=torch.bool)
    border[1:-1, 1:-1] = False
    assert float(err[..., border].max() / ref[..., border].abs().max()) <= 1e-12


@pytest.mark.parametrize("c", [96, 768])
def test_packed_fold_is_the_float64_fold_rounded_once(c):
    """What the pack stores: [G][tap][ci][co] (the layout of the packed q2), fp32, each entry the float64 sum rounded once."""
    from mmsa.backbone import fold_gfe_qkv
    q1, q2, _ = _weights(c, 9 + c)
    w12 = fold_gfe_qkv(q1.float(), q2.float())
    assert w12.dtype == torch.float32 and tuple(w12.shape) == (G, 9, c // G, 3 * c // G) and w12.is_contiguous()
    want = _fold64(q1.float().double(), q2.float().double())                                  # [3c, ci, 3, 3]
    want = want.reshape(G, 3 * c // G, c // G, 9).permute(0, 3, 2, 1)                          # [G][tap][ci][co]
    # the two float64 sums may differ in their last bits (summation order); after the one rounding to fp32 they are within one ulp
    assert float(((w12.double() - want).abs() / want.abs().clamp_min(1e-30)).max()) <= 2.0 ** -23
    assert float(((w12.double() - want).abs()).max()) <= 2.0 ** -24 * float(want.abs().max())


def test_no_fold_with_a_qkv1_bias():
    """With a bias on qkv1 the zero padding of qkv2 no longer commutes with the 1x1 conv: the pack step refuses to fold."""
    from mmsa.backbone import fold_gfe_qkv
    q1, q2, x = _weights(96, 3)
    bias = torch.randn(3 * 96, dtype=torch.float64)
    assert fold_gfe_qkv(q1, q2, bias) is None
    assert fold_gfe_qkv(q1, q2, None) is not None
    # and the reason: the border of the composition differs from the folded conv's by the bias seen through the taps that fall outside
    ref = F.conv2d(F.conv2d(x, q1, bias, groups=G), q2, padding=1, groups=G)
    inner = F.conv2d(x, _fold64(q1, q2), padding=1, groups=G) + F.conv2d(bias.view(1, -1, 1, 1).expand(2, -1, 5, 7), q2, padding=1, groups=G)
    assert float((ref - inner).abs().max()) <= 1e-10 * float(ref.abs().max())
    full = F.conv2d(x, _fold64(q1, q2), padding=1, groups=G) + q2.sum((2, 3)).reshape(G, 9, 9).bmm(bias.reshape(G, 9, 1)).reshape(1, -1, 1, 1)
    assert float((ref - full)[..., 1:-1, 1:-1].abs().max()) <= 1e-10 * float(ref.abs().max())
    assert float((ref - full)[..., 0, :].abs().max()) > 1e-3
