"""Torch restatement of the confidence map's rule (csrc/softmax_px.h; F.softmax(seg_logit, dim=1) of segmentors/encoder_decoder.py:449,460, its maximum
over the classes) in float32, operation by operation, and the inputs and the error bound the confidence tests share -- TEST INFRASTRUCTURE ONLY."""
import torch


def confidence(x):
    """x float32 [B, C, H, W] -> float32 [B, H, W]: m = max_c x_c from m = x_0; s = e_0, s += e_c in class order, e_c = exp(x_c - m); exp(m - m) / s."""
    assert x.dtype == torch.float32
    C = x.shape[1]
    m = x[:, 0]
    for c in range(1, C):
        m = torch.where(x[:, c] > m, x[:, c], m)
    s = torch.exp(x[:, 0] - m)
    for c in range(1, C):
        s = s + torch.exp(x[:, c] - m)
    return torch.exp(m - m) / s


def planted_logits(n, C, seed, hw=(16, 16)):
    """Head-resolution logits [n, C, h, w] = randn * 6; with more than one class, the first window's top-left logit is +15 in class 0 and -15 in class 1.
    That logit IS the frame's pixel (0, 0) wherever window 0 starts there and is its only window (the align_corners=False source coordinate of a window's
    first pixel is clamped to 0), so a pixel's spread D = max_c |x_c - m| reaches 30 whatever the noise does."""
    x = torch.randn(n, C, hw[0], hw[1], generator=torch.Generator().manual_seed(seed)) * 6.0
    if C > 1:
        x[0, 0, 0, 0], x[0, 1, 0, 0] = 15.0, -15.0
    return x


def float64_check(conf, logits):
    """conf float32 [B, H, W] against the float64 softmax of the SAME float32 logits [B, C, H, W] -> (worst relative error / bound, largest D).  The bound
    per pixel is (2 D + C + 4) 2^-23, D = max_c |x_c - m|: the one DESIGN.md section 2 derives for a softmax element and tests/test_aug_gpu.py asserts for
    the softmax kernel (one rounding of x - m entering the exponent, expf within 1 ulp, C - 1 additions of positive terms, one division; times 2 as margin for
    the quoted 1 ulp).  The confidence's numerator is exp(0) = 1 exactly, so it holds a fortiori."""
    x = logits.double().cpu()
    C = x.shape[1]
    want = torch.softmax(x, dim=1).max(1).values
    D = (x - x.max(1, keepdim=True).values).abs().max(1).values
    bound = (2 * D + C + 4) * 2.0 ** -23
    rel = (conf.double().cpu() - want).abs() / want
    return (rel / bound).max().item(), D.max().item()
