"""Torch restatement of the two uncertainty scores (csrc/softmax_px.h: top-2 margin and entropy score, formed from the float32 probabilities of the
confidence paths) in float32, operation by operation, their float64 values on the same float32 logits, and the error bounds DESIGN.md section 2 derives
for them -- TEST INFRASTRUCTURE ONLY.  Nothing here is measured: the bounds come from the roundings counted there."""
import numpy as np
import torch

KINDS = {"margin": 1, "entropy": 2}


def inv_log_c(C):
    """float32(1 / log(float64(C))) as a float32 tensor; 0 for one class (what mmsa.evaluate.inv_log_classes hands to the launches)."""
    return torch.tensor(0.0 if C == 1 else float(np.float32(np.float64(1.0) / np.log(np.float64(C)))), dtype=torch.float32)


def first_argmax(x):
    """The class the map names: c == 0 or x_c > best, in class order -> int64 [B, H, W]."""
    best, bi = x[:, 0], torch.zeros_like(x[:, 0], dtype=torch.int64)
    for c in range(1, x.shape[1]):
        up = x[:, c] > best
        best, bi = torch.where(up, x[:, c], best), torch.where(up, torch.full_like(bi, c), bi)
    return bi


def probabilities(x, it=None):
    """x float32 [B, C, H, W] -> float32 probabilities, as csrc/softmax_px.h forms them: m in class order from x_0; e_c = exp(x_c - m), or
    exp((x_c - m) * it) with an inverse temperature (ONE float32 product); s = e_0, s += e_c in class order; p_c = e_c / s."""
    assert x.dtype == torch.float32
    C = x.shape[1]
    m = x[:, 0]
    for c in range(1, C):
        m = torch.where(x[:, c] > m, x[:, c], m)
    z = x - m.unsqueeze(1)
    if it is not None:
        z = z * torch.tensor(it, dtype=torch.float32)
    e = torch.exp(z)
    s = e[:, 0]
    for c in range(1, C):
        s = s + e[:, c]
    return e / s.unsqueeze(1)


def score(p, bi, kind):
    """p float32 [B, C, H, W] probabilities, bi int64 [B, H, W] the class the map names -> float32 [B, H, W]:
    margin:  p[bi] - p2, p2 = the largest p_c over c != bi in class order with `>` (the first such class starts it); one class: p[bi];
    entropy: max(0, 1 - H * ilc), H = t_0, H += t_c in class order, t_c = p_c > 0 ? -(p_c * log(p_c)) : 0."""
    assert p.dtype == torch.float32
    C = p.shape[1]
    if kind == "margin":
        pb = p.gather(1, bi.unsqueeze(1)).squeeze(1)
        p2, none = torch.zeros_like(pb), torch.ones_like(pb, dtype=torch.bool)
        for c in range(C):
            other = bi != c
            take = other & (none | (p[:, c] > p2))
            p2 = torch.where(take, p[:, c], p2)
            none = none & ~other
        return torch.where(none, pb, pb - p2)
    assert kind == "entropy"
    t = torch.where(p > 0, -(p * torch.log(torch.where(p > 0, p, torch.ones_like(p)))), torch.zeros_like(p))
    H = t[:, 0]
    for c in range(1, C):
        H = H + t[:, c]
    v = 1.0 - H * inv_log_c(C)
    return torch.where(v > 0, v, torch.zeros_like(v))


def restated(x, kind, it=None):
    """Both steps on float32 logits [B, C, H, W]: what every path writes (up to the last bits of exp and log, which are the device library's)."""
    return score(probabilities(x, it), first_argmax(x), kind)


def float64_scores(x, it=None):
    """The float64 scores of float32 logits (at float64(x) * float64(float32 it)) -> dict: margin = P_(1) - P_(2) (P alone for one class), entropy =
    max(0, 1 - H / log C) (1 for one class), and what the bounds need: p12 = P_(1) + P_(2), H, the spread D (tempered: D_T) per pixel."""
    z = x.double().cpu()
    if it is not None:
        z = z * float(np.float64(np.float32(it)))
    C = z.shape[1]
    p = torch.softmax(z, dim=1)
    top = p.topk(min(2, C), dim=1).values
    p1, p2 = top[:, 0], (top[:, 1] if C > 1 else torch.zeros_like(top[:, 0]))
    H = -(torch.where(p > 0, p * torch.log(torch.where(p > 0, p, torch.ones_like(p))), torch.zeros_like(p))).sum(1)
    ent = torch.ones_like(H) if C == 1 else (1.0 - H / np.log(float(C))).clamp_min(0.0)
    D = (z - z.max(1, keepdim=True).values).abs().max(1).values
    return dict(margin=p1 - p2, entropy=ent, p12=p1 + p2, H=H, D=D, C=C)


def bound(ref, kind, tempered=False):
    """The absolute bound of DESIGN.md section 2 per pixel, float64 [B, H, W].  eps = (2 D + C + 4) 2^-23 is the relative bound of one probability
    (tempered: (4 D_T + C + 4) 2^-23), margin for the quoted ulp of expf included.
    margin:  eps (P_(1) + P_(2)) + 2^-24                                   (both operands, the rounded subtraction of a value <= 1)
    entropy: (eps (H + 1) + (C + 2) 2^-24 H) / log C + 3 * 2^-24           (d(-p log p) = -(log p + 1) dp over the classes; logf within 1 ulp, doubled, and
                                                                            the product: 3 roundings per term; C - 1 additions of non-negative terms; then the
                                                                            rounding of ilc, of the product with it, and of the subtraction); 0 for one class."""
    C, D = ref["C"], ref["D"]
    eps = ((4 if tempered else 2) * D + C + 4) * 2.0 ** -23
    if kind == "margin":
        return eps * ref["p12"] + 2.0 ** -24
    if C == 1:
        return torch.zeros_like(D)
    return (eps * (ref["H"] + 1.0) + (C + 2) * 2.0 ** -24 * ref["H"]) / np.log(float(C)) + 3 * 2.0 ** -24


def float64_check(got, logits, kind, it=None):
    """got float32 [B, H, W] against the float64 score of the SAME float32 logits [B, C, H, W] -> (worst |error| / bound, largest D).  One class: the
    scores are exact, a pixel with any error counts as infinitely far out."""
    ref = float64_scores(logits, it)
    err = (got.double().cpu() - ref[kind]).abs()
    b = bound(ref, kind, tempered=it is not None)
    ratio = torch.where(b > 0, err / b.clamp_min(1e-300), torch.where(err > 0, torch.full_like(err, float("inf")), torch.zeros_like(err)))
    return ratio.max().item(), ref["D"].max().item()
