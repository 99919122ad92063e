"""Torch restatement of the top-K of a pixel (csrc/softmax_px.h: TopkPx -- rank 0 the class the map names, rank r >= 1 the largest remaining float32
probability, the lowest class among equal ones, 255 / 0 from rank C on and where the map is 255), operation by operation as the kernels perform it, the
float64 probabilities and their stable order on the same float32 logits, and the three checks against them -- TEST INFRASTRUCTURE ONLY.  Nothing here is
measured: the bound is the one DESIGN.md section 2 derives for one softmax element."""
import numpy as np
import torch

from tests import uncertainty_ref as UR

NONE = 255


def topk(p, bi, K, slots=None):
    """p float32 [B, C, H, W] probabilities, bi int64 [B, H, W] the class the map names (>= C: a pixel without a class) -> (classes uint8 [K, B, H, W],
    probs float32 [K, B, H, W]).  The rank list of S >= K slots (2 / 4 / 8, the smallest that holds K), empty = class 255 with -1; per class in class order:
    bi goes to slot 0, any other class in front of the first slot of 1 .. S-1 it beats with `>`, the slots behind move down by one."""
    assert p.dtype == torch.float32 and 1 <= K <= 8
    C = p.shape[1]
    S = slots or (2 if K <= 2 else 4 if K <= 4 else 8)
    tp = [torch.full_like(p[:, 0], -1.0) for _ in range(S)]
    tc = [torch.full_like(bi, NONE) for _ in range(S)]
    for c in range(C):
        pc, cc = p[:, c], torch.full_like(bi, c)
        is_bi = bi == c
        tp[0], tc[0] = torch.where(is_bi, pc, tp[0]), torch.where(is_bi, cc, tc[0])
        for q in range(S - 1, 0, -1):
            inside = ~is_bi & (pc > tp[q])
            here = torch.ones_like(inside) if q == 1 else ~(pc > tp[q - 1])
            tp[q] = torch.where(inside, torch.where(here, pc, tp[q - 1]), tp[q])
            tc[q] = torch.where(inside, torch.where(here, cc, tc[q - 1]), tc[q])
    none = bi >= C
    classes = torch.stack([torch.where(none, torch.full_like(bi, NONE), tc[q]) for q in range(K)])
    probs = torch.stack([torch.where(none | (tc[q] == NONE), torch.zeros_like(tp[q]), tp[q]) for q in range(K)])
    return classes.to(torch.uint8), probs


def by_sort(p, bi, K):
    """The same by definition: a stable descending sort of the probabilities with bi moved to the front; ranks >= C are 255 / 0."""
    B, C, H, W = p.shape
    order = torch.sort(p, dim=1, descending=True, stable=True).indices                   # equal values keep class order
    last = order.permute(0, 2, 3, 1)                                                      # classes last: the mask below keeps C - 1 of every pixel, in order
    rest = last[last != bi.unsqueeze(-1)].reshape(B, H, W, C - 1).permute(0, 3, 1, 2) if C > 1 else order[:, :0]
    full = torch.cat([bi.unsqueeze(1), rest], dim=1)                                      # [B, C, H, W]
    vals = p.gather(1, full)
    classes = torch.full((K, B, H, W), NONE, dtype=torch.int64)
    probs = torch.zeros((K, B, H, W), dtype=torch.float32)
    n = min(K, C)
    classes[:n] = full[:, :n].permute(1, 0, 2, 3)
    probs[:n] = vals[:, :n].permute(1, 0, 2, 3)
    return classes.to(torch.uint8), probs


def restated(x, K, it=None):
    """Both steps on float32 logits [B, C, H, W]: the probabilities of tests/uncertainty_ref.py, bi = the first maximum of the LOGITS, the rank list."""
    return topk(UR.probabilities(x, it), UR.first_argmax(x), K)


def float64_probabilities(x, it=None):
    """float64 softmax of float32 logits [B, C, H, W] (at float64(x) * float64(float32 it)) and the spread D (tempered: D_T) per pixel."""
    z = x.double().cpu()
    if it is not None:
        z = z * float(np.float64(np.float32(it)))
    return torch.softmax(z, dim=1), (z - z.max(1, keepdim=True).values).abs().max(1).values


def eps_of(D, C, tempered=False):
    """The relative bound of one probability, DESIGN.md section 2: (2 D + C + 4) 2^-23, tempered (4 D_T + C + 4) 2^-23."""
    return ((4 if tempered else 2) * D + C + 4) * 2.0 ** -23


def undecided(P, eps, K):
    """Pixels whose float64 order is within the bound of a swap among the first min(K, C - 1) gaps -> bool [B, H, W].  P float64 [B, C, H, W], eps [B, H, W]."""
    C = P.shape[1]
    s = torch.sort(P, dim=1, descending=True, stable=True).values
    n = min(K, C - 1)
    if n < 1:
        return torch.zeros_like(eps, dtype=torch.bool)
    gap, both = s[:, :n] - s[:, 1:n + 1], s[:, :n] + s[:, 1:n + 1]
    return ~(gap > eps.unsqueeze(1) * both).all(1)


def float64_check(classes, probs, P, eps, K, covered=None):
    """The device's planes against the float64 probabilities P [B, C, H, W] of the same logits with the relative bound eps [B, H, W] per pixel; no pixel
    is left out of (a) and (b) but the uncovered ones (`covered` False), which must be 255 / 0:
      (a) every probs[r] within eps of P[class named at rank r]           -> worst error / bound
      (b) the order is a valid order within the bound                     -> number of violations
      (c) exact equality with the float64 stable order on decided pixels  -> (mismatches on decided pixels, undecided share)"""
    cls, pr = classes.cpu().long(), probs.cpu().double()
    B, C, H, W = P.shape
    n = min(K, C)
    ok = torch.ones(B, H, W, dtype=torch.bool) if covered is None else covered.cpu()
    assert bool((cls[:, ~ok] == NONE).all()) and bool((pr[:, ~ok] == 0).all())
    assert bool((cls[n:] == NONE).all()) and bool((pr[n:] == 0).all())
    safe = cls[:n].clamp_max(C - 1)
    named = P.gather(1, safe.permute(1, 0, 2, 3)).permute(1, 0, 2, 3)                     # [n, B, H, W]
    assert bool((cls[:n][:, ok] < C).all())
    rel = ((pr[:n] - named).abs() / named)[:, ok]
    worst = float((rel / eps[ok].unsqueeze(0)).max())
    bad = 0
    for r in range(n - 1):
        bad += int((named[r] < named[r + 1] - eps * (named[r] + named[r + 1]))[ok].sum())
    ranked = torch.zeros(B, C, H, W, dtype=torch.bool).scatter_(1, safe.permute(1, 0, 2, 3), True)
    last = named[n - 1].unsqueeze(1)
    bad += int(((P > last + eps.unsqueeze(1) * (P + last)) & ~ranked)[ok.unsqueeze(1).expand(-1, C, -1, -1)].sum())
    und = undecided(P, eps, K)
    order = torch.sort(P, dim=1, descending=True, stable=True).indices[:, :n].permute(1, 0, 2, 3)
    decided = ok & ~und
    wrong = int((cls[:n] != order)[:, decided].sum())
    return worst, bad, wrong, float(und[ok].double().mean()) if bool(ok.any()) else 0.0


def rank_counts(classes, labels, lut, C, ymap=None, xmap=None, slots=None, n_slots=None):
    """numpy restatement of mmsa_eval_topk_u8: classes uint8 [K, B, H, W], labels uint8 [B, Hl, Wl], lut uint8 [256] -> int64 [n_slots, C, K + 1]."""
    K, B, H, W = classes.shape
    slots = list(range(B)) if slots is None else list(slots)
    out = np.zeros((n_slots or max(slots) + 1, C, K + 1), dtype=np.int64)
    Hl, Wl = labels.shape[1:]
    ys = np.arange(H) if ymap is None else np.clip(ymap, 0, Hl - 1)
    xs = np.arange(W) if xmap is None else np.clip(xmap, 0, Wl - 1)
    for b in range(B):
        l = lut[labels[b][np.ix_(ys, xs)]].astype(np.int64)
        take = l < C
        hit = classes[:, b].astype(np.int64) == l[None]
        r = np.where(hit.any(0), hit.argmax(0), K)
        np.add.at(out[slots[b]], (l[take], r[take]), 1)
    return out
