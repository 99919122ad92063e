"""numpy restatement of the Euclidean boundary passes (mmsa_boundary_distance_u8, mmsa_eval_boundary_d2, mmsa_eval_boundary_displacement),
written from the definition and independent of the kernel's form: per pixel the minimum of dy^2 + dx^2 over ALL pixels of another code, pair by pair -- no
separable pass, no row runs, no scipy -- TEST INFRASTRUCTURE ONLY.

  D2(p) = min over pixels q of the image with M(q) != M(p) of (qy - py)^2 + (qx - px)^2;  border=True: also <= db^2, db = min(y, x, H - 1 - y, W - 1 - x) + 1
  d2[p] = D2(p) where D2(p) <= cap^2, else FAR (65535)
  zone = 2 * (d2_label <= t) + (d2_pred <= t); counts[slot][zone][min(L, C)][P] += 1 for every pixel whose own L is not 255
  hist[slot][0][min(L, C)][k(d2_pred)] += 1 where d2_label <= 2, hist[slot][1][P][k(d2_label)] += 1 where d2_pred <= 2, for the same pixels;
  k(d2) = the smallest k >= 1 with k^2 >= d2, cap + 1 for FAR"""
import numpy as np

from tests import boundary_ref as BR

FAR = 65535
INF = np.iinfo(np.int64).max


def d2_full(code, border=False):
    """int64 [H, W]: the exact squared distance to the nearest pixel of another code, INF where the image holds one code (and border is False)."""
    code = np.asarray(code)
    H, W = code.shape
    yy, xx = np.mgrid[0:H, 0:W]
    yy, xx, flat = yy.ravel().astype(np.int64), xx.ravel().astype(np.int64), code.ravel()
    out = np.full(H * W, INF, dtype=np.int64)
    for c in np.unique(flat):
        mine, other = np.nonzero(flat == c)[0], np.nonzero(flat != c)[0]
        if other.size == 0:
            continue
        oy, ox = yy[other][None, :], xx[other][None, :]
        step = max(1, (1 << 22) // other.size)
        for i in range(0, mine.size, step):
            p = mine[i:i + step]
            out[p] = ((yy[p][:, None] - oy) ** 2 + (xx[p][:, None] - ox) ** 2).min(1)
    out = out.reshape(H, W)
    return np.minimum(out, border_d2(H, W)) if border else out


def border_d2(H, W):
    """int64 [H, W]: db^2, db = min(y, x, H - 1 - y, W - 1 - x) + 1, the distance to the first pixel outside the image."""
    y, x = np.arange(H, dtype=np.int64)[:, None], np.arange(W, dtype=np.int64)[None, :]
    db = np.minimum(np.minimum(y, x), np.minimum(H - 1 - y, W - 1 - x)) + 1
    return db * db


def capped(d, cap):
    """The cap / FAR rule: uint16, the distance where it is <= cap^2, FAR elsewhere."""
    return np.where(d <= cap * cap, d, FAR).astype(np.uint16)


def d2_map(code, cap, border=False):
    """uint16 [H, W]: what the distance launch writes for one image's codes."""
    return capped(d2_full(code, border), cap)


def k_of(d2, cap):
    """The bin of a uint16 distance: the smallest k >= 1 with k^2 >= d2, found among the squares themselves; cap + 1 for FAR."""
    d2 = np.asarray(d2).astype(np.int64)
    k = np.searchsorted(np.arange(cap + 1, dtype=np.int64) ** 2, d2, side="left")
    return np.where(d2 == FAR, cap + 1, k).astype(np.int64)


def maps(pred, label, lut, C, cap, border=False, ymap=None, xmap=None):
    """One image -> (d2_label, d2_pred uint16 [H, W], L, P)."""
    L, P = BR.codes(pred, label, lut, C, ymap, xmap)
    return d2_map(L, cap, border), d2_map(P, cap, border), L, P


def counts_from_maps(d2l, d2p, L, P, C, t):
    zone = 2 * (d2l.astype(np.int64) <= t).astype(np.int64) + (d2p.astype(np.int64) <= t).astype(np.int64)
    return BR.counts_of(zone, L, P, C)


def displacement_from_maps(d2l, d2p, L, P, C, cap):
    """int64 [2, C + 1, cap + 2] of one image."""
    out = np.zeros((2, C + 1, cap + 2), dtype=np.int64)
    keep = L != BR.IGNORE
    on_l, on_p = keep & (d2l <= 2), keep & (d2p <= 2)
    np.add.at(out[0], (np.minimum(L[on_l], C), k_of(d2p[on_l], cap)), 1)
    np.add.at(out[1], (P[on_p], k_of(d2l[on_p], cap)), 1)
    return out


def evaluate(pred, labels, lut, C, cap, t, border=False, ymap=None, xmap=None, slots=None, n_slots=None):
    """pred uint8 [B, H, W], labels uint8 [B, Hl, Wl] -> (counts int64 [n_slots, 4, C + 1, C + 1], hist int64 [n_slots, 2, C + 1, cap + 2],
    d2_pred, d2_label uint16 [B, H, W]): everything one EuclideanBoundaryEvaluator.add() leaves behind, restated."""
    B = pred.shape[0]
    slots = list(range(B)) if slots is None else list(slots)
    n = n_slots or max(slots) + 1
    counts = np.zeros((n, 4, C + 1, C + 1), dtype=np.int64)
    hist = np.zeros((n, 2, C + 1, cap + 2), dtype=np.int64)
    dp, dl = [], []
    for b in range(B):
        d2l, d2p, L, P = maps(pred[b], labels[b], lut, C, cap, border, ymap, xmap)
        counts[slots[b]] += counts_from_maps(d2l, d2p, L, P, C, t)
        hist[slots[b]] += displacement_from_maps(d2l, d2p, L, P, C, cap)
        dp.append(d2p)
        dl.append(d2l)
    return counts, hist, np.stack(dp), np.stack(dl)
