"""numpy restatement of the boundary counts (mmsa_eval_boundary_u8), written from the definition and independent of the kernel's form:
explicit shifts over the (2 d + 1)^2 window, a neighbour outside the image simply not looked at -- no separable pass, no min / max, no clamp trick
(`zones_clamped` below is the clamp form, kept apart so that a test can show the two agree) -- TEST INFRASTRUCTURE ONLY.

  L(p) = lut[label[ymap[y], xmap[x]]] normalised: a class < C, C (kept but out of range), 255 (ignored);   P(p) = min(pred[p], C)
  near_label(p) iff some pixel q of the image with max(|dy|, |dx|) <= d has L(q) != L(p); near_pred(p) the same for P
  border=True: a pixel with y < d, x < d, y >= H - d or x >= W - d is near on both sides
  counts[slot][2 * near_label + near_pred][min(L, C)][P] += 1 for every pixel whose own L is not 255"""
import numpy as np

IGNORE = 255


def codes(pred, label, lut, C, ymap=None, xmap=None):
    """One image: pred uint8 [H, W], raw label uint8 [Hl, Wl] -> (L, P) int64 [H, W]."""
    H, W = pred.shape
    Hl, Wl = label.shape
    ys = np.arange(H) if ymap is None else np.clip(np.asarray(ymap), 0, Hl - 1)
    xs = np.arange(W) if xmap is None else np.clip(np.asarray(xmap), 0, Wl - 1)
    l = np.asarray(lut)[label[np.ix_(ys, xs)]].astype(np.int64)
    L = np.where(l == IGNORE, IGNORE, np.minimum(l, C))
    return L, np.minimum(pred.astype(np.int64), C)


def near(code, d, border=False):
    """bool [H, W]: some pixel of the image within Chebyshev distance d holds another code.  One shifted comparison per offset of the window."""
    H, W = code.shape
    out = np.zeros((H, W), dtype=bool)
    for dy in range(-min(d, H - 1), min(d, H - 1) + 1):
        for dx in range(-min(d, W - 1), min(d, W - 1) + 1):
            if dy == 0 and dx == 0:
                continue
            # p = (y, x) with q = (y + dy, x + dx) inside the image
            ya, yb = max(0, -dy), min(H, H - dy)
            xa, xb = max(0, -dx), min(W, W - dx)
            out[ya:yb, xa:xb] |= code[ya:yb, xa:xb] != code[ya + dy:yb + dy, xa + dx:xb + dx]
    if border:
        out |= border_mask(H, W, d)
    return out


def near_loops(code, d, border=False):
    """The same by a double loop over the window of every pixel (slow: small maps only)."""
    H, W = code.shape
    out = np.zeros((H, W), dtype=bool)
    for y in range(H):
        for x in range(W):
            for qy in range(y - d, y + d + 1):
                for qx in range(x - d, x + d + 1):
                    if 0 <= qy < H and 0 <= qx < W and code[qy, qx] != code[y, x]:
                        out[y, x] = True
            if border and (y < d or x < d or y >= H - d or x >= W - d):
                out[y, x] = True
    return out


def near_clamped(code, d):
    """The clamp-to-edge form of border=False: every offset of the window is looked at, at the nearest pixel of the image."""
    H, W = code.shape
    out = np.zeros((H, W), dtype=bool)
    yy, xx = np.arange(H)[:, None], np.arange(W)[None, :]
    for dy in range(-d, d + 1):
        for dx in range(-d, d + 1):
            out |= code[np.clip(yy + dy, 0, H - 1), np.clip(xx + dx, 0, W - 1)] != code
    return out


def border_mask(H, W, d):
    y, x = np.arange(H)[:, None], np.arange(W)[None, :]
    return (y < d) | (x < d) | (y >= H - d) | (x >= W - d)


def zones(pred, label, lut, C, d, border=False, ymap=None, xmap=None):
    """One image -> (zone int64 [H, W], L, P)."""
    L, P = codes(pred, label, lut, C, ymap, xmap)
    return 2 * near(L, d, border).astype(np.int64) + near(P, d, border).astype(np.int64), L, P


def counts_of(zone, L, P, C):
    """int64 [4, C + 1, C + 1] of one image from its zones and codes."""
    keep = L != IGNORE
    idx = (zone[keep] * (C + 1) + np.minimum(L[keep], C)) * (C + 1) + P[keep]
    return np.bincount(idx, minlength=4 * (C + 1) ** 2).reshape(4, C + 1, C + 1).astype(np.int64)


def boundary_counts(pred, labels, lut, C, d, border=False, ymap=None, xmap=None, slots=None, n_slots=None):
    """pred uint8 [B, H, W], labels uint8 [B, Hl, Wl], lut uint8 [256] -> int64 [n_slots, 4, C + 1, C + 1] (mmsa_eval_boundary_u8, restated)."""
    B = pred.shape[0]
    slots = list(range(B)) if slots is None else list(slots)
    out = np.zeros((n_slots or max(slots) + 1, 4, C + 1, C + 1), dtype=np.int64)
    for b in range(B):
        z, L, P = zones(pred[b], labels[b], lut, C, d, border, ymap, xmap)
        out[slots[b]] += counts_of(z, L, P, C)
    return out


def boundary_iou(counts):
    """The Boundary IoU per class from int64 [4, C + 1, C + 1], by its definition, class by class."""
    C = counts.shape[-1] - 1
    out = np.full(C, np.nan)
    for c in range(C):
        G = int(counts[2, c, :].sum() + counts[3, c, :].sum())
        Pd = int(counts[1, :, c].sum() + counts[3, :, c].sum())
        I = int(counts[3, c, c])
        if G + Pd - I:
            out[c] = I / (G + Pd - I)
    return out
