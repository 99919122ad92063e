"""numpy restatement of the segment passes (mmsa_components_u8, mmsa_component_area, mmsa_suppress_small_u8, mmsa_eval_segments), written
from the definitions on the WHOLE image -- no tiles, no borders to merge, no waves -- TEST INFRASTRUCTURE ONLY.

  two pixels of one image are connected iff they are 4- or 8-neighbours and hold the same code; root(p) = the smallest y * W + x of p's component
  area[r] = the pixels of the component at its root r, 0 elsewhere;  suppressed[p] = fill where area[root(p)] < min_area, pred[p] elsewhere
  over every pixel whose own label code L is not 255, P = min(pred, C):  area0[root_label(p)] += 1, area1[root_pred(p)] += 1, and the hits likewise where
  L < C and P == L;  every root with area > 0 and code c < C adds 1 at [slot, side, c, min(23, floor(log2 area)), floor(bins * hit / area)]

`roots` lowers every pixel to the smallest label among its equal neighbours, hangs the label it held before under the new one, and then replaces every label by
its label's label until nothing moves: a serpentine of n pixels takes about log n rounds, not n.  tests/test_components_cpu.py holds it to scipy.ndimage.label."""
import numpy as np

from tests import boundary_ref as BR

SIZE_BUCKETS = 24
HALF = {4: ((0, 1), (1, 0)), 8: ((0, 1), (1, 0), (1, 1), (1, -1))}      # every neighbour pair once: (dy, dx) with its mirror


def _pair(H, W, dy, dx):
    """The slices (a, b) with b = a shifted by (dy, dx), dy >= 0."""
    ya, yb = slice(0, H - dy), slice(dy, H)
    xa, xb = (slice(0, W - dx), slice(dx, W)) if dx >= 0 else (slice(-dx, W), slice(0, W + dx))
    return (ya, xa), (yb, xb)


def roots(code, connectivity=8):
    """int32 [H, W] for the codes [H, W] of one image."""
    code = np.asarray(code)
    H, W = code.shape
    lab = np.arange(H * W, dtype=np.int64)
    pairs = [(a, b, code[a] == code[b]) for a, b in (_pair(H, W, dy, dx) for dy, dx in HALF[connectivity])]
    while True:
        grid = lab.reshape(H, W)
        low = grid.copy()
        for a, b, same in pairs:
            low[a] = np.where(same, np.minimum(low[a], grid[b]), low[a])
            low[b] = np.where(same, np.minimum(low[b], grid[a]), low[b])
        new = low.ravel().copy()
        np.minimum.at(new, lab, low.ravel())          # what a pixel pointed at follows it down
        while True:
            up = new[new]
            if np.array_equal(up, new):
                break
            new = up
        if np.array_equal(new, lab):
            return lab.reshape(H, W).astype(np.int32)
        lab = new


def roots_batch(codes, connectivity=8):
    return np.stack([roots(c, connectivity) for c in codes])


def areas(root):
    """int32 [..., H, W]: the component's pixel count at its root, 0 elsewhere."""
    root = np.asarray(root)
    H, W = root.shape[-2:]
    flat = root.reshape(-1, H * W)
    return np.stack([np.bincount(r, minlength=H * W) for r in flat]).reshape(root.shape).astype(np.int32)


def suppress(pred, C, min_area, connectivity=8, fill=255):
    """uint8 [B, H, W]: pred without the components (of min(pred, C)) below min_area."""
    out = []
    for p in np.asarray(pred):
        r = roots(np.minimum(p, C), connectivity)
        a = areas(r).ravel()[r]
        out.append(np.where(a < min_area, fill, p).astype(np.uint8))
    return np.stack(out)


def segment_planes(L, P, C, root_label, root_pred):
    """One image -> int64 [4, H, W]: area0, hit0 (label segments), area1, hit1 (prediction segments) at the root pixels."""
    H, W = L.shape
    keep = (L != BR.IGNORE).ravel()
    hit = keep & ((L < C) & (P == L)).ravel()
    out = np.zeros((4, H * W), dtype=np.int64)
    for k, (r, who) in enumerate(((root_label, keep), (root_label, hit), (root_pred, keep), (root_pred, hit))):
        out[k] = np.bincount(r.ravel()[who], minlength=H * W)
    return out.reshape(4, H, W)


def counts_from_planes(planes, L, P, C, bins):
    """int64 [2, C, 24, bins + 1] of one image."""
    out = np.zeros((2, C, SIZE_BUCKETS, bins + 1), dtype=np.int64)
    for side, code in ((0, L), (1, P)):
        area, hit = planes[2 * side].ravel(), planes[2 * side + 1].ravel()
        at = np.nonzero((area > 0) & (code.ravel() < C))[0]
        for i in at:
            a, h = int(area[i]), int(hit[i])
            out[side, int(code.ravel()[i]), min(SIZE_BUCKETS - 1, a.bit_length() - 1), bins * h // a] += 1
    return out


def segment_counts(pred, labels, lut, C, bins, connectivity=8, ymap=None, xmap=None, slots=None, n_slots=None):
    """pred uint8 [B, H, W], labels uint8 [B, Hl, Wl] -> (counts int64 [n_slots, 2, C, 24, bins + 1], planes int64 [4, B, H, W], root_pred, root_label int32
    [B, H, W]): everything one SegmentEvaluator.add() leaves behind, restated."""
    B = pred.shape[0]
    slots = list(range(B)) if slots is None else list(slots)
    counts = np.zeros((n_slots or max(slots) + 1, 2, C, SIZE_BUCKETS, bins + 1), dtype=np.int64)
    planes, rp, rl = [], [], []
    for b in range(B):
        L, P = BR.codes(pred[b], labels[b], lut, C, ymap, xmap)
        rl.append(roots(L, connectivity))
        rp.append(roots(P, connectivity))
        planes.append(segment_planes(L, P, C, rl[-1], rp[-1]))
        counts[slots[b]] += counts_from_planes(planes[-1], L, P, C, bins)
    return counts, np.stack(planes, 1), np.stack(rp), np.stack(rl)


# ---- the maps both test files share
def serpentine(H, W, a=1, b=2):
    """uint8 [H, W]: a one-pixel-wide path of code `a` that runs along every second row and turns at alternating ends, in a field of code `b`."""
    m = np.full((H, W), b, dtype=np.uint8)
    m[0::2] = a
    for k, y in enumerate(range(1, H, 2)):
        m[y, W - 1 if k % 2 == 0 else 0] = a
    return m


def spiral(H, W, a=1, b=2):
    """uint8 [H, W]: a one-pixel-wide rectangular spiral of code `a` from the corner inwards, one pixel of `b` between its turns."""
    m = np.full((H, W), b, dtype=np.uint8)
    y = x = d = turns = 0
    m[0, 0] = a
    free = lambda yy, xx: not (0 <= yy < H and 0 <= xx < W) or m[yy, xx] == b      # noqa: E731
    while turns < 2:
        dy, dx = ((0, 1), (1, 0), (0, -1), (-1, 0))[d]
        if 0 <= y + dy < H and 0 <= x + dx < W and m[y + dy, x + dx] == b and free(y + 2 * dy, x + 2 * dx):
            y, x, turns = y + dy, x + dx, 0
            m[y, x] = a
        else:
            d, turns = (d + 1) % 4, turns + 1
    return m


def comb(H, W, a=1, b=2):
    """uint8 [H, W]: teeth of code `a` in every second column that join only in the last row."""
    m = np.full((H, W), b, dtype=np.uint8)
    m[:, 0::2] = a
    m[H - 1] = a
    return m


def staircase(H, W, a=1, b=2):
    """uint8 [H, W]: the diagonal y == x (mod W) of code `a`: connected at 8, every pixel alone at 4."""
    m = np.full((H, W), b, dtype=np.uint8)
    y = np.arange(H)
    m[y, y % W] = a
    return m


def blocky(rng, H, W, C, lo=5, hi=40):
    """uint8 [H, W]: noise upsampled to blocks of a random size in lo .. hi."""
    by, bx = int(rng.integers(lo, hi + 1)), int(rng.integers(lo, hi + 1))
    coarse = rng.integers(0, C, size=((H + by - 1) // by, (W + bx - 1) // bx), dtype=np.uint8)
    return np.repeat(np.repeat(coarse, by, 0), bx, 1)[:H, :W].copy()
