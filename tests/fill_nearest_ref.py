"""numpy restatement of the nearest-label fill (mmsa_fill_nearest_u8, csrc/fill.hip), a brute-force search over all sources for small
maps, and the cases the CPU and the GPU tests share -- TEST INFRASTRUCTURE ONLY.

  role: 0 = source (every byte in neither list), 1 = hole, 2 = inert.  For a hole p: among the sources q of the image with d2 = |q - p|^2 <= cap^2 the one
  with the smallest key (d2, qy, qx); out[p] = M[q], d2[p] = d2.  None: out[p] = M[p], d2[p] = FAR.  Every other pixel: out[p] = M[p], d2[p] = 0.

`fill` is vectorised and separable.  Row pass: per pixel the nearest source of its row, the first argmin of |dx| in ascending qx (of a left and a right source
equally far the left one), found by a running maximum / minimum of the source columns.  Column pass: per hole the first argmin of dy^2 + g^2 over the rows in
ascending qy (a strict < while qy rises keeps the first).  `brute` compares the keys of all sources pair by pair."""
import functools
from collections import namedtuple

import numpy as np

FAR = 65535
BIG = 1 << 30                          # "none": above every index and every cap^2, and its square still fits int64
HOLES, INERT = (250, 255), (254,)      # the bytes of the shared cases: two hole bytes (the smaller one is the launch's none_byte), one inert byte
CLASSES = 25


def roles(hole=255, inert=()):
    r = np.zeros(256, dtype=np.uint8)
    r[np.asarray(hole, dtype=np.int64).reshape(-1)] = 1
    r[np.asarray(inert, dtype=np.int64).reshape(-1)] = 2
    return r


def row_pass(m, role):
    """One image -> (g int64 [H, W], v uint8 [H, W]): the distance along the row to the row's nearest source (BIG: the row has none) and its value."""
    H, W = m.shape
    src = role[m] == 0
    x = np.arange(W, dtype=np.int64)[None, :]
    left = np.maximum.accumulate(np.where(src, x, -1), axis=1)                       # the last source at or before x
    right = np.minimum.accumulate(np.where(src, x, BIG)[:, ::-1], axis=1)[:, ::-1]   # the first source at or behind x
    dl, dr = np.where(left >= 0, x - left, BIG), np.where(right < BIG, right - x, BIG)
    at = np.where(dl <= dr, left, right)                                             # equally far: the left one, the smaller qx
    g = np.minimum(dl, dr)
    v = np.take_along_axis(m, np.clip(at, 0, W - 1), axis=1)
    return g, v


def fill(m, hole=255, inert=(), cap=32):
    """uint8 [H, W] -> (out uint8 [H, W], d2 uint16 [H, W])."""
    m = np.asarray(m, dtype=np.uint8)
    H, W = m.shape
    role = roles(hole, inert)
    g, v = row_pass(m, role)
    ys, xs = np.nonzero(role[m] == 1)
    best, val = np.full(ys.size, BIG, dtype=np.int64), m[ys, xs].copy()
    reach = min(cap, H - 1)
    has = np.concatenate([(g < BIG).any(axis=1), [False]])                           # the rows that hold a source at all; index H (and -1): outside
    for dy in range(-reach, reach + 1):                                              # ascending qy
        yy = ys + dy
        sel = np.nonzero(has[np.clip(yy, -1, H)])[0]
        if sel.size == 0:
            continue
        y_, x_ = yy[sel], xs[sel]
        d = dy * dy + g[y_, x_] ** 2
        take = (d <= cap * cap) & (d < best[sel])
        best[sel[take]], val[sel[take]] = d[take], v[y_, x_][take]
    out, d2 = m.copy(), np.zeros((H, W), dtype=np.uint16)
    out[ys, xs] = val
    d2[ys, xs] = np.where(best < BIG, best, FAR)
    return out, d2


def fill_batch(maps, hole=255, inert=(), cap=32):
    """uint8 [B, H, W] -> (out, d2), image by image."""
    res = [fill(one, hole, inert, cap) for one in maps]
    return np.stack([r[0] for r in res]), np.stack([r[1] for r in res])


def brute(m, hole=255, inert=(), cap=32):
    """The same from the definition: every hole against every source, the keys compared as tuples."""
    m = np.asarray(m, dtype=np.uint8)
    role = roles(hole, inert)
    sy, sx = np.nonzero(role[m] == 0)
    out, d2 = m.copy(), np.zeros(m.shape, dtype=np.uint16)
    for py, px in zip(*np.nonzero(role[m] == 1)):
        keys = [((qy - py) ** 2 + (qx - px) ** 2, qy, qx) for qy, qx in zip(sy.tolist(), sx.tolist())]
        keys = [k for k in keys if k[0] <= cap * cap]
        if keys:
            k = min(keys)
            out[py, px], d2[py, px] = m[k[1], k[2]], k[0]
        else:
            d2[py, px] = FAR
    return out, d2


# ---- hand-made patterns: h = a hole, i = the inert byte
h, i = HOLES[1], INERT[0]
CROSS = np.array([[h, 1, h], [3, h, 4], [h, 2, h]], dtype=np.uint8)          # four sources at distance 1 of the centre: up wins; at cap 1 the result is
CROSS_FILLED = np.array([[1, 1, 1], [3, 1, 4], [3, 2, 4]], dtype=np.uint8)   # this: every corner has two sources at d2 = 1, the upper one or else the left one
DIAG = np.array([[i, i, 5], [i, h, i], [6, i, i]], dtype=np.uint8)           # up-right against down-left at d2 = 2: up-right, the smaller qy


def noise(H, W, seed, hole_share, inert_share=0.05):
    """25-class noise; `hole_share` of the pixels hold one of the two hole bytes, `inert_share` of the rest the inert byte."""
    rng = np.random.default_rng(seed)
    m = rng.integers(0, CLASSES, size=(H, W)).astype(np.uint8)
    u = rng.random((H, W))
    m[u < hole_share] = np.asarray(HOLES, dtype=np.uint8)[rng.integers(0, 2, size=(H, W))][u < hole_share]
    m[(u >= hole_share) & (u < hole_share + (1 - hole_share) * inert_share)] = INERT[0]
    return m


def sparse(H, W, seed, source_share):
    """Holes everywhere but at `source_share` of the pixels, which hold 25-class noise."""
    rng = np.random.default_rng(seed)
    m = np.full((H, W), HOLES[1], dtype=np.uint8)
    keep = rng.random((H, W)) < source_share
    m[keep] = rng.integers(0, CLASSES, size=(H, W)).astype(np.uint8)[keep]
    return m


def one_source(H, W, y, x, value=7):
    m = np.full((H, W), HOLES[1], dtype=np.uint8)
    m[y, x] = value
    return m


STACK = ("no hole", "all holes", "corner source", "centre source", "cross tiled", "diag tiled", "noise 5%", "noise 50%", "noise 95%")


def stack(H, W):
    """The nine maps of one shape, uint8 [9, H, W], in the order of STACK."""
    seed = 1000 * H + W
    nohole = noise(H, W, seed, 0.0)
    tiled = [np.tile(t, ((H + 2) // 3, (W + 2) // 3))[:H, :W] for t in (CROSS, DIAG)]
    return np.stack([nohole, np.full((H, W), HOLES[0], dtype=np.uint8), one_source(H, W, H - 1, 0), one_source(H, W, H // 2, W // 2), tiled[0], tiled[1],
                     noise(H, W, seed + 1, 0.05), noise(H, W, seed + 2, 0.5), noise(H, W, seed + 3, 0.95)])


Case = namedtuple("Case", "name build cap")      # build() -> uint8 [B, H, W]; hole = HOLES and inert = INERT in every case

# the smallest shapes at which each mechanism can fail: degenerate axes, the 64-column tile, a lane's piece going 1 -> 2 -> 3 pixels, the group of 4 rows, more
# than one block both ways, and row distances beyond 255 (which must never fill)
SHAPES = [(1, 1), (1, 131), (67, 1), (9, 63), (9, 64), (9, 65), (3, 255), (3, 256), (3, 257), (2, 513), (3, 70), (4, 70), (5, 70), (67, 131), (300, 520)]


def _batch2():
    return np.stack([noise(37, 90, 5, 0.5), np.full((37, 90), HOLES[1], dtype=np.uint8)])


CASES = [Case(f"stack {H}x{W} cap {cap}", functools.partial(stack, H, W), cap)
         for H, W in SHAPES for cap in ((3, 255) if H * W < 67 * 131 else (3, 20, 255))]
CASES += [Case(f"scan {H}x513 source at x = {x}", functools.partial(lambda H, x: one_source(H, 513, H // 2, x)[None], H, x), 255) for H in (1, 5) for x in (0, 512)]
CASES += [Case("partial 67x131 1% cap 4", lambda: sparse(67, 131, 11, 0.01)[None], 4),
          Case("full 67x131 1% cap 255", lambda: sparse(67, 131, 11, 0.01)[None], 255),
          Case("partial 300x520 0.05% cap 32", lambda: sparse(300, 520, 12, 0.0005)[None], 32),
          Case("batch of two", _batch2, 6)]
CASE = {c.name: c for c in CASES}
assert len(CASE) == len(CASES)


@functools.lru_cache(maxsize=None)
def maps_of(name):
    """The case's maps, read-only, built once."""
    m = np.ascontiguousarray(CASE[name].build())
    m.setflags(write=False)
    return m


@functools.lru_cache(maxsize=None)
def want_of(name):
    """The restated (out, d2) of the case, read-only, computed once."""
    out, d2 = fill_batch(maps_of(name), HOLES, INERT, CASE[name].cap)
    out.setflags(write=False)
    d2.setflags(write=False)
    return out, d2
