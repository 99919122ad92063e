"""numpy restatement of the majority filter (mmsa_majority_filter_u8, csrc/majority.hip), a brute-force version straight from the
definition for small maps, and the cases the CPU and the GPU tests share -- TEST INFRASTRUCTURE ONLY.

  role: 0 = voter, 1 = hole, 2 = inert.  Window of p: the pixels q of the image with |qy - py| <= r and |qx - px| <= r (clipped at the border, no padding).
  n_v(p) = voters of value v in the window, T = sum_v n_v, n_best = max_v n_v.  w(p) = the own value if p is a voter and n_own = n_best, else the smallest v
  with n_v = n_best.  Targets: the holes, with all = 1 the voters too.  out = w iff target and T > 0 and (not half or 2 n_best > T), else the input;
  support = n_best at a target, 0 elsewhere.

`votes` counts per value by box sums of the voter indicator (a 2-D cumulative sum) while v ascends; `apply` forms (out, support) from those counts for any
`all` / `half`.  `brute` loops over the pixels with a bincount of the clipped window."""
import functools
from collections import namedtuple

import numpy as np

VOTER, HOLE, INERT_ROLE = 0, 1, 2
HOLES, INERT = (250, 255), (254,)      # the bytes of the shared cases: two hole bytes, one inert byte
CLASSES = 25
Votes = namedtuple("Votes", "best value own total tied")      # int64 [H, W] each: n_best, the smallest v holding it, n_own (0 off the voters), T, how many v hold n_best


def roles(num_classes=None, hole=(), inert=()):
    r = np.zeros(256, dtype=np.uint8)
    if num_classes is not None:
        r[int(num_classes):] = INERT_ROLE
    r[np.asarray(hole, dtype=np.int64).reshape(-1)] = HOLE
    r[np.asarray(inert, dtype=np.int64).reshape(-1)] = INERT_ROLE
    return r


def box(ind, r):
    """int64 [H, W]: the sum of `ind` over the clipped (2 r + 1)^2 window of every pixel."""
    H, W = ind.shape
    c = np.zeros((H + 1, W + 1), dtype=np.int64)
    c[1:, 1:] = np.cumsum(np.cumsum(ind.astype(np.int64), axis=0), axis=1)
    y0, y1 = np.clip(np.arange(H) - r, 0, H), np.clip(np.arange(H) + r + 1, 0, H)
    x0, x1 = np.clip(np.arange(W) - r, 0, W), np.clip(np.arange(W) + r + 1, 0, W)
    return c[y1][:, x1] - c[y0][:, x1] - c[y1][:, x0] + c[y0][:, x0]


def votes(m, role, r):
    """One image uint8 [H, W] -> Votes."""
    m = np.asarray(m, dtype=np.uint8)
    voter = role[m] == VOTER
    z = np.zeros(m.shape, dtype=np.int64)
    best, value, own, total, tied = z.copy(), z.copy(), z.copy(), z.copy(), z.copy()
    for v in np.unique(m[voter]).tolist():                                         # ascending
        is_v = voter & (m == v)
        n = box(is_v, r)
        more = n > best                                                            # strict: the smallest of equals stays
        tied = np.where(more, 1, tied + ((n == best) & (n > 0)))
        best, value = np.where(more, n, best), np.where(more, v, value)
        own[is_v] = n[is_v]
        total += n
    return Votes(best, value, own, total, tied)


def apply(m, role, vt, all_=True, half=False):
    """(out uint8 [H, W], support uint16 [H, W]) of one image from its Votes."""
    m = np.asarray(m, dtype=np.uint8)
    ro = role[m]
    voter = ro == VOTER
    target = (ro == HOLE) | (voter & bool(all_))
    winner = np.where(voter & (vt.own == vt.best), m, vt.value)
    change = target & (vt.total > 0) & ((2 * vt.best > vt.total) | (not half))
    return np.where(change, winner, m).astype(np.uint8), np.where(target, vt.best, 0).astype(np.uint16)


def majority(m, role, r, all_=True, half=False):
    return apply(m, role, votes(m, role, r), all_, half)


def majority_batch(maps, role, r, all_=True, half=False):
    res = [majority(one, role, r, all_, half) for one in maps]
    return np.stack([a for a, _ in res]), np.stack([s for _, s in res])


def brute(m, role, r, all_=True, half=False):
    """The same from the definition, pixel by pixel."""
    m = np.asarray(m, dtype=np.uint8)
    H, W = m.shape
    out, support = m.copy(), np.zeros((H, W), dtype=np.uint16)
    for py in range(H):
        for px in range(W):
            ro = role[m[py, px]]
            if not (ro == HOLE or (ro == VOTER and all_)):
                continue
            win = m[max(py - r, 0):py + r + 1, max(px - r, 0):px + r + 1].ravel()
            n = np.bincount(win[role[win] == VOTER], minlength=256)
            T, nb = int(n.sum()), int(n.max())
            support[py, px] = nb
            if T == 0 or (half and not 2 * nb > T):
                continue
            out[py, px] = m[py, px] if (ro == VOTER and n[m[py, px]] == nb) else int(np.argmax(n))      # argmax: the first, the smallest v
    return out, support


# ---- the maps
def noise(H, W, seed, values=CLASSES, hole_share=0.03, inert_share=0.01):
    """Noise over the bytes 0 .. values - 1; `hole_share` of the pixels hold one of the two hole bytes, `inert_share` the inert byte."""
    rng = np.random.default_rng(seed)
    m = rng.integers(0, values, size=(H, W)).astype(np.uint8)
    u = rng.random((H, W))
    m[u < hole_share] = np.asarray(HOLES, dtype=np.uint8)[rng.integers(0, 2, size=(H, W))][u < hole_share]
    m[(u >= hole_share) & (u < hole_share + inert_share)] = INERT[0]
    return m


def patchy(H, W, seed, block=24):
    """A class map of patches with 8 % noise pixels, 5 % + 2 % hole bytes (250, 255) and 1.5 % of the inert byte (254)."""
    rng = np.random.default_rng(seed)
    coarse = rng.integers(0, CLASSES, size=((H + block - 1) // block + 1, (W + block - 1) // block + 1)).astype(np.uint8)
    dy, dx = (int(v) for v in rng.integers(0, block, size=2))
    m = np.kron(coarse, np.ones((block, block), dtype=np.uint8))[dy:dy + H, dx:dx + W].copy()
    u = rng.random((H, W))
    spots = rng.integers(0, CLASSES, size=(H, W)).astype(np.uint8)
    m[u < 0.08] = spots[u < 0.08]
    m[(u >= 0.08) & (u < 0.13)] = HOLES[0]
    m[(u >= 0.13) & (u < 0.15)] = HOLES[1]
    m[(u >= 0.15) & (u < 0.165)] = INERT[0]
    return m


def hole_block(H, W, seed, r):
    """3-value noise with a solid block of holes of 2 r + 3 pixels a side in the top-left corner: the block's core has no voter in its window."""
    m = noise(H, W, seed, 3, 0.0, 0.0)
    m[:2 * r + 3, :2 * r + 3] = HOLES[1]
    return m


STACK = ("noise 25", "noise 3", "noise 200", "patchy", "one value", "all holes", "hole block")
NOISY = ("noise 25", "noise 3", "noise 200", "patchy")      # the maps a filter of radius <= 3 must change in at least 1 % of the pixels (where="all")


def stack(H, W, r):
    """The seven maps of one shape, uint8 [7, H, W], in the order of STACK."""
    seed = 1000 * H + W
    return np.stack([noise(H, W, seed), noise(H, W, seed + 1, 3), noise(H, W, seed + 2, 200), patchy(H, W, seed + 3), np.full((H, W), 7, dtype=np.uint8),
                     np.full((H, W), HOLES[0], dtype=np.uint8), hole_block(H, W, seed + 4, r)])


# the role tables of the shared cases: with the class count every byte from 25 on that is no hole is inert (most of "noise 200"); without it, it votes
CONFIGS = {"C25": dict(num_classes=CLASSES, hole=HOLES, inert=INERT), "any": dict(num_classes=None, hole=HOLES, inert=INERT)}
MODES = [("all", False), ("all", True), ("holes", False), ("holes", True)]      # (where, half): every case runs all four

Case = namedtuple("Case", "name build radius config")      # build() -> uint8 [B, H, W]

# the smallest shapes at which each mechanism can fail: degenerate axes, an image thinner than the halo, the 64-column tile, the tile heights 16 (radius <= 8),
# 32 (radius <= 16) and 64 (above) with one row less and one more, several tiles both ways on both sides of either tile-height switch (8 | 9, 16 | 17), and many
# ragged tiles in a batch
_SHAPES = [(1, 1, 1, "any"), (1, 1, 32, "C25"), (1, 5, 1, "any"), (1, 5, 2, "C25"), (5, 1, 1, "C25"), (5, 1, 2, "any"), (3, 200, 8, "any"),
           (9, 63, 1, "any"), (9, 64, 1, "C25"), (9, 65, 1, "any"), (9, 63, 3, "C25"), (9, 64, 3, "any"), (9, 65, 3, "C25"),
           (15, 70, 2, "C25"), (16, 70, 2, "any"), (17, 70, 2, "C25"), (31, 70, 9, "any"), (32, 70, 9, "C25"), (33, 70, 9, "any"),
           (63, 70, 17, "C25"), (64, 70, 17, "any"), (65, 70, 17, "C25")]
_SHAPES += [(67, 131, r, "any") for r in (1, 2, 3, 8, 9, 16, 17, 32)] + [(130, 200, r, "C25") for r in (1, 2, 3, 8, 9, 16, 17, 32)]
_SHAPES += [(67, 131, 1, "C25"), (67, 131, 17, "C25")]


def _big():
    return np.stack([patchy(600, 900, 5), noise(600, 900, 6)])


def _three():
    return np.stack([patchy(70, 90, 21), noise(70, 90, 22, 3), noise(70, 90, 23)])


CASES = [Case(f"stack {H}x{W} radius {r} {cfg}", functools.partial(stack, H, W, r), r, cfg) for H, W, r, cfg in _SHAPES]
CASES += [Case("two of 600x900 radius 2", _big, 2, "C25"), Case("three of 70x90 radius 3", _three, 3, "C25")]
CASE = {c.name: c for c in CASES}
assert len(CASE) == len(CASES)


def role_of(name):
    return roles(**CONFIGS[CASE[name].config])


@functools.lru_cache(maxsize=None)
def maps_of(name):
    """The case's maps, read-only, built once."""
    m = np.ascontiguousarray(CASE[name].build())
    m.setflags(write=False)
    return m


@functools.lru_cache(maxsize=None)
def votes_of(name):
    """The Votes of every image of the case, computed once."""
    return tuple(votes(one, role_of(name), CASE[name].radius) for one in maps_of(name))


@functools.lru_cache(maxsize=None)
def want_of(name, where="all", half=False):
    """The restated (out, support) of the case in one mode, read-only, computed once."""
    res = [apply(one, role_of(name), vt, where == "all", half) for one, vt in zip(maps_of(name), votes_of(name))]
    out, support = np.stack([a for a, _ in res]), np.stack([s for _, s in res])
    out.setflags(write=False)
    support.setflags(write=False)
    return out, support
