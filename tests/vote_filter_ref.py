"""numpy restatement of the guided vote filter (mmsa_vote_filter_u8, csrc/vote.hip), a brute-force version straight from the definition for
small maps, and the cases the CPU and the GPU tests share -- TEST INFRASTRUCTURE ONLY.  Maps, roles and modes are tests/majority_ref.py's.

  Window, roles, targets and the half rule: the majority filter's.  d(p, q) = sum_c |g_p[c] - g_q[c]| on the top-left H x W of the guide; lut: 255 G + 1 entries
  in 0 .. 4096 (1 without a guide); wq(q) = min(255, int(clamp(w) * 256)) in float32, NaN / negatives -> 0, above 1 -> 1 (1 without weights).
  S_v(p) = sum of lut[d(p, q)] wq(q) over the voters q of value v in the window, T = sum_v S_v, S_best = max_v S_v.  w(p) = the own value if p is a voter and
  S_own = S_best, else the smallest v with S_v = S_best.  out = w iff target and T > 0 and (not half or 2 S_best > T), else the input; support = S_best at a
  target, 0 elsewhere (uint32).

`sums` goes tap by tap: the weight plane lut[d] * wq[q] of one displacement (dy, dx) is added into hist[slot[q], p] by fancy indexing -- within one tap every
(slot, p) is unique, so a plain += is right -- and `majority_ref.apply` takes the decision on those sums.  `brute` loops over the pixels."""
import functools
from collections import namedtuple

import numpy as np

from tests import majority_ref as MR

MAX_RADIUS = 16
MAX_WEIGHT = 4096


def range_table(sigma, channels):
    """floor(256 exp(-d^2 / (2 sigma^2)) + 0.5) in float64, uint16 [255 channels + 1]: written out here a second time, on purpose."""
    d = np.arange(255 * channels + 1, dtype=np.float64)
    return np.floor(256.0 * np.exp(-d * d / (2.0 * sigma * sigma)) + 0.5).astype(np.uint16)


def cut_table(channels, first_zero=40):
    """A hand-made table: 37 at d = 0, falling by one per step down to 1, then 0 from `first_zero` on."""
    d = np.arange(255 * channels + 1)
    return np.where(d < first_zero, np.maximum(37 - d, 1), 0).astype(np.uint16)


def wq_of(weights):
    """float32 [..] -> int64 [..]: min(255, int(clamp(w) * 256.0f)); NaN and everything <= 0 give 0, everything >= 1 gives 255."""
    w = np.asarray(weights, dtype=np.float32)
    with np.errstate(invalid="ignore"):
        c = np.where(w > 0, np.where(w > 1, np.float32(1), w), np.float32(0)).astype(np.float32)
    return np.minimum(255, (c * np.float32(256)).astype(np.int64))


def _planes(m, role, guide, wq):
    m = np.asarray(m, dtype=np.uint8)
    H, W = m.shape
    voter = role[m] == MR.VOTER
    w0 = np.where(voter, 1 if wq is None else np.asarray(wq, dtype=np.int64), 0).astype(np.int64)
    g = None if guide is None else np.asarray(guide)[:H, :W].reshape(H, W, -1).astype(np.int64)
    return m, voter, w0, g


def _sums_block(m, role, r, guide, lut, wq):
    m, voter, w0, g = _planes(m, role, guide, wq)
    H, W = m.shape
    vals = np.unique(m[voter])
    ns = max(len(vals), 1)
    slot_of = np.zeros(256, dtype=np.int64)
    slot_of[vals] = np.arange(len(vals))
    slot = slot_of[m]
    hist = np.zeros((ns, H * W), dtype=np.int64)
    pix = np.arange(H * W).reshape(H, W)
    lut = None if lut is None else np.asarray(lut, dtype=np.int64)
    for dy in range(-min(r, H - 1), min(r, H - 1) + 1):
        py = slice(max(0, -dy), min(H, H - dy))
        qy = slice(py.start + dy, py.stop + dy)
        for dx in range(-min(r, W - 1), min(r, W - 1) + 1):
            px = slice(max(0, -dx), min(W, W - dx))
            qx = slice(px.start + dx, px.stop + dx)
            wt = w0[qy, qx]
            if g is not None:
                wt = wt * lut[np.abs(g[py, px] - g[qy, qx]).sum(axis=2)]
            hist[slot[qy, qx].ravel(), pix[py, px].ravel()] += wt.ravel()      # one tap: every (slot, p) once
    best = hist.max(axis=0)
    value = (vals[hist.argmax(axis=0)] if len(vals) else np.zeros(H * W)).astype(np.int64)      # argmax: the first, the smallest value
    own = np.where(voter.ravel(), hist[slot.ravel(), pix.ravel()], 0)
    total, tied = hist.sum(axis=0), ((hist == best) & (hist > 0)).sum(axis=0)
    return MR.Votes(*(a.reshape(H, W) for a in (best, value, own, total, tied)))


def sums(m, role, r, guide=None, lut=None, wq=None, cells=1 << 25):
    """One image uint8 [H, W] -> majority_ref.Votes of the weighted sums (int64 [H, W] each).  A large map goes in bands of rows, each with its halo, so that
    the histogram of a band stays below `cells` entries."""
    m = np.asarray(m, dtype=np.uint8)
    H, W = m.shape
    band = max(1, cells // (max(len(np.unique(m)), 1) * W) - 2 * r)
    if band >= H:
        return _sums_block(m, role, r, guide, lut, wq)
    parts = []
    for a in range(0, H, band):
        b, lo, hi = min(H, a + band), max(0, a - r), min(H, a + band + r)
        vt = _sums_block(m[lo:hi], role, r, None if guide is None else np.asarray(guide)[lo:hi], lut, None if wq is None else np.asarray(wq)[lo:hi])
        parts.append([x[a - lo:b - lo] for x in vt])
    return MR.Votes(*(np.concatenate(x) for x in zip(*parts)))


def apply(m, role, vt, all_=True, half=False):
    """(out uint8 [H, W], support uint32 [H, W]): majority_ref.apply's decision on the sums; the support is kept in 32 bits."""
    m = np.asarray(m, dtype=np.uint8)
    out, _ = MR.apply(m, role, vt, all_, half)
    ro = role[m]
    target = (ro == MR.HOLE) | ((ro == MR.VOTER) & bool(all_))
    assert int(vt.total.max(initial=0)) < 1 << 31
    return out, np.where(target, vt.best, 0).astype(np.uint32)


def vote(m, role, r, all_=True, half=False, guide=None, lut=None, wq=None):
    return apply(m, role, sums(m, role, r, guide, lut, wq), all_, half)


def vote_batch(maps, role, r, all_=True, half=False, guide=None, lut=None, wq=None):
    res = [vote(one, role, r, all_, half, None if guide is None else guide[b], lut, None if wq is None else wq[b]) for b, one in enumerate(maps)]
    return np.stack([a for a, _ in res]), np.stack([s for _, s in res])


def brute(m, role, r, all_=True, half=False, guide=None, lut=None, wq=None):
    """The same from the definition, pixel by pixel."""
    m, voter, w0, g = _planes(m, role, guide, wq)
    H, W = m.shape
    out, support = m.copy(), np.zeros((H, W), dtype=np.uint32)
    for py in range(H):
        for px in range(W):
            ro = role[m[py, px]]
            if not (ro == MR.HOLE or (ro == MR.VOTER and all_)):
                continue
            S = [0] * 256
            for qy in range(max(py - r, 0), min(py + r, H - 1) + 1):
                for qx in range(max(px - r, 0), min(px + r, W - 1) + 1):
                    if role[m[qy, qx]] != MR.VOTER:
                        continue
                    k = 1 if g is None else int(lut[sum(abs(int(a) - int(b)) for a, b in zip(g[py, px], g[qy, qx]))])
                    S[int(m[qy, qx])] += k * int(w0[qy, qx])
            T, nb = sum(S), max(S)
            support[py, px] = nb
            if T == 0 or (half and not 2 * nb > T):
                continue
            out[py, px] = m[py, px] if (ro == MR.VOTER and S[int(m[py, px])] == nb) else S.index(nb)      # index: the first, the smallest v
    return out, support


# ---- the guide and the weights of a case
def guide_of(maps, G, pad, seed):
    """uint8 [B, H + pad[0], W + pad[1], G] (G = 1: [B, Hg, Wg]): a colour per byte of the map plus noise of -6 .. 6 per channel, so that the guide has the
    map's edges; the padding holds other bytes, which a wrong row pitch would bring into the window."""
    rng = np.random.default_rng(seed)
    B, H, W = maps.shape
    palette = rng.integers(0, 256, size=(256, G))
    g = np.clip(palette[maps] + rng.integers(-6, 7, size=(B, H, W, G)), 0, 255)
    full = rng.integers(0, 256, size=(B, H + pad[0], W + pad[1], G))
    full[:, :H, :W] = g
    full = full.astype(np.uint8)
    return np.ascontiguousarray(full[..., 0] if G == 1 else full)


SPECIAL_WEIGHTS = np.array([np.nan, np.inf, -np.inf, -0.0, 0.0, 1.0, 1.5, -0.25, 1e-40, -1e-40, 1.0 / 256, np.nextafter(np.float32(1.0 / 256), np.float32(0)),
                            0.5, np.nextafter(np.float32(0.5), np.float32(0)), np.nextafter(np.float32(1), np.float32(0)), 255.0 / 256], dtype=np.float32)


def weights_of(shape, seed):
    """float32 `shape`: uniform in [0, 1) with one pixel in eight replaced by a special value."""
    rng = np.random.default_rng(seed)
    w = rng.random(shape, dtype=np.float32)
    pick = rng.random(shape) < 0.125
    w[pick] = SPECIAL_WEIGHTS[rng.integers(0, len(SPECIAL_WEIGHTS), size=shape)][pick]
    return w


# ---- the shared cases
Case = namedtuple("Case", "name build radius config G pad weights table")      # table: "sigma" (sigma = 8), "cut" (zeros from d = 40 on) or None (no guide)
TH, TH_SMALL = 16, 8                                                           # the tile heights csrc/vote.hip builds: 8 rows up to radius 2, 16 above

# (H, W, radius, config); the options rotate over them.  15 / 16 / 17 rows at radius 2 are two tiles of 8 rows and a ragged third; at radius 3 and above they
# are the rows around the 16-row tile, and 7 / 8 / 9 rows those around the 8-row tile
_SMALL = [(1, 1, 1, "any"), (1, 1, 16, "C25"), (1, 5, 1, "any"), (1, 5, 2, "C25"), (5, 1, 1, "C25"), (5, 1, 2, "any"), (3, 200, 8, "any"),
          (9, 63, 1, "any"), (9, 64, 1, "C25"), (9, 65, 1, "any"), (9, 63, 3, "C25"), (9, 64, 3, "any"), (9, 65, 3, "C25"),
          (TH - 1, 70, 2, "C25"), (TH, 70, 2, "any"), (TH + 1, 70, 2, "C25"), (TH - 1, 70, 16, "any"), (TH + 1, 70, 8, "C25"),
          (TH_SMALL - 1, 70, 2, "any"), (TH_SMALL, 70, 1, "C25"), (TH_SMALL + 1, 70, 2, "any"), (TH - 1, 70, 3, "C25"), (TH, 70, 4, "any"), (TH + 1, 70, 3, "any")]
_OPTIONS = [(3, (0, 0), True, "sigma"), (1, (5, 3), False, "cut"), (3, (5, 3), False, "sigma"), (1, (0, 0), True, "cut"),
            (1, (5, 3), True, "sigma"), (3, (0, 0), False, "cut"), (3, (5, 3), True, "cut"), (1, (0, 0), False, "sigma")]


def _stack(H, W, r):
    return MR.stack(H, W, r)


def _three():
    return np.stack([MR.patchy(70, 90, 21), MR.noise(70, 90, 22, 3), MR.noise(70, 90, 23)])


CASES = []
for _i, (_H, _W, _r, _cfg) in enumerate(_SMALL):
    _G, _pad, _wt, _tab = _OPTIONS[_i % len(_OPTIONS)]
    CASES.append(Case(f"stack {_H}x{_W} radius {_r} {_cfg} G{_G} pad{_pad[0]} {'w' if _wt else 'u'} {_tab}", functools.partial(_stack, _H, _W, _r), _r, _cfg,
                      _G, _pad, _wt, _tab))
# the two larger shapes at every radius class: between them the two cases of a radius hold every option both ways
for _j, _r in enumerate((1, 2, 4, 8, 16)):
    _a, _b = _OPTIONS[2 * (_j % 4)], _OPTIONS[2 * (_j % 4) + 1]      # each the other's opposite in every option
    if _j % 2:
        _a, _b = _b, _a
    for (_H, _W, _cfg), (_G, _pad, _wt, _tab) in (((67, 131, "any"), _a), ((130, 200, "C25"), _b)):
        CASES.append(Case(f"stack {_H}x{_W} radius {_r} {_cfg} G{_G} pad{_pad[0]} {'w' if _wt else 'u'} {_tab}", functools.partial(_stack, _H, _W, _r), _r,
                          _cfg, _G, _pad, _wt, _tab))
CASES += [Case("three of 70x90 radius 3", _three, 3, "C25", 3, (5, 3), True, "sigma"),
          Case("weights alone 67x131 radius 2", functools.partial(_stack, 67, 131, 2), 2, "C25", 0, (0, 0), True, None),
          Case("weights alone 16x70 radius 16", functools.partial(_stack, 16, 70, 16), 16, "any", 0, (0, 0), True, None)]
CASE = {c.name: c for c in CASES}
assert len(CASE) == len(CASES)
for _o in (0, 1, 2, 3):      # (G, pad, weights, table): every value of every option meets every radius class of the larger shapes
    for _r in (1, 2, 4, 8, 16):
        assert len({(c.G, c.pad, c.weights, c.table)[_o] for c in CASES if c.radius == _r and c.table and c.name.startswith(("stack 67x131", "stack 130x200"))}) == 2


def role_of(name):
    return MR.roles(**MR.CONFIGS[CASE[name].config])


def table_of(name):
    c = CASE[name]
    return None if c.table is None else range_table(8.0, c.G) if c.table == "sigma" else cut_table(c.G)


@functools.lru_cache(maxsize=None)
def inputs_of(name):
    """(maps uint8 [B, H, W], guide or None, weights float32 [B, H, W] or None) of the case, read-only, built once."""
    c = CASE[name]
    maps = np.ascontiguousarray(c.build())
    seed = 7 * maps.shape[1] + 13 * maps.shape[2] + c.radius
    guide = guide_of(maps, c.G, c.pad, seed) if c.table else None
    weights = weights_of(maps.shape, seed + 1) if c.weights else None
    for a in (maps, guide, weights):
        if a is not None:
            a.setflags(write=False)
    return maps, guide, weights


@functools.lru_cache(maxsize=None)
def sums_of(name):
    """The sums of every image of the case, computed once."""
    maps, guide, weights = inputs_of(name)
    wq = None if weights is None else wq_of(weights)
    return tuple(sums(one, role_of(name), CASE[name].radius, None if guide is None else guide[b], table_of(name), None if wq is None else wq[b])
                 for b, one in enumerate(maps))


@functools.lru_cache(maxsize=None)
def want_of(name, where="all", half=False):
    """The restated (out, support) of the case in one mode, read-only, computed once."""
    res = [apply(one, role_of(name), vt, where == "all", half) for one, vt in zip(inputs_of(name)[0], sums_of(name))]
    out, support = np.stack([a for a, _ in res]), np.stack([s for _, s in res])
    out.setflags(write=False)
    support.setflags(write=False)
    return out, support
