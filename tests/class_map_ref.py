"""Float64 restatement of the class-map family (csrc/segment.hip, csrc/slide_pixel.h, csrc/slide_taps.h, csrc/augment.hip), the per-element bound the
geometry tests hold the device to (tests/test_class_map_geometry_gpu.py), the case table, and a float32 emulation of the kernels' formula with switchable
mutations (tests/test_class_map_geometry_cpu.py keeps reference, bound and table honest) -- TEST INFRASTRUCTURE ONLY.

Reference.  A window's logits [C, hs, ws] become [C, hc, wc] by PyTorch's upsample_bilinear2d with align_corners=False, written as a plain gather: per
axis s = (i + 0.5) hs / hc - 0.5 clamped at 0, first tap floor(s), second tap first + 1 clamped to the last row / column, weight l = s - floor(s).  The
coordinate is formed in INTEGERS, s = ((2 i + 1) hs - hc) / (2 hc), so that floor(s) and l are those of the exact rational: a double evaluation of
(i + 0.5) * (hs / hc) - 0.5 can land 2^-52 below an integer and name the tap on its other side (ratio 1/3, i = 4).  A frame is the sum of its covering
windows in window order divided by their number; an optional second resize H x W -> Hd x Wd follows the same rule, then the cut [:Ho, :Wo]; the class map
is the first argmax, the confidence the maximum of the float64 softmax; an augmented frame is the mean over the views of the float64 softmax, each flipped
back, then argmax and maximum.

Bound, per element, u = 2^-24, g(n) = n u / (1 - n u).  Counted from the kernels' text, nothing measured:
  coordinate   r = fl(hs / hc) is off by at most u r; the product (i + 0.5) r and the subtraction of 0.5 round once each, (i + 0.5) itself is exact:
               |s_dev - s| <= delta_s = g(3) (s + 0.5), with s the unclamped coordinate's magnitude; the clamp at 0 does not enlarge it and
               lh = sh - h0 is exact (sh and h0 share their integer part).  The interpolant is continuous and piecewise bilinear in (sh, sw), so the value
               moves by at most (delta_s_h + delta_s_w) R, R = max - min of the float64 source values over the clamped 3 x 3 neighbourhood of the
               reference's top-left tap.  The neighbourhood, not the 2 x 2 cell, because continuity is what the term rests on: it also covers a device
               floor that lands on the other side of an integer.  That can only happen where the exact s IS an integer h0 (any other s is at least
               1 / (2 hc) from one, far more than delta_s), and then the device's cell is rows h0 - 1, h0 or h0, h0 + 1: inside the neighbourhood.
  arithmetic   (1 - lh) ((1 - lw) a + lw b) + lh ((1 - lw) c + lw d): on every path from a source value to the result lie `1 - lw`, its product with the
               value, the inner sum, `1 - lh` (or nothing: at most as many), the outer product and the outer sum -- six roundings:
               g(6) sum_k c_k |v_k|, c_k the float64 weights.
  overlap      nk - 1 additions in window order and the division: g(nk) sum_k |t_k| / nk on top of the mean of the windows' own bounds.
  second stage the same two terms on the float64 canvas values, plus the convex combination (the float64 weights) of the four taps' first-stage bounds.
  confidence   relative: (2 D + C + 4) 2^-23 of tests/confidence_ref.py::float64_check (D = max_c |x_c - m|) for the softmax of the logits as given, plus
               2 max_c bnd_c: a logit error d moves every exponent x_c - m by at most 2 d, hence a probability by at most 2 d relatively.
  aug          per view and class the same relative bound times the probability; the mean adds A - 1 additions and the division: g(A) times the mean.
               The confidence (max over the classes, which is 1-Lipschitz) gets the largest of the classes' bounds.

Class maps cannot be bounded by value.  A pixel passes when it equals the float64 argmax, or when the float64 margin between the top class and the class
the device chose is at most the sum of those two classes' bounds at that pixel; pixels excused the second way are counted, and at most EXCUSED_CAP of a
case's pixels may be.  A 255 pixel never passes."""
import numpy as np
import torch

from tests import confidence_ref as CR
from tests.variant_ref import gen_for

U = 2.0 ** -24
EXCUSED_CAP = 1e-3
F32 = np.float32
MUTATIONS = ("swap_l", "rh_from_w", "no_clamp0", "row_step_hs", "h0_clamp_ws", "first_adds", "wrong_count", "hflip_Ho")


def g(n):
    return n * U / (1.0 - n * U)


# ------------------------------------------------------------------------------------------------ case table
def _geo(hs, ws, hc, wc, H, W, B, wins, stride, targets):
    """targets: (Hd, Wd, Ho, Wo) of the second stage; None = the frame's own size (mmsa_slide_argmax)."""
    return dict(hs=hs, ws=ws, hc=hc, wc=wc, H=H, W=W, B=B, wins=tuple(wins), stride=stride, targets=(None,) + tuple(targets))


GEOS = {
    # ratios 5/12 and 7/20, overlap 1 / 2 / 4, every h/w swap
    "nonsq-5x7-12x20-20x33-b2": _geo(5, 7, 12, 20, 20, 33, 2, [(0, 0), (0, 13), (8, 0), (8, 13)], (8, 13),
                                     [(29, 47, 29, 47), (13, 21, 13, 21), (26, 24, 20, 17)]),
    # overlap up to 8: all eight slots of slide_pixel.h, the scanning form of the resized kernels
    "ov8-5x7-12x20-18x35-b1": _geo(5, 7, 12, 20, 18, 35, 1, [(y, x) for y in (0, 6) for x in (0, 5, 10, 15)], (6, 5),
                                   [(25, 51, 25, 51), (11, 23, 11, 23), (27, 22, 21, 16)]),
    # W > 256: the second workgroup in x; ratios 1/3 and 7/27 (no map may exceed 300 a side, so no target is wider than the frame)
    "wide-3x70-9x270-9x300-b1": _geo(3, 70, 9, 270, 9, 300, 1, [(0, 0), (0, 30)], (9, 30),
                                     [(13, 299, 13, 299), (5, 131, 5, 131), (7, 290, 6, 270)]),
    # logits larger than the window: taps skip source pixels
    "down-13x11-6x5-6x8-b2": _geo(13, 11, 6, 5, 6, 8, 2, [(0, 0), (0, 3)], (6, 3), [(11, 13, 11, 13), (4, 5, 4, 5), (9, 6, 7, 5)]),
    # no row below / no column to the right anywhere
    "thin-h-1x4-7x10-7x10-b2": _geo(1, 4, 7, 10, 7, 10, 2, [(0, 0)], (7, 10), [(10, 17, 10, 17), (5, 7, 5, 7), (9, 7, 8, 6)]),
    "thin-w-4x1-10x7-10x7-b2": _geo(4, 1, 10, 7, 10, 7, 2, [(0, 0)], (10, 7), [(17, 10, 17, 10), (7, 5, 7, 5), (7, 9, 6, 8)]),
    # integer ratio 3: coordinates inexact in fp32, source coordinates that ARE integers
    "third-4x5-12x15-12x15-b1": _geo(4, 5, 12, 15, 12, 15, 1, [(0, 0)], (12, 15), [(17, 22, 17, 22), (7, 11, 7, 11), (19, 11, 13, 9)]),
    # ratio 1: all weights 0, the canvas equals the logits bit for bit
    "ident-6x9-6x9-6x9-b1": _geo(6, 9, 6, 9, 6, 9, 1, [(0, 0)], (6, 9), [(10, 14, 10, 14), (4, 7, 4, 7), (8, 7, 7, 5)]),
}
NONSQ, OV8, WIDE, DOWN, THIN_H, THIN_W, THIRD, IDENT = GEOS
# (geometry, C): C = 33 -> 128 lanes of aug_argmax; C = 70 -> the second-pass form of slide_argmax_conf and the 64 lanes of aug_argmax
CASES = [(k, 5) for k in GEOS] + [(NONSQ, 33), (NONSQ, 70)]
CASE_IDS = [f"{k}-c{C}" for k, C in CASES]

# Augmented frames: views (geometry, flip code 0 none / 1 horizontal / 2 vertical), every view resized to the shared (Hd, Wd) and cut to (Ho, Wo) -- Ho != Wo
# != Hd != Wd, so no two of the row's columns can stand in for each other; all views of a case share B.
AUGS = {
    "aug3-26x37-cut23x31-b2": dict(views=((NONSQ, 0), (DOWN, 1), ("third-4x5-12x15-12x15-b2", 2)), target=(26, 37, 23, 31)),
    "aug-ov8-25x41-b1": dict(views=((OV8, 1), (THIRD, 0)), target=(25, 41, 25, 41)),
}
GEOS_AUG = dict(GEOS)
GEOS_AUG["third-4x5-12x15-12x15-b2"] = _geo(4, 5, 12, 15, 12, 15, 2, [(0, 0)], (12, 15), [])
AUG_CASES = [("aug3-26x37-cut23x31-b2", 5), ("aug3-26x37-cut23x31-b2", 33), ("aug3-26x37-cut23x31-b2", 70), ("aug-ov8-25x41-b1", 5)]
AUG_IDS = [f"{k}-c{C}" for k, C in AUG_CASES]


def jobs_of(geo):
    """The windows (image, y0, x0) in MapPlan.slide order: every window once per image."""
    return [(b, y0, x0) for y0, x0 in geo["wins"] for b in range(geo["B"])]


def logits_of(case_id, geo, C, ties=False):
    """Seeded head-resolution logits float32 [n, C, hs, ws]; `ties`: class 3 is a copy of class 1 and both are the maximum everywhere."""
    x = torch.randn(len(jobs_of(geo)), C, geo["hs"], geo["ws"], generator=gen_for(case_id))
    if ties:
        x[:, 1] += 8.0
        x[:, 3] = x[:, 1]
    return x


# ------------------------------------------------------------------------------------------------ float64 reference and bound
def axis(n_src, n_dst):
    """One axis of the reference resize, from integers -> (first tap, second tap, weight of the second, |unclamped coordinate|)."""
    num = (2 * np.arange(n_dst, dtype=np.int64) + 1) * n_src - n_dst       # s = num / (2 n_dst)
    mag = np.abs(num) / (2.0 * n_dst)
    num = np.maximum(num, 0)
    i0 = np.minimum(num // (2 * n_dst), n_src - 1)
    lam = (num - i0 * 2 * n_dst) / (2.0 * n_dst)
    i1 = np.minimum(i0 + 1, n_src - 1)
    return i0, i1, np.where(i1 > i0, lam, 0.0), mag


def _range3(v, i0, j0):
    """max - min of v [..., hs, ws] over the clamped 3 x 3 neighbourhood of (i0[a], j0[b]) -> [..., len(i0), len(j0)]."""
    hs, ws = v.shape[-2:]
    hi = lo = None
    for di in (-1, 0, 1):
        for dj in (-1, 0, 1):
            t = v[..., np.clip(i0 + di, 0, hs - 1)[:, None], np.clip(j0 + dj, 0, ws - 1)[None, :]]
            hi = t if hi is None else np.maximum(hi, t)
            lo = t if lo is None else np.minimum(lo, t)
    return hi - lo


def resize(v, hd, wd, bnd=None):
    """v float64 [..., hs, ws] -> (resized [..., hd, wd], its bound): the coordinate and arithmetic terms, plus the convex combination of `bnd` (the
    bounds of v's own elements) where given."""
    hs, ws = v.shape[-2:]
    i0, i1, lh, mh = axis(hs, hd)
    j0, j1, lw, mw = axis(ws, wd)
    I0, I1, J0, J1 = i0[:, None], i1[:, None], j0[None, :], j1[None, :]
    LH, LW = lh[:, None], lw[None, :]
    w = ((1 - LH) * (1 - LW), (1 - LH) * LW, LH * (1 - LW), LH * LW)
    at = ((I0, J0), (I0, J1), (I1, J0), (I1, J1))
    out = sum(c * v[..., a, b] for c, (a, b) in zip(w, at))
    mag = sum(c * np.abs(v[..., a, b]) for c, (a, b) in zip(w, at))
    delta = g(3) * ((mh + 0.5)[:, None] + (mw + 0.5)[None, :])
    b = g(6) * mag + delta * _range3(v, i0, j0)
    if bnd is not None:
        b = b + sum(c * bnd[..., a, b_] for c, (a, b_) in zip(w, at))
    return out, b


def canvas(lg, geo):
    """lg float64 numpy [n, C, hs, ws] -> (averaged canvas [B, C, H, W], its bound, count int [B, H, W])."""
    B, H, W, hc, wc = geo["B"], geo["H"], geo["W"], geo["hc"], geo["wc"]
    C = lg.shape[1]
    acc, mag, bsum = (np.zeros((B, C, H, W)) for _ in range(3))
    cnt = np.zeros((B, H, W), dtype=np.int64)
    for k, (b, y0, x0) in enumerate(jobs_of(geo)):
        t, tb = resize(lg[k], hc, wc)
        sl = (b, slice(None), slice(y0, y0 + hc), slice(x0, x0 + wc))
        acc[sl] += t
        mag[sl] += np.abs(t)
        bsum[sl] += tb
        cnt[b, y0:y0 + hc, x0:x0 + wc] += 1
    assert cnt.min() >= 1, "the case's windows must cover its frame"
    n = cnt[:, None].astype(np.float64)
    return acc / n, bsum / n + g(n) * mag / n, cnt


def frame(lg, geo, target=None):
    """The logits the class map is the argmax of -> (float64 [B, C, Ho, Wo], bound): the canvas, or its second resize to (Hd, Wd) cut to (Ho, Wo)."""
    v, b, _ = canvas(lg, geo)
    if target is None:
        return v, b
    Hd, Wd, Ho, Wo = target
    v2, b2 = resize(v, Hd, Wd, b)
    return v2[..., :Ho, :Wo], b2[..., :Ho, :Wo]


def softmax(v):
    e = np.exp(v - v.max(1, keepdims=True))
    return e / e.sum(1, keepdims=True)


def softmax_rel(v, b):
    """The relative bound of every softmax element of a pixel -> [B, 1, h, w]."""
    D = np.abs(v - v.max(1, keepdims=True)).max(1, keepdims=True)
    return (2 * D + v.shape[1] + 4) * 2.0 ** -23 + 2 * b.max(1, keepdims=True)


def confidence(v, b):
    """-> (max of the float64 softmax [B, h, w], its ABSOLUTE bound)."""
    want = softmax(v).max(1)
    return want, softmax_rel(v, b)[:, 0] * want


def flip_back(p, code):
    return p[..., ::-1] if code == 1 else p[..., ::-1, :] if code == 2 else p


def aug(lgs, aug_case):
    """lgs: one float64 [n_a, C, hs_a, ws_a] per view -> (mean probabilities [B, C, Ho, Wo], their absolute bound)."""
    A = len(lgs)
    P = Pb = None
    for lg, (gk, code) in zip(lgs, aug_case["views"]):
        v, b = frame(lg, GEOS_AUG[gk], aug_case["target"])
        p = softmax(v)
        p, pb = flip_back(p, code), flip_back(softmax_rel(v, b) * p, code)
        P, Pb = (p, pb) if P is None else (P + p, Pb + pb)
    return P / A, Pb / A + g(A) * P / A


def check_values(y, r, bnd, what):
    """Element by element |y - r| <= bnd (NaN fails) -> the worst |err| / bound."""
    y = np.asarray(y, dtype=np.float64)
    assert y.shape == r.shape, f"{what}: shape {y.shape} vs {r.shape}"
    err = np.abs(y - r)
    ratio = err / np.maximum(bnd, 1e-300)
    bad = ~(err <= bnd)
    if bad.any():
        k = tuple(int(i) for i in np.unravel_index(np.argmax(np.nan_to_num(ratio, nan=np.inf)), y.shape))
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.size} elements outside the bound; worst at {k}: got {float(y[k])!r}, "
                             f"reference {float(r[k])!r}, bound {float(bnd[k]):.3e}")
    return float(ratio.max()) if ratio.size else 0.0


def map_faults(m, r, bnd):
    """Class map m uint8 [B, h, w] against the float64 values r [B, C, h, w] and their bounds -> (pixels that do not pass, pixels excused)."""
    m = np.asarray(m).astype(np.int64)
    top = r.argmax(1)
    legal = m < r.shape[1]
    mc = np.where(legal, m, 0)[:, None]
    pick = lambda a, i: np.take_along_axis(a, i, 1)[:, 0]
    margin = pick(r, top[:, None]) - pick(r, mc)
    allow = pick(bnd, top[:, None]) + pick(bnd, mc)
    same = legal & (m == top)
    excused = legal & ~same & (margin <= allow)
    return int((~same & ~excused).sum()), int(excused.sum())


def check_map(m, r, bnd, what):
    """The excused-pixel rule -> number of excused pixels (at most EXCUSED_CAP of the map)."""
    wrong, excused = map_faults(m, r, bnd)
    assert wrong == 0, f"{what}: {wrong} of {np.asarray(m).size} pixels name a class whose float64 margin to the top class exceeds the two bounds"
    assert excused <= EXCUSED_CAP * np.asarray(m).size, f"{what}: {excused} of {np.asarray(m).size} pixels excused, more than {EXCUSED_CAP:.1%}"
    return excused


# ------------------------------------------------------------------------------------------------ float32 emulation, with mutations
def emu_axis(n_src, n_dst, mut=(), h_axis=False, other=None):
    """One axis as tap_coords computes it in float32 -> (first tap, has-a-second-tap flag, weight).  `other` = (n_src, n_dst) of the other axis, for the
    mutations that take a height for a width."""
    r = F32(n_src) / F32(n_dst)
    last = n_src - 1
    if h_axis and "rh_from_w" in mut:
        r = F32(other[0]) / F32(other[1])
    if h_axis and "h0_clamp_ws" in mut:
        last = other[0] - 1
    s = (np.arange(n_dst).astype(F32) + F32(0.5)) * r - F32(0.5)
    if "no_clamp0" not in mut:
        s = np.maximum(s, F32(0))
    i0 = np.minimum(s.astype(np.int64), last)      # (int): truncation
    lam = s - i0.astype(F32)
    assert s.dtype == F32 and lam.dtype == F32
    return i0, i0 < last, lam


def emu_resize(v, hd, wd, mut=()):
    """v float32 [C, hs, ws] -> [C, hd, wd]: tap_coords + tap_term, operation by operation (numpy float32 arrays round every operation, no contraction)."""
    C, hs, ws = v.shape
    h0, fh, lh = emu_axis(hs, hd, mut, True, (ws, wd))
    w0, fw, lw = emu_axis(ws, wd, mut, False, (hs, hd))
    o = h0[:, None] * ws + w0[None, :]
    dh = np.where(fh, hs if "row_step_hs" in mut else ws, 0)[:, None]
    dw = fw.astype(np.int64)[None, :]
    sp = v.reshape(C, hs * ws)
    at = lambda i: sp[:, np.clip(i, 0, hs * ws - 1)]       # the clip only ever acts under an index mutation
    LH, LW = lh[:, None], lw[None, :]
    if "swap_l" in mut:
        LH, LW = np.broadcast_to(lw[None, :], o.shape), np.broadcast_to(lh[:, None], o.shape)
    one = F32(1)
    out = (one - LH) * ((one - LW) * at(o) + LW * at(o + dw)) + LH * ((one - LW) * at(o + dh) + LW * at(o + dh + dw))
    assert out.dtype == F32
    return out


def emu_sums(lg, geo, mut=()):
    """lg float32 [n, C, hs, ws] -> (window sums in window order float32 [B, C, H, W], count float32 [B, H, W]); the first window WRITES."""
    B, H, W, hc, wc = geo["B"], geo["H"], geo["W"], geo["hc"], geo["wc"]
    acc = np.zeros((B, lg.shape[1], H, W), dtype=F32)
    cnt = np.zeros((B, H, W), dtype=F32)
    if "first_adds" in mut:
        acc += F32(2.0 ** -10)
    for k, (b, y0, x0) in enumerate(jobs_of(geo)):
        acc[b, :, y0:y0 + hc, x0:x0 + wc] += emu_resize(lg[k], hc, wc, mut)      # 0 + v == v
        cnt[b, y0:y0 + hc, x0:x0 + wc] += F32(1)
    return acc, cnt


def emu_frame(lg, geo, target=None, mut=()):
    """The emulated logits at the map's size, float32 [B, C, Ho, Wo]: tap_value / slide_pixel.h, then two_stage_value."""
    acc, cnt = emu_sums(lg, geo, mut)
    if target is None:
        return acc / cnt[:, None]
    Hd, Wd, Ho, Wo = target
    B, C, H, W = acc.shape
    y0, fy, lh = emu_axis(H, Hd)
    x0, fx, lw = emu_axis(W, Wd)
    y1, x1 = y0 + fy, x0 + fx
    Y0, Y1, X0, X1 = y0[:, None], y1[:, None], x0[None, :], x1[None, :]
    tap = lambda Y, X, Xc: acc[:, :, Y, X] / cnt[:, None, Y, Xc]
    wc_ = "wrong_count" in mut                                                  # a tap divided by its horizontal neighbour's count
    p00, p01 = tap(Y0, X0, X1 if wc_ else X0), tap(Y0, X1, X0 if wc_ else X1)
    p10, p11 = tap(Y1, X0, X1 if wc_ else X0), tap(Y1, X1, X0 if wc_ else X1)
    LH, LW, one = lh[:, None], lw[None, :], F32(1)
    out = (one - LH) * ((one - LW) * p00 + LW * p01) + LH * ((one - LW) * p10 + LW * p11)
    assert out.dtype == F32
    return np.ascontiguousarray(out[..., :Ho, :Wo])


def emu_confidence(x):
    return CR.confidence(torch.from_numpy(np.ascontiguousarray(x))).numpy()


def emu_softmax(x):
    """csrc/softmax_px.h on float32 [B, C, h, w]: m in class order, e = exp(x - m), s in class order, e / s."""
    m = x[:, 0]
    for c in range(1, x.shape[1]):
        m = np.where(x[:, c] > m, x[:, c], m)
    e = np.exp(x - m[:, None])
    s = e[:, 0]
    for c in range(1, x.shape[1]):
        s = s + e[:, c]
    assert e.dtype == F32 and s.dtype == F32
    return e / s[:, None]


def emu_aug(lgs, aug_case, mut=()):
    """-> mean probabilities float32 [B, C, Ho, Wo]: the views' softmax, flipped back, added in view order, divided by A."""
    Ho, Wo = aug_case["target"][2:]
    acc = None
    for lg, (gk, code) in zip(lgs, aug_case["views"]):
        p = emu_softmax(emu_frame(lg, GEOS_AUG[gk], aug_case["target"], mut))
        if code == 1:
            p = p[..., np.clip((Ho if "hflip_Ho" in mut else Wo) - 1 - np.arange(Wo), 0, Wo - 1)]
        elif code == 2:
            p = p[..., ::-1, :]
        acc = p if acc is None else acc + p
    out = acc / F32(len(lgs))
    assert out.dtype == F32
    return out


def first_argmax(x):
    return np.argmax(x, axis=1).astype(np.uint8)      # numpy's argmax names the first maximum


def aug_logits(aug_id, C):
    ac = AUGS[aug_id]
    return [logits_of(f"{aug_id}-c{C}-view{a}", GEOS_AUG[gk], C) for a, (gk, _) in enumerate(ac["views"])]
