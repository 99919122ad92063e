"""numpy restatement of the panoptic passes (mmsa_segment_pairs, mmsa_eval_panoptic), written from the definitions -- no waves, no
atomics, no schedule -- TEST INFRASTRUCTURE ONLY.

  a pixel takes part iff its label code L is not 255; area_g / area_p = the participating pixels of a label / prediction segment
  a HIT pixel has L < C and P == L (P = min(pred, C)); inter(p, g) = the hit pixels with root_pred == p and root_label == g
  p and g MATCH iff 3 * inter > area_p + area_g; over the segments of class c < C with area > 0: a matched pair is a TP of c and adds
  floor(inter * 2^24 / (area_p + area_g - inter)) to the IoU sum, an unmatched label segment an FN, an unmatched prediction segment an FP, at the size
  bucket min(23, floor(log2 area)) of area_g (TP, FN) / area_p (FP)

The table: key = ((b * H * W + root_label) << 31) | root_pred, slot = (key * 0x9e3779b97f4a7c15 mod 2^64) >> (64 - log2 capacity), linear probing over at
most min(128, capacity) slots.  `table_prediction` inserts the distinct keys one after the other WITHOUT the bound: the set of occupied slots of a
linear-probing table does not depend on the order, so it is the device's set whenever the device dropped nothing -- and the device drops nothing, in any
order, when every key's walk from its home slot to the end of its run of occupied slots stays inside the bound (`longest_walk`)."""
from fractions import Fraction

import numpy as np

from tests import boundary_ref as BR
from tests import components_ref as CR

SIZE_BUCKETS = 24
IOU_ONE = 1 << 24
HASH_MUL = 0x9E3779B97F4A7C15
MAX_PROBES = 128
EMPTY = -1


def bucket(area):
    return min(SIZE_BUCKETS - 1, int(area).bit_length() - 1)


def pairs_of(L, P, C, root_label, root_pred, b=0):
    """One image -> (keys int64 sorted, counts int64): the distinct pairs of its hit pixels."""
    HW = L.size
    hit = ((L < C) & (P == L)).ravel()
    key = ((b * HW + root_label.ravel()[hit].astype(np.int64)) << 31) | root_pred.ravel()[hit].astype(np.int64)
    return np.unique(key, return_counts=True)


def slot_of(key, capacity):
    log2 = capacity.bit_length() - 1
    assert capacity == 1 << log2 and log2 >= 1
    return ((int(key) * HASH_MUL) & ((1 << 64) - 1)) >> (64 - log2)


def table_prediction(keys, capacity):
    """The distinct `keys` into an unbounded linear-probing table of `capacity` slots -> dict(occupied = the sorted occupied slots, longest_walk = the most
    slots a key can look at in ANY insertion order (the distance from its home slot to the first free slot of the full table, inclusive),
    overflow_impossible: every key finds a slot within the device's bound whatever the order, overflow_certain: more keys than slots, load)."""
    keys = [int(k) for k in keys]
    if len(keys) > capacity:
        return dict(occupied=np.arange(capacity), longest_walk=capacity, overflow_impossible=False, overflow_certain=True, load=len(keys) / capacity)
    used = np.zeros(capacity, dtype=bool)
    homes = []
    for k in keys:
        at = slot_of(k, capacity)
        homes.append(at)
        while used[at]:
            at = (at + 1) & (capacity - 1)
        used[at] = True
    longest = 0
    if keys and used.all():
        longest = capacity
    elif keys:
        free = np.nonzero(~used)[0]
        nxt = free[np.searchsorted(free, homes) % len(free)]                 # the first free slot at or behind the home, around the end
        longest = int(((nxt - np.asarray(homes)) % capacity).max())           # occupied slots a key may have to pass: it takes a slot at or before `nxt`
    bound = min(MAX_PROBES, capacity)
    return dict(occupied=np.nonzero(used)[0], longest_walk=longest, overflow_impossible=longest <= bound, overflow_certain=False, load=len(keys) / capacity)


def panoptic(pred, labels, lut, C, connectivity=8, ymap=None, xmap=None, slots=None, n_slots=None):
    """pred uint8 [B, H, W], labels uint8 [B, Hl, Wl] -> dict(counts int64 [n_slots, C, 24, 4], match int32 [2, B, H, W], keys, inter (the sorted pair list
    over the batch), planes int64 [4, B, H, W], root_pred, root_label, ious = [(class, Fraction)] of the TPs): everything a PanopticEvaluator.add() leaves."""
    B, H, W = pred.shape
    HW = H * W
    slots = list(range(B)) if slots is None else list(slots)
    counts = np.zeros((n_slots or max(slots) + 1, C, SIZE_BUCKETS, 4), dtype=np.int64)
    match = np.full((2, B, HW), -1, dtype=np.int32)
    all_keys, all_inter, planes, rps, rls, ious = [], [], [], [], [], []
    for b in range(B):
        L, P = BR.codes(pred[b], labels[b], lut, C, ymap, xmap)
        rl, rp = CR.roots(L, connectivity), CR.roots(P, connectivity)
        pl = CR.segment_planes(L, P, C, rl, rp).reshape(4, HW)
        keys, inter = pairs_of(L, P, C, rl, rp, b)
        Lf, Pf = L.ravel(), P.ravel()
        for k, n in zip(keys.tolist(), inter.tolist()):
            g, p = (k >> 31) - b * HW, k & ((1 << 31) - 1)
            ag, ap = int(pl[0, g]), int(pl[2, p])
            if 3 * n > ap + ag:
                assert match[0, b, g] < 0 and match[1, b, p] < 0             # uniqueness
                match[0, b, g], match[1, b, p] = p, g
                c = int(Lf[g])
                assert c < C and int(Pf[p]) == c
                counts[slots[b], c, bucket(ag), 0] += 1
                counts[slots[b], c, bucket(ag), 3] += (n << 24) // (ap + ag - n)
                ious.append((c, Fraction(n, ap + ag - n)))
        for g in np.nonzero((rl.ravel() == np.arange(HW)) & (pl[0] > 0) & (Lf < C) & (match[0, b] < 0))[0]:
            counts[slots[b], int(Lf[g]), bucket(pl[0, g]), 2] += 1
        for p in np.nonzero((rp.ravel() == np.arange(HW)) & (pl[2] > 0) & (Pf < C) & (match[1, b] < 0))[0]:
            counts[slots[b], int(Pf[p]), bucket(pl[2, p]), 1] += 1
        all_keys.append(keys), all_inter.append(inter), planes.append(pl.reshape(4, H, W)), rps.append(rp), rls.append(rl)
    return dict(counts=counts, match=match.reshape(2, B, H, W), keys=np.concatenate(all_keys), inter=np.concatenate(all_inter), planes=np.stack(planes, 1),
                root_pred=np.stack(rps), root_label=np.stack(rls), ious=ious)


def brute_force(L, P, C, connectivity=8):
    """One image, from sets of pixels: -> (tp, fp, fn as lists of (class, area), matches as a list of (label root, prediction root, Fraction IoU)).  A
    segment is the set of its participating pixels; IoU = |p & g| / |p | g| as a Fraction, over pairs of ONE class; match iff IoU > 1/2."""
    rl, rp = CR.roots(L, connectivity).ravel(), CR.roots(P, connectivity).ravel()
    Lf, Pf = L.ravel(), P.ravel()
    part = Lf != BR.IGNORE

    def segs(root, code):
        out = {}
        for r in np.unique(root):
            px = frozenset(np.nonzero((root == r) & part)[0].tolist())
            if px and code[r] < C:
                out[int(r)] = (int(code[r]), px)
        return out

    G, Pd = segs(rl, Lf), segs(rp, Pf)
    matches, got_g, got_p = [], set(), set()
    for g, (cg, sg) in G.items():
        for p, (cp, sp) in Pd.items():
            if cg == cp and sg & sp:
                iou = Fraction(len(sg & sp), len(sg | sp))
                if iou > Fraction(1, 2):
                    assert g not in got_g and p not in got_p
                    matches.append((g, p, iou))
                    got_g.add(g), got_p.add(p)
    tp = [(G[g][0], len(G[g][1])) for g, _, _ in matches]
    fn = [(c, len(s)) for g, (c, s) in G.items() if g not in got_g]
    fp = [(c, len(s)) for p, (c, s) in Pd.items() if p not in got_p]
    return tp, fp, fn, matches


def counts_of_brute_force(tp, fp, fn, matches, C):
    out = np.zeros((C, SIZE_BUCKETS, 4), dtype=np.int64)
    for (c, a), (_, _, iou) in zip(tp, matches):
        out[c, bucket(a), 0] += 1
        out[c, bucket(a), 3] += (iou.numerator << 24) // iou.denominator
    for k, items in ((1, fp), (2, fn)):
        for c, a in items:
            out[c, bucket(a), k] += 1
    return out


# ---- the cases both test files share: name -> (pred, label, C, LabelPrep keywords, label grid or None), read-only
def _blobs(H, W):
    """Hand-made pairs on a background of class 0 (label and prediction agree on it except under the blobs)."""
    label = np.zeros((H, W), dtype=np.uint8)
    pred = np.zeros((H, W), dtype=np.uint8)
    # IoU exactly 1/2 (no match): label 1 x 4, prediction 1 x 2 inside it: inter 2, union 4
    label[1, 1:5] = 1
    pred[1, 1:3] = 1
    # IoU exactly 2/3 (match): label 1 x 3, prediction 1 x 2 inside it
    label[3, 1:4] = 2
    pred[3, 1:3] = 2
    # one prediction blob over two label segments of one class (the gap is class 0 in the label): 2 x 7 over two 2 x 3
    label[5:7, 1:4] = 3
    label[5:7, 5:8] = 3
    pred[5:7, 1:8] = 3
    # one label segment under two blobs: 2 x 7 under two 2 x 3
    label[8:10, 1:8] = 4
    pred[8:10, 1:4] = 4
    pred[8:10, 5:8] = 4
    return pred, label


def case(name, H, W, C=25):
    """(pred uint8 [B, H, W], label uint8 [B, Hl, Wl], C, LabelPrep keywords, resize or None)."""
    rng = np.random.default_rng(7 * H + W + len(name))
    kw, resize = {}, None
    if name == "same":
        label = np.stack([CR.blocky(rng, H, W, C, 3, 12)])
        pred = label.copy()
    elif name == "shifted":
        label = np.stack([CR.blocky(rng, H, W, C, 4, 15), CR.blocky(rng, H, W, C, 9, 30), CR.blocky(rng, H, W, 3, 9, 30)])
        pred = np.roll(label, 1, 2)
    elif name == "noise":
        label = rng.integers(0, C, size=(1, H, W)).astype(np.uint8)
        pred = rng.integers(0, C, size=(1, H, W)).astype(np.uint8)
    elif name == "patchy":                                 # patches wider than a wave: whole waves share one pair
        label = np.stack([CR.blocky(rng, H, W, C, 40, 90) for _ in range(3)])
        pred = label.copy()
        pred[:, H // 3:H // 2] = np.roll(pred[:, H // 3:H // 2], 7, 2)
    elif name == "checker":                                # at connectivity 4 every pixel is its own segment on both sides, and its own pair
        y, x = np.mgrid[:H, :W]
        label = ((y + x) % 2)[None].astype(np.uint8)
        pred = label.copy()
    elif name == "blobs":
        assert H >= 11 and W >= 9
        pred, label = (m[None] for m in _blobs(H, W))
    elif name == "ignored":                                # ignored regions: area_p excludes them; the blob of class 5 lies wholly inside one
        label = np.stack([CR.blocky(rng, H, W, 6, 4, 15), CR.blocky(rng, H, W, 6, 9, 30)])
        pred = np.roll(label, 2, 1)
        label[0, H // 4:H // 2, W // 4:3 * W // 4] = 255
        label[1, :, W // 2:W // 2 + 3] = 255
        pred[0, H // 4 + 2:H // 2 - 2, W // 4 + 2:3 * W // 4 - 2] = 0
        pred[0, H // 4 + 4:H // 2 - 4, W // 4 + 4:W // 4 + 9] = 5
        label[1, H - 5:, :9] = 40                          # kept, out of range: the code C
        C = 6
    elif name == "lut":                                    # reduce_zero_label, a label_map, nearest-resize tables: the labels live on a smaller grid
        C = 6
        Hl, Wl = max(1, (2 * H) // 3), max(1, (3 * W) // 5)
        label = np.stack([CR.blocky(rng, Hl, Wl, 8, 3, 9), CR.blocky(rng, Hl, Wl, 8, 5, 20)])
        label[0, Hl // 5:Hl // 3, Wl // 3:2 * Wl // 3] = 255
        label[1, Hl // 2:, :Wl // 4] = 40
        kw, resize = dict(reduce_zero_label=True, label_map={3: 1, 5: 255}), (Hl, Wl)
        pred = rng.integers(0, C + 1, size=(2, H, W)).astype(np.uint8)
        pred[:, :H // 2] = CR.blocky(rng, H, W, C, 5, 20)[:H // 2]
    else:
        raise KeyError(name)
    for a in (pred, label):
        a.setflags(write=False)
    return pred, label, C, kw, resize


# ---- the inputs of tests/test_panoptic_gpu.py, listed here so that tests/test_panoptic_cpu.py can predict every table before a GPU sees it
SHAPES = [(1, 1), (5, 7), (32, 64), (70, 45), (130, 97)]      # one pixel; a few; exactly one 64 x 32 tile; ragged tiles; several ragged tiles


def default_capacity(n):
    """The smallest power of two >= n / 2, at least 2."""
    c = 2
    while 2 * c < n:
        c *= 2
    return c


def gpu_cases():
    """(name, H, W, connectivity, capacity, overflows): capacity None = the default of the shape's batch."""
    out = []
    for H, W in SHAPES:
        for conn in (4, 8):
            for name in ("same", "shifted", "noise"):
                out.append((name, H, W, conn, 4 if H * W == 1 else None, False))      # three one-pixel images that agree are three pairs: above the default
            # every pixel its own pair at 4: H * W keys, which the default (half the pixels) cannot hold; four slots per key do
            out.append(("checker", H, W, conn, None if conn == 8 else 2 * default_capacity(4 * H * W), False))
            if H >= 32:
                for name in ("patchy", "ignored", "lut", "blobs"):
                    out.append((name, H, W, conn, None, False))
    out.append(("checker", 32, 64, 4, 2, True))            # 2048 keys, two slots: the bounded loop gives up
    return out


def lut_of(C, kw):
    from tests import eval_ref as ER
    return ER.lut(C, **kw)


def tables_of(label, H, W):
    """(ymap, xmap) of labels [B, Hl, Wl] read on an H x W grid, or (None, None) where the sizes agree."""
    from tests import eval_ref as ER
    Hl, Wl = label.shape[1:]
    return (None, None) if (Hl, Wl) == (H, W) else (ER.nearest_index(Hl, H), ER.nearest_index(Wl, W))
