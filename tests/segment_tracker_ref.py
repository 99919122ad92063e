"""numpy restatement of the segment tracker (mmsa_track_pairs, mmsa_track_update), written from the definition on whole frames -- no hash
table, no waves, no scan in trips -- TEST INFRASTRUCTURE ONLY.  It works on sequences of (count, ids, records) as tests/segment_table_ref.py produces them.

  image b of one update follows image b of the previous one; R = the table's rows per image; a segment of either frame takes part iff its id is in [0, R)
  inter(k, j) = the pixels with ids_cur == k and ids_prev == j;  k CONTINUES j iff 3 * inter > AREA_k + AREA_j and (same_class) CLASS_k == CLASS_j
  state[k] = TRACK, AGE, PREV, INTER for k < min(count, R): the predecessor's TRACK, AGE + 1, j, inter -- or next_track + (non-continuing rows k' < k), 1, -1, 0;
  (-1, 0, -1, 0) behind;  stats = continued, born, ended (previous rows in [0, min(prev_count, R)) that nothing continues), ADDED to totals

tests/test_segment_tracker_cpu.py holds it to a brute-force statement from sets of pixels and Fractions; the sequences and the case list of the GPU file live
here, so that the CPU file can predict the pair table of every update the GPU file makes."""
import functools
from fractions import Fraction

import numpy as np

from tests import components_ref as CR
from tests import segment_table_ref as SR

TRACK, AGE, PREV, INTER = range(4)
C = SR.C
TRIP = 1024                        # mmsa.evaluate.TRACK_TRIP, held to it by tests/test_segment_tracker_cpu.py
UNMATCHED = (-1, 0, -1, 0)


def pairs_of(ids_cur, ids_prev, R):
    """[B, H, W] each -> (keys int64 sorted, counts int64): key = ((b * R + id_cur) << 31) | id_prev over the pixels whose two ids lie in [0, R)."""
    cur, prev = np.asarray(ids_cur).astype(np.int64), np.asarray(ids_prev).astype(np.int64)
    b = np.arange(cur.shape[0], dtype=np.int64).reshape(-1, 1, 1)
    part = (cur >= 0) & (cur < R) & (prev >= 0) & (prev < R)
    keys = (((b * R + cur) << 31) | prev)[part]
    return np.unique(keys, return_counts=True)


class Tracker:
    """The restatement's state for B images of R rows; update(count, ids, records) -> dict of what the device leaves after one SegmentTracker.update()."""

    def __init__(self, B, R, same_class=True):
        self.B, self.R, self.same_class = B, R, same_class
        self.prev = [None] * B           # per image: (n, ids [H, W], CLASS [n], AREA [n], TRACK [n], AGE [n]) or None: no previous frame
        self.next_track = np.zeros(B, dtype=np.int32)
        self.totals = np.zeros((B, 3), dtype=np.int64)

    def reset(self, b=None):
        for i in range(self.B) if b is None else [b]:
            self.prev[i] = None
            self.next_track[i] = 0

    def update(self, count, ids, records):
        B, R = self.B, self.R
        ids, records = np.asarray(ids), np.asarray(records)
        assert ids.shape[0] == B and records.shape[:2] == (B, R)
        state = np.tile(np.array(UNMATCHED, dtype=np.int32), (B, R, 1))
        succ, prev_area = np.full((B, R), -1, dtype=np.int32), np.zeros((B, R), dtype=np.int32)
        stats, tracks = np.zeros((B, 3), dtype=np.int32), np.full(ids.shape, -1, dtype=np.int32)
        prev_ids = np.stack([np.full(ids.shape[1:], -1, dtype=np.int32) if p is None else p[1] for p in self.prev])
        keys, inters = pairs_of(ids, prev_ids, R)
        for b in range(B):
            n = min(int(count[b]), R)
            cls, area = records[b, :n, SR.CLASS], records[b, :n, SR.AREA]
            p = self.prev[b]
            n_prev = 0 if p is None else p[0]
            for key, inter in zip(keys.tolist(), inters.tolist()):
                g, j = key >> 31, key & ((1 << 31) - 1)
                if g // R != b:
                    continue
                k = g % R
                assert k < n and j < n_prev
                if 3 * inter > int(area[k]) + int(p[3][j]) and (not self.same_class or cls[k] == p[2][j]):
                    assert state[b, k, PREV] == -1 and succ[b, j] == -1      # uniqueness, both ways
                    state[b, k, PREV], state[b, k, INTER], prev_area[b, k], succ[b, j] = j, inter, p[3][j], k
            born = 0
            for k in range(n):
                j = state[b, k, PREV]
                if j < 0:
                    state[b, k, TRACK], state[b, k, AGE] = self.next_track[b] + born, 1
                    born += 1
                else:
                    state[b, k, TRACK], state[b, k, AGE] = p[4][j], p[5][j] + 1
            ended = int((succ[b, :n_prev] < 0).sum())
            stats[b] = n - born, born, ended
            self.next_track[b] += born
            inside = (ids[b] >= 0) & (ids[b] < R)
            tracks[b] = np.where(inside, state[b, np.clip(ids[b], 0, R - 1), TRACK], -1)
            self.prev[b] = (n, ids[b].astype(np.int32), cls.copy(), area.copy(), state[b, :n, TRACK].copy(), state[b, :n, AGE].copy())
        self.totals += stats
        return dict(state=state, stats=stats, totals=self.totals.copy(), next_track=self.next_track.copy(), tracks=tracks, keys=keys, inters=inters,
                    prev_area=prev_area, succ=succ)


def keep(state, min_age=None, max_age=None, tracks=None):
    """uint8 [..., R]: the rows with a track that pass."""
    s = np.asarray(state)
    ok = s[..., TRACK] >= 0
    if min_age is not None:
        ok &= s[..., AGE] >= min_age
    if max_age is not None:
        ok &= s[..., AGE] < max_age
    if tracks is not None:
        ok &= np.isin(s[..., TRACK], list(tracks))
    return ok.astype(np.uint8)


def brute_force(ids_cur, classes_cur, ids_prev, classes_prev, R, same_class=True):
    """One image, from sets of pixels: {k: (j, Fraction IoU)} over the segments with ids in [0, R): IoU = |k & j| / |k | j| as a Fraction, match iff > 1/2
    and (same_class) equal classes.  EVERY qualifying pair is returned as a list per k, so that uniqueness is the caller's to see."""
    cur, prev = np.asarray(ids_cur).ravel(), np.asarray(ids_prev).ravel()
    sets_cur = {int(k): set(np.flatnonzero(cur == k).tolist()) for k in np.unique(cur) if 0 <= k < R}
    sets_prev = {int(j): set(np.flatnonzero(prev == j).tolist()) for j in np.unique(prev) if 0 <= j < R}
    out = {}
    for k, pk in sets_cur.items():
        for j in {int(prev[i]) for i in pk if 0 <= prev[i] < R}:
            pj = sets_prev[j]
            iou = Fraction(len(pk & pj), len(pk | pj))
            if iou > Fraction(1, 2) and (not same_class or classes_cur[k] == classes_prev[j]):
                out.setdefault(k, []).append((j, iou))
    return out


# ---- the sequences both test files share (their own seeds)
def _shift(m, dy, dx, fill):
    """m moved down by dy and right by dx; what comes in takes `fill` (an array of m's shape)."""
    out = fill.copy()
    H, W = m.shape
    out[dy:, dx:] = m[:H - dy, :W - dx]
    return out


def moving(seed, H, W, T, salt=0.02, classes=C, lo=3, hi=12):
    """T frames uint8 [H, W]: a blocky map shifted by 0-2 px down and right per frame, a `salt` share of the pixels re-drawn in every frame."""
    rng = np.random.default_rng(seed)
    frames = [CR.blocky(rng, H, W, classes, lo, hi)]
    for _ in range(T - 1):
        dy, dx = (int(v) for v in rng.integers(0, 3, size=2))
        frames.append(_shift(frames[-1], min(dy, H - 1), min(dx, W - 1), CR.blocky(rng, H, W, classes, lo, hi)))
    out = []
    for f in frames:
        redraw = rng.random((H, W)) < salt
        out.append(np.where(redraw, rng.integers(0, classes, size=(H, W)), f).astype(np.uint8))
    return out


def blobs(seed=5, H=40, W=60, density=(0.05, 0.05, 0.75, 0.75, 0.05)):
    """Five frames of 25-class blobs shifted by 1-2 px per frame with salt noise.  The salt FIELD is one noise map that stays in place; a frame shows it at a
    random `density` of its pixels -- frames 2 and 3 at three quarters, so that they hold more than TRIP segments and share single-pixel segments."""
    rng = np.random.default_rng(seed)
    base = CR.blocky(rng, H, W, C, 6, 14)
    field = rng.integers(0, C, size=(H, W)).astype(np.uint8)
    out = []
    for d in density:
        out.append(np.where(rng.random((H, W)) < d, field, base).astype(np.uint8))
        dy, dx = (int(v) for v in rng.integers(1, 3, size=2))
        base = _shift(base, dy, dx, CR.blocky(rng, H, W, C, 6, 14))
    return out


def hand():
    """Two frames uint8 [24, 20] on a background of class 0 (one segment at connectivity 8, which continues itself).  Row y holds one case each; the returned
    dict names a pixel of every segment of interest: name -> (frame, y, x)."""
    a, b = np.zeros((24, 20), dtype=np.uint8), np.zeros((24, 20), dtype=np.uint8)
    at = {}
    a[1, 2:5], b[1, 3:6] = 5, 5                      # half: a bar of 3 moved by 1 -- inter 2, union 4: IoU exactly 1/2, no match
    at["half_prev"], at["half_cur"] = (0, 1, 2), (1, 1, 5)
    a[3, 2:7], b[3, 3:8] = 5, 5                      # two thirds: a bar of 5 moved by 1 -- inter 4, union 6
    at["twothirds_prev"], at["twothirds_cur"] = (0, 3, 2), (1, 3, 7)
    a[5, 2:12] = 7                                   # split 6 | gap | 3: the left part has IoU 6 / 10 and inherits, the right part is born
    b[5, 2:8], b[5, 9:12] = 7, 7
    at["split_prev"], at["split_left"], at["split_right"] = (0, 5, 2), (1, 5, 2), (1, 5, 11)
    a[7, 2:12] = 7                                   # split 5 | gap | 4: 5 / 10 is exactly 1/2 -- both are born, the old track ends
    b[7, 2:7], b[7, 8:12] = 7, 7
    at["even_prev"], at["even_left"], at["even_right"] = (0, 7, 2), (1, 7, 2), (1, 7, 11)
    a[9, 2:9], a[9, 10:12] = 8, 8                    # merge 7 | gap | 2 -> 10: 7 / 10 inherits the long one's track, the short one ends
    b[9, 2:12] = 8
    at["merge_long"], at["merge_short"], at["merge_cur"] = (0, 9, 2), (0, 9, 11), (1, 9, 2)
    a[11, 2:7], a[11, 8:12] = 8, 8                   # merge 5 | gap | 4 -> 10: nobody inherits
    b[11, 2:12] = 8
    at["tie_a"], at["tie_b"], at["tie_cur"] = (0, 11, 2), (0, 11, 11), (1, 11, 2)
    a[14:17, 3:6], b[14:17, 3:6] = 4, 9              # a block that changes class in place: IoU 1
    at["class_prev"], at["class_cur"] = (0, 14, 3), (1, 14, 3)
    a[19:22, 3:6] = 6                                # a block that is gone in the next frame: ended
    b[19:22, 12:15] = 6                              # and one that was not there: born
    at["gone"], at["new"] = (0, 19, 3), (1, 19, 12)
    return [a, b], at


VOID = 255


@functools.lru_cache(maxsize=None)
def sequence(name):
    """-> the frames of a named sequence, a tuple of read-only uint8 [B, H, W] batches."""
    if name == "1x1":
        frames = [np.full((1, 1, 1), v, dtype=np.uint8) for v in (3, 3, 5, VOID, 5)]
    elif name == "row":
        frames = [f[None] for f in moving(11, 1, 257, 3, salt=0.05)]
    elif name == "column":
        frames = [f[None] for f in moving(12, 257, 1, 3, salt=0.05)]
    elif name in ("w63", "w64", "w65"):
        frames = [f[None] for f in moving(int(name[1:]), 3, int(name[1:]), 3, salt=0.05, lo=3, hi=9)]
    elif name == "ragged":           # three images that must not see each other: the same seed family, different maps
        per = [moving(100 + b, 67, 131, 4, lo=12, hi=30) for b in range(3)]
        frames = [np.stack([per[b][t] for b in range(3)]) for t in range(4)]
    elif name == "twins":            # three images with the SAME frames: what one image does, every image does
        one = moving(7, 20, 33, 3)
        frames = [np.stack([f] * 3) for f in one]
    elif name == "blobs":
        frames = [f[None] for f in blobs()]
    elif name == "blobs_again":      # the last frame three more times: a frame against itself, every segment continues itself
        frames = [f[None] for f in blobs()] + [blobs()[4][None].copy() for _ in range(3)]
    elif name == "gap":              # a frame with no listed segment between two that have some
        f = moving(21, 30, 45, 2)
        frames = [f[0][None], np.full((1, 30, 45), VOID, dtype=np.uint8), f[0][None], f[1][None]]
    elif name == "hand":
        frames = [f[None] for f in hand()[0]]
    elif name == "noise":            # more segments than a small table has rows
        rng = np.random.default_rng(31)
        base = rng.integers(0, C, size=(31, 63)).astype(np.uint8)
        frames = [base[None], base[None], _shift(base, 0, 1, base)[None]]
    else:
        raise KeyError(name)
    for f in frames:
        f.setflags(write=False)
    return tuple(frames)


@functools.lru_cache(maxsize=None)
def tables(name, capacity=None, connectivity=8):
    """-> per frame (count int32 [B], ids int32 [B, H, W], records int64 [B, capacity, 10]) of the named sequence: min_area 1, classes only; capacity None: H * W."""
    out = []
    for f in sequence(name):
        codes = np.minimum(f, C)
        out.append(SR.table_batch(codes, [CR.roots(c, connectivity) for c in codes], capacity=capacity))
    return tuple(out)


def run(name, capacity=None, same_class=True, resets=()):
    """The restatement over the named sequence -> the list of update() results; `resets` = ((frame index t, image b or None), ...): reset before frame t."""
    tabs = tables(name, capacity)
    B, R = tabs[0][2].shape[:2]
    tr = Tracker(B, R, same_class)
    out = []
    for t, (count, ids, records) in enumerate(tabs):
        for at, b in resets:
            if at == t:
                tr.reset(b)
        out.append(tr.update(count, ids, records))
    return out


# every tracker of tests/test_segment_tracker_gpu.py: (sequence, capacity (None: H * W), same_class, pair_capacity (None: the default), resets, overflows).  The
# CPU file predicts the pair table of every update of each: no key can be dropped, or -- where `overflows` -- some key must be.
CASES = ([(name, None, True, None, (), False) for name in ("1x1", "row", "column", "w63", "w64", "w65", "ragged", "twins", "gap")]
         + [("blobs", None, True, 8192, (), False), ("blobs_again", None, True, 8192, (), False)]      # its noisy frames form about 1800 pairs: the default of 2048 slots would be nearly full
         + [("hand", None, True, None, (), False), ("hand", None, False, None, (), False)]
         + [("ragged", None, True, None, ((2, 1),), False), ("ragged", None, False, None, (), False)]
         + [("noise", 100, True, None, (), False), ("ragged", None, True, 2, (), True)])
