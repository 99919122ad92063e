"""numpy restatement of the run-length tables (mmsa_run_lengths_u8 / _i32, mmsa_run_decode_i32), written from the definition on the
WHOLE image -- no blocks, no tiles, no prefix sums over units -- TEST INFRASTRUCTURE ONLY.

  flat = m.ravel() (order "row") or m.T.ravel() (order "column");  a head is index 0 and every i > 0 with flat[i] != flat[i - 1]
  count = the heads;  starts[j], values[j] = the flat index and the value of the j-th head, ascending, for j < min(count, capacity)
  length[j] = (starts[j + 1] or H * W) - starts[j]

tests/test_run_length_cpu.py holds it to independent statements; the maps and the case list of the GPU file live here, so that the CPU file can predict every
count against the capacity its test uses."""
import functools

import numpy as np

from tests import segment_table_ref as SR

C = SR.C
ORDERS = ("row", "column")
BLOCK = 2048                       # mmsa.evaluate.RUNS_BLOCK (the flat indices per scan unit), held to it by tests/test_run_length_cpu.py
TILE = 64                          # mmsa.evaluate.RUNS_TILE (the tile edge of the column order's transpose)
SCAN_LANES = 256                   # mmsa.evaluate.SCAN_LANES (the lanes of the compaction's scan workgroup)
SCAN_TRIP = 1024                   # mmsa.evaluate.SCAN_TRIP (the unit counts one trip of the scan takes)


def default_capacity(H, W):
    return max(4096, H * W // 8)


def units(H, W):
    """The scan units of one image: blocks of BLOCK flat indices, in either order."""
    return -(-H * W // BLOCK)


def flat_of(m, order):
    m = np.asarray(m)
    return (m if order == "row" else m.T).ravel()


def runs(m, order):
    """One image [H, W] -> (starts, lengths, values) int64, every run."""
    flat = flat_of(m, order).astype(np.int64)
    starts = np.flatnonzero(np.r_[True, flat[1:] != flat[:-1]])
    return starts, np.diff(starts, append=flat.size), flat[starts]


def table(maps, order, capacity, canary=-7):
    """[B, H, W] -> (count int32 [B], starts, values int32 [B, capacity]): the first min(count, capacity) rows, `canary` in the rows that are not written."""
    B = len(maps)
    count = np.zeros(B, dtype=np.int32)
    starts = np.full((B, capacity), canary, dtype=np.int32)
    values = np.full((B, capacity), canary, dtype=np.int32)
    for b, m in enumerate(maps):
        s, _, v = runs(m, order)
        count[b] = len(s)
        k = min(len(s), capacity)
        starts[b, :k], values[b, :k] = s[:k], v[:k]
    return count, starts, values


def decode(m, order, capacity, fill):
    """What run_decode makes of the table of m at this capacity: m itself where the table holds every run; of an overflowed table the runs before the last
    kept one and that one's head pixel, `fill` past it."""
    m = np.asarray(m)
    s, _, _ = runs(m, order)
    if len(s) <= capacity:
        return m.astype(np.int32)
    flat = flat_of(m, order).astype(np.int32)
    flat[s[capacity - 1] + 1:] = fill
    H, W = m.shape
    return flat.reshape(H, W) if order == "row" else flat.reshape(W, H).T


def rle_mask(rle):
    """An uncompressed COCO RLE -> bool [H, W], by a plain loop over the counts into a Fortran-order mask."""
    H, W = rle["size"]
    flat = np.zeros(H * W, dtype=bool)
    at, one = 0, False
    for c in rle["counts"]:
        assert c >= 0 and at + c <= H * W
        if one:
            flat[at:at + c] = True
        at += c
        one = not one
    assert at == H * W
    return flat.reshape((H, W), order="F")


# ---- the maps both test files share
@functools.lru_cache(maxsize=None)
def image(kind, H, W):
    """[H, W], read-only and shared: uint8, or int32 for "ids"."""
    rng = np.random.default_rng(6151 * H + 17 * W + len(kind))
    if kind in ("one", "blocky", "special", "blobs"):
        return SR.image(kind, H, W)
    if kind == "noise25":                # plain 25-class noise: one pixel in 25 continues its neighbour's run
        return SR.image("noise", H, W)
    if kind == "noise":                  # 25-class noise in which no pixel equals its predecessor in EITHER order, line ends included: every pixel is a run
        m = rng.integers(0, C, size=(H, W)).astype(np.int64)
        for y in range(H):
            for x in range(W):
                near = [m[y, x - 1] if x else (m[y - 1, W - 1] if y else -1), m[y - 1, x] if y else -1]      # the predecessor in row order, and in column order
                if H > 1 and y == H - 1 and x + 1 < W:
                    near.append(m[0, x + 1])                                     # this pixel ends a column: it precedes the next column's first pixel
                while m[y, x] in near:
                    m[y, x] = (m[y, x] + 1) % C
        m = m.astype(np.uint8)
    elif kind == "vstripes":             # columns of one value: the worst case of the row order, the best of the column order
        m = np.broadcast_to(((np.arange(W) // 2) % 5).astype(np.uint8), (H, W)).copy()
    elif kind == "hstripes":
        m = np.broadcast_to(((np.arange(H) // 2) % 5).astype(np.uint8)[:, None], (H, W)).copy()
    elif kind == "seams":                # three-class noise whose line ends continue into the next line on every second line, in both orders
        m = rng.integers(0, 3, size=(H, W)).astype(np.uint8)
        if H >= 4 and W >= 4:
            for x in range(W - 1):
                m[0, x + 1] = (m[H - 1, x] + x % 2) % 3
            for y in range(H - 1):
                m[y + 1, 0] = (m[y, W - 1] + y % 2) % 3
            m[0, 1] = m[H - 1, 0]
    elif kind == "ids":                  # the ids of a segment table (-1 where the code is no class), spread beyond a byte
        ids = SR.table(np.minimum(SR.image("special", H, W), C), SR.image_roots("special", H, W))[1].astype(np.int64)
        m = np.where(ids >= 0, ids * 65537 + 300, -1).astype(np.int32)
    else:
        raise ValueError(kind)
    m.setflags(write=False)
    return m


@functools.lru_cache(maxsize=None)
def count_of(kind, H, W, order):
    return len(runs(image(kind, H, W), order)[0])


KINDS = ("one", "noise", "blocky", "vstripes", "hstripes", "seams")
EDGES = [(H, W) for H in (TILE - 1, TILE, TILE + 1) for W in (TILE - 1, TILE, TILE + 1)]      # one below, at and one above the column tile in each axis
LINES = [(1, BLOCK - 1), (1, BLOCK), (1, BLOCK + 1)]                                           # the same for the scan block
SHAPES = [(1, 1), (1, 131), (67, 1)] + EDGES + LINES + [(67, 131), (130, 200)]
MANY = [(67, 131), (130, 200)]     # several scan blocks, and several transpose tiles with ragged edges in each axis
LARGE = (1400, 1502)               # 1027 scan blocks: more than the scan workgroup has lanes, and more than one trip of the scan takes

# every input of tests/test_run_length_gpu.py: (kind, H, W, capacity, overflows in (row, column)); capacity "HW" = H * W, None = the default, "count-1" = one
# row fewer than the runs of that order.  The CPU file predicts the count of each in both orders against it.
CASES = ([(kind, H, W, "HW", (False, False)) for H, W in SHAPES for kind in KINDS]
         + [("ids", H, W, "HW", (False, False)) for H, W in MANY + [(TILE + 1, TILE + 1)]]
         + [("noise25", LARGE[0], LARGE[1], "HW", (False, False))]
         + [(kind, 67, 131, cap, (True, True)) for kind in ("noise", "seams") for cap in ("count-1", 1)]
         + [("blocky", 130, 200, None, (False, False)), ("noise", 130, 200, None, (True, True))]
         + [(kind, 50, 70, "HW", (False, False)) for kind in ("blocky", "seams", "one")])      # the batch of three


def capacity_of(kind, H, W, capacity, order):
    return {"HW": H * W, None: default_capacity(H, W), "count-1": count_of(kind, H, W, order) - 1}.get(capacity, capacity)
