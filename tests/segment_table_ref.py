"""numpy restatement of the segment table (mmsa_segment_table, mmsa_select_segments_u8), written from the definitions on the WHOLE image --
no blocks, no prefix sums over blocks, no waves -- TEST INFRASTRUCTURE ONLY.

  a component of an image is LISTED iff its area >= min_area and its code is a class (< C); void=True also lists the components of the other codes
  the listed segments are numbered 0 .. n - 1 in ascending order of their root index;  ids[p] = the number of p's segment, -1 where it is not listed
  records[k] = ROOT, CLASS, AREA, X0, Y0, X1, Y1, SUM_X, SUM_Y, SUM_Q for k < min(n, capacity), zero rows behind;  SUM_Q = sum of floor(clamp(v) * 2^24)

tests/test_segment_table_cpu.py holds it to scipy.ndimage (label per class, find_objects, sum_labels, center_of_mass); the maps and the case list of the GPU file
live here, so that the CPU file can predict every n_b against the capacity its test uses."""
import functools

import numpy as np

from tests import components_ref as CR

ROOT, CLASS, AREA, X0, Y0, X1, Y1, SUM_X, SUM_Y, SUM_Q = range(10)
FIELDS = 10
C = 25
ONE = 1 << 24


def default_capacity(H, W):
    return max(1024, H * W // 64)


def q24(values):
    """floor(clamp(v) * 2^24) as int64: NaN, negatives and -0.0 -> 0, above 1 and +inf -> 1; ONE float32 product, truncated."""
    v = np.asarray(values, dtype=np.float32)
    with np.errstate(invalid="ignore"):
        c = np.where(v > 0, np.where(v > 1, np.float32(1), v), np.float32(0)).astype(np.float32)
    return (c * np.float32(ONE)).astype(np.int64)


def table(code, root, num_classes=C, min_area=1, void=False, capacity=None, values=None):
    """One image: code uint8 [H, W], root int32 [H, W] -> (n, ids int32 [H, W], records int64 [capacity, 10]); capacity None: H * W."""
    code, root = np.asarray(code), np.asarray(root)
    H, W = code.shape
    HW = H * W
    r, c = root.ravel().astype(np.int64), code.ravel().astype(np.int64)
    area = np.bincount(r, minlength=HW)
    listed = (r == np.arange(HW)) & (area >= min_area) & ((c < num_classes) | bool(void))
    rank = np.cumsum(listed) - listed
    ids = np.where(listed[r], rank[r], -1)
    n = int(listed.sum())
    rec = np.zeros((n, FIELDS), dtype=np.int64)
    at = ids >= 0
    k = ids[at]
    y, x = np.divmod(np.arange(HW), W)
    rec[:, ROOT] = np.nonzero(listed)[0]
    rec[:, CLASS] = c[rec[:, ROOT]]
    rec[:, X0], rec[:, Y0] = W, H
    rec[:, X1] = rec[:, Y1] = -1
    np.add.at(rec[:, AREA], k, 1)
    np.minimum.at(rec[:, X0], k, x[at])
    np.minimum.at(rec[:, Y0], k, y[at])
    np.maximum.at(rec[:, X1], k, x[at])
    np.maximum.at(rec[:, Y1], k, y[at])
    np.add.at(rec[:, SUM_X], k, x[at])
    np.add.at(rec[:, SUM_Y], k, y[at])
    if values is not None:
        np.add.at(rec[:, SUM_Q], k, q24(values).ravel()[at])
    cap = HW if capacity is None else int(capacity)
    out = np.zeros((cap, FIELDS), dtype=np.int64)
    out[:min(n, cap)] = rec[:cap]
    return n, ids.reshape(H, W).astype(np.int32), out


def table_batch(codes, roots, **kw):
    """[B, H, W] each -> (count int32 [B], ids int32 [B, H, W], records int64 [B, capacity, 10]); values= [B, H, W] or None."""
    values = kw.pop("values", None)
    parts = [table(c, r, values=None if values is None else values[b], **kw) for b, (c, r) in enumerate(zip(codes, roots))]
    return np.array([p[0] for p in parts], dtype=np.int32), np.stack([p[1] for p in parts]), np.stack([p[2] for p in parts])


def keep(records, min_area=None, max_area=None, min_score_q=None, classes=None):
    """uint8 [..., capacity]: the rows that pass, in integers; empty rows are 0."""
    r = np.asarray(records)
    ok = r[..., AREA] > 0
    if min_area is not None:
        ok &= r[..., AREA] >= min_area
    if max_area is not None:
        ok &= r[..., AREA] < max_area
    if min_score_q is not None:
        ok &= r[..., SUM_Q] >= min_score_q * r[..., AREA]
    if classes is not None:
        ok &= np.isin(r[..., CLASS], list(classes))
    return ok.astype(np.uint8)


def select(pred, ids, keep_mask, fill=255):
    """uint8 [B, H, W]: fill where 0 <= id < capacity and keep[b, id] == 0, pred elsewhere."""
    pred, ids, keep_mask = np.asarray(pred), np.asarray(ids), np.asarray(keep_mask)
    cap = keep_mask.shape[1]
    inside = (ids >= 0) & (ids < cap)
    kept = np.take_along_axis(keep_mask, np.clip(ids, 0, cap - 1).reshape(ids.shape[0], -1), 1).reshape(ids.shape)
    return np.where(inside & (kept == 0), fill, pred).astype(np.uint8)


# ---- the maps both test files share (their own seeds)
@functools.lru_cache(maxsize=None)
def image(kind, H, W):
    """uint8 [H, W], read-only and shared."""
    rng = np.random.default_rng(7919 * H + 31 * W + len(kind))
    if kind == "noise":
        m = rng.integers(0, C, size=(H, W)).astype(np.uint8)
    elif kind == "blocky":
        m = CR.blocky(rng, H, W, C)
    elif kind == "special":      # regions of the bytes C, C + 3 and 255 (ONE code of a class map, min(v, C)) next to classes
        m = CR.blocky(rng, H, W, 4, 5, 11)
        m[H // 5:H // 2, W // 4:W // 2] = C
        m[H // 3:2 * H // 3, W // 2:3 * W // 4] = 255
        m[H // 2:H // 2 + 3, :] = C + 3
    elif kind == "blobs":        # three classes of noise: components of every small size, and a few large ones
        m = rng.integers(0, 3, size=(H, W)).astype(np.uint8)
    elif kind == "one":
        m = np.full((H, W), 7, dtype=np.uint8)
    else:
        m = getattr(CR, kind)(H, W)
    m.setflags(write=False)
    return m


@functools.lru_cache(maxsize=None)
def image_roots(kind, H, W, connectivity=8, num_classes=C):
    r = CR.roots(np.minimum(image(kind, H, W), num_classes), connectivity)
    r.setflags(write=False)
    return r


@functools.lru_cache(maxsize=None)
def image_values(kind, H, W):
    """float32 [H, W] in [0, 1]; kind "nasty": NaN, +-inf, negatives, -0.0, denormals, exactly 1.0 and values above 1 scattered over it."""
    rng = np.random.default_rng(104729 + 7 * H + W)
    v = rng.random((H, W), dtype=np.float32)
    if kind == "nasty":
        odd = np.array([np.nan, np.inf, -np.inf, -1.5, -0.0, 1e-41, -1e-41, 1.0, 1.0000001, 7.0, 0.0, np.float32(1) - np.float32(2) ** -24], dtype=np.float32)
        at = rng.integers(0, odd.size + 6, size=(H, W))
        v = np.where(at < odd.size, odd[np.minimum(at, odd.size - 1)], v).astype(np.float32)
    v.setflags(write=False)
    return v


SHAPES = [(1, 1), (1, 257), (257, 1), (31, 63), (67, 131), (130, 200)]
BLOCK = 2048                       # mmsa.evaluate.SEGTAB_BLOCK, held to it by tests/test_segment_table_cpu.py
LARGE = (600, 900)                 # 264 scan blocks of 2048 pixels: more than the 256 lanes of the scan workgroup (mmsa.evaluate.SCAN_LANES)
LARGER = (1400, 1502)              # 1027 scan blocks: more than the 1024 counts of one trip of the scan (mmsa.evaluate.SCAN_TRIP), so the carry is used

# every input of tests/test_segment_table_gpu.py: (kind, H, W, connectivity, min_area, void, capacity (None: the default), overflows).  The CPU file predicts
# n_b of each against its capacity: exactly the cases marked so overflow.
CASES = ([(kind, H, W, conn, 1, False, H * W, False) for H, W in SHAPES for conn in (4, 8) for kind in ("noise", "blocky", "special")]
         + [(kind, H, W, 8, 1, False, H * W, False) for kind, H, W in (("one", 67, 131), ("one", 130, 200), ("spiral", 67, 131), ("serpentine", 67, 131),
                                                                      ("comb", 67, 131))]
         + [("noise", 1, BLOCK + d, 8, 1, False, BLOCK + d, False) for d in (-1, 0, 1)]
         + [(kind, H, W, 8, 1, False, 96 * 160, False) for kind, H, W in (("noise", 96, 160), ("blocky", 96, 160), ("one", 96, 160), ("blocky", 50, 70),
                                                                           ("special", 50, 70))]      # the batches through one SegmentTable(capacity=96 * 160)
         + [("blobs", 67, 131, conn, a, v, 67 * 131, False) for a in (1, 2, 5, 64) for v in (False, True) for conn in (4, 8)]
         + [("special", 67, 131, 8, a, True, 67 * 131, False) for a in (1, 64)]
         + [("noise", 31, 63, 8, 1, False, None, True)]
         + [("blocky", 67, 131, 8, 1, True, 67 * 131, False), ("noise", 31, 63, 8, 1, True, 31 * 63, False), ("special", 67, 131, 4, 1, True, 67 * 131, False)])
