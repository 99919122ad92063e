"""The second and third trip of every kernel whose workgroups walk a list of items, tiles or elements, held to float64 and to the bits of the first trip.

wattn_persist_kernel (csrc/wattn.hip) launches at most one workgroup per CU and dwconv7_blk_kernel (csrc/conv.hip) at most two; gelu_gate / ca_apply /
lnhw_apply stop at 8192 blocks, im2col_nchw at 16384 and the generic gconv_nhwc_kernel at 32768.  None of them has a grid-cap argument, so only a problem
larger than the grid sends a workgroup round its loop again -- into the next item's K DMA behind barrier #2, the counted `s_waitcnt vmcnt(4)`, the Q loads at the
loop's end and `decode(it_next)` next to the current item's store (wattn); into the register prefetch, the barriers around to_lds() and the re-decode of image,
chunk, weights and bias (dwconv7_blk); into the stride of the element loops.  Every case here is sized from the device's CU count n, and every test asserts from
its own shape arithmetic the trips it claims (walk_facts / dw7_facts / STRIDE), so that a part with another CU count cannot turn it back into a one-trip test.

An item's result cannot depend on the trip that computes it: each large launch is compared BIT FOR BIT with the same work done in launches that stay at one
trip (one image = one item per workgroup; sub-batches of at most 2n / 6 images; row or image chunks below the block cap) -- the path the existing unit tests hold
to float64 -- and then, like those, with float64 itself: ref_attention under the existing ("window", vf, fmt) bounds of tests/test_attention_gpu.py, image by
image, and the element-wise bounds of tests/variant_ref.py.  Outputs are NaN-filled first: an item that no trip reaches shows.

tests/test_persistent_walks_cpu.py checks the shape helpers at other CU counts, the bounds on the CPU, and the max |logit| >= 4 precondition of every image.

Measured on an MI355X (n = 256; the grid is the one the restated cost model picks; worst figure over the case's images / elements):
  window ws7        2 heads  B 13  520 items  grid 174: 172 workgroups x 3 trips, 2 x 2      max_rel  vf 0: b3 5.2e-6  h8c 2.3e-5    vf 2: b3 1.3e-4  h8c 1.4e-4
  window ws14       2 heads  B 29  522 items  grid 256:  10 workgroups x 3 trips, 246 x 2    max_rel  vf 0: b3 6.0e-6  h8c 3.9e-5    vf 2: b3 1.5e-4  h8c 1.5e-4
  window ws7_h3     3 heads  B 10  600 items  grid 200: 200 workgroups x 3 trips             max_rel  vf 0: b3 7.2e-6  h8c 2.8e-5    vf 2: b3 1.6e-4  h8c 1.7e-4
  window ws7_mixed  3 heads  B  5  300 items  grid 256:  44 workgroups x 2 trips, 212 x 1    max_rel  h8c: vf 0 2.9e-5  vf 2 1.4e-4
      (bounds, tests/test_attention_gpu.py TOL: vf 0 b3 9.2e-6, h8c 4.8e-5; vf 2 2.2e-4.)
      With two heads both grids are even and a workgroup never changes head: `head` == `head_cur` throughout.  In the three-head cases every second and third
      trip changes head (grid 200 or 256, neither a multiple of 3); a kernel that addressed its store with `head` in place of `head_cur` passed every two-head
      case and failed all six three-head ones.
  dw7-blk       B 174  1044 tiles grid 512:  20 workgroups x 3 trips, 492 x 2    worst |y - r| / bound  0.119 (one weight set)  0.151 (two groups, bias)
  gelu_gate / ca_apply / lnhw   2 129 920 float4, 8192 blocks: 32 768 on a second trip     worst |y - r| / bound  0.354 / 0.238 / 0.566
  gconv k = 1 + bias            8 519 680 outputs, 32768 blocks: 131 072 on a second trip   worst |y - r| / bound  0.326
  im2col_nchw                   4 239 872 elements, 16384 blocks: 45 568 on a second trip   exact
"""
import pytest
import torch

from tests import variant_ref as V
from tests.test_attention_gpu import B3, FMT_NAME, H8C, check_guard, check_leaf, make_problem, ref_attention, run_fused
from tests.test_kernel_variants_gpu import bits, dev, nanbuf, planes_equal_split, run_ca_apply, run_dwconv, run_gconv, run_gelu_gate, run_lnhw

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
HD = 64


def cdiv(a, b):
    return -(-a // b)


# ------------------------------------------------------------------------------------------------ shapes from the CU count (pure arithmetic: the CPU companion runs it too)
# windowed attention: name -> (H, W, window size, heads, seed of make_problem)
#   ws7    23 x 31: T = 713 is odd (h8c row pairs straddle images); 4 x 5 windows, live_h = 2, live_w = 3: 12 interior + 8 overhanging windows, 40 items per image
#   ws14   30 x 30: the model's window; 3 x 3 windows, 2 live rows / columns in the last ones: 4 interior + 5 overhanging, whole waves without a live query
#   ws7_h3 the ws7 image with THREE heads.  An item's head is item % heads (heads x B items per window), so a workgroup changes head between two of its items
#          exactly when its grid is no multiple of the head count.  With two heads and the even grids of a 256-CU part (174, 256) it never does: `head` and
#          `head_cur` of the item loop are then always equal and a store addressed with the wrong one of them would pass.  Three heads and a batch chosen so that
#          NEITHER grid the launcher may pick is a multiple of 3 make every workgroup change head on every trip, whichever grid runs.
#   ws7_mixed   the ws7 image, three heads, at a batch with n < items < 2n: under the one-per-CU grid some workgroups stop after one trip while others go on to
#          an item of another head
WATTN = {"ws7": (23, 31, 7, 2, 107), "ws14": (30, 30, 14, 2, 114), "ws7_h3": (23, 31, 7, 3, 131), "ws7_mixed": (23, 31, 7, 3, 207)}
THREE_TRIPS = ("ws7", "ws14", "ws7_h3")


def wattn_windows(H, W, ws):
    """(windows per image, interior windows per image): interior = neither in the last window row nor in the last window column (wattn.hip `decode`)."""
    nh, nw = cdiv(H, ws), cdiv(W, ws)
    return nh * nw, (nh - 1) * (nw - 1)


def wattn_grids(items, n):
    """The two grids the launcher chooses between: the fewest workgroups that finish in ceil(items / n) trips, and one per CU."""
    return cdiv(items, cdiv(items, n)), min(items, n)


def wattn_batch(geom, n):
    """ws7 / ws14: the smallest batch with items >= 2n + 1 (three trips under any grid of at most n workgroups).  ws7_h3: the smallest such batch, among the next
    eight, for which neither candidate grid is a multiple of the head count (walk_facts fails on a part where there is none).  ws7_mixed: the smallest with items > n."""
    H, W, ws, heads, _ = WATTN[geom]
    per = wattn_windows(H, W, ws)[0] * heads
    if geom == "ws7_mixed":
        return n // per + 1
    B0 = cdiv(2 * n + 1, per)
    if geom == "ws7_h3":
        return next((B for B in range(B0, B0 + 8) if all(g % heads for g in wattn_grids(per * B, n))), B0)
    return B0


def wattn_launch_grid(H, W, ws, heads, B, n):
    """The launcher's choice between the two (mmsa_window_attention_planes, RESTATED here: nothing reports the grid a launch really used): the cheaper schedule by
    its two-class cost model -- an interior item costs 1, an overhanging one 0.35 + 0.65 x its share of live query rows and columns; a workgroup's cost is the sum
    over its items, a schedule's the largest.  What depends on this restatement staying in step with wattn.hip: the trips printed by the tests, and the assertions
    of the ws7_mixed case (walk_facts).  Every assertion of the three-trip cases is made for BOTH candidate grids and does not depend on it."""
    nh, nw, nhb = cdiv(H, ws), cdiv(W, ws), heads * B
    items, n_int = nh * nw * nhb, (nh - 1) * (nw - 1) * nhb
    edge = 0.35 + 0.65 * (0.5 * ((H - (nh - 1) * ws) + (W - (nw - 1) * ws)) / ws)

    def cost(G):
        worst = 0.0
        for g in range(G):
            c = 0.0
            for it in range(g, items, G):
                c += 1.0 if it < n_int else edge
            worst = max(worst, c)
        return worst
    grid, grid_all = wattn_grids(items, n)
    return grid_all if cost(grid_all) < cost(grid) - 1e-9 else grid


def walk_shape(geom, n):
    """The trip-count conditions of a case at n CUs, from the item count and the two candidate grids alone; -> (B, items)."""
    H, W, ws, heads, _ = WATTN[geom]
    nwin = wattn_windows(H, W, ws)[0]
    B = wattn_batch(geom, n)
    items = nwin * heads * B
    assert nwin * heads <= n, "a one-image launch must be one item per workgroup"
    one_per_cu = [len(range(g, items, n)) for g in range(n)]
    assert min(one_per_cu) < max(one_per_cu), "the last round of the one-per-CU grid must be ragged (has_next differs between workgroups)"
    if geom == "ws7_mixed":
        assert n < items < 2 * n and (min(one_per_cu), max(one_per_cu)) == (1, 2)
    else:
        assert items >= 2 * n + 1
        for grid in wattn_grids(items, n):
            assert cdiv(items, grid) >= 3, (items, grid)
    return B, items


def walk_of(geom, B, grid):
    """(trips -> workgroups, what consecutive items of a workgroup differ in) under `grid` workgroups.  item -> (interior window?, image, head) as wattn.hip's
    `decode`: items are window-major, interior windows first, then (image, head) within a window."""
    H, W, ws, heads, _ = WATTN[geom]
    nwin, nint = wattn_windows(H, W, ws)
    nhb = heads * B
    items = nwin * nhb
    walks = [[(it // nhb < nint, (it % nhb) // heads, it % heads) for it in range(g, items, grid)] for g in range(grid)]
    pairs = [(a, b) for w in walks for a, b in zip(w, w[1:])]
    trips = [len(w) for w in walks]
    mix = dict(interior_then_overhanging=sum(a[0] and not b[0] for a, b in pairs), image_changes=sum(a[1] != b[1] for a, b in pairs),
               head_changes=sum(a[2] != b[2] for a, b in pairs))
    return {t: trips.count(t) for t in sorted(set(trips))}, mix


def walk_facts(geom, n):
    """walk_shape, and what a workgroup's list mixes; -> (B, items, the grid the cost model picks, its trips -> workgroups, its mix).
    Three-trip cases, under BOTH candidate grids: some workgroup follows an interior window with an overhanging one; ws7_h3: workgroups change head.
    ws7_mixed, under the grid the restated cost model picks (the other candidate, ceil(items / 2), would give every workgroup two trips): workgroups of one trip
    and of two, and a head change in front of the second.
    Image changes are reported, not asserted: a grid that is a multiple of heads x B (ws14 at 256 CUs under the 174-workgroup candidate) has none."""
    H, W, ws, heads, _ = WATTN[geom]
    B, items = walk_shape(geom, n)
    grid = wattn_launch_grid(H, W, ws, heads, B, n)
    assert grid in wattn_grids(items, n)
    if geom in THREE_TRIPS:
        for g in wattn_grids(items, n):
            mix = walk_of(geom, B, g)[1]
            assert mix["interior_then_overhanging"] > 0, f"grid {g}: no workgroup follows an interior window with an overhanging one"
            if geom == "ws7_h3":
                assert mix["head_changes"] > 0, f"grid {g}: no workgroup changes head between two of its items"
    trips, mix = walk_of(geom, B, grid)
    if geom == "ws7_mixed":
        assert sorted(trips) == [1, 2], f"grid {grid}: has_next must be true in some workgroups and false in others, trips {trips}"
        assert mix["head_changes"] > 0, f"grid {grid}: no workgroup changes head in front of its second item"
    return B, items, grid, trips, mix


# depthwise 7 x 7 block kernel: 32 x 16 x 96 = 2 tiles x 3 channel chunks = 6 tiles per image
DW7 = dict(H=32, W=16, C=96, k=7, act="none")
DW7_TILES = (DW7["H"] // 16) * (DW7["W"] // 16) * (DW7["C"] // 32)


def dw7_batch(n):
    """The smallest even batch with 6 B >= 4n + 1 (tiles beyond twice the grid of 2n) whose tile count is not a multiple of 8 (mmsa_xcd_order then leaves a tail
    in dispatch order).  6 B = 12 (B / 2) is a multiple of 8 exactly when B / 2 is even -- at n = 256 that rules out B = 172 (1032 tiles), so B = 174."""
    B = cdiv(4 * n + 1, DW7_TILES)
    while B % 2 or (DW7_TILES * B) % 8 == 0:
        B += 1
    return B


def xcd_order(lin, total):
    """csrc/common.h mmsa_xcd_order: dispatch-order id -> work index."""
    per = total >> 3
    return (lin & 7) * per + (lin >> 3) if lin < (per << 3) else lin


def dw7_facts(n, ipg):
    """Asserts the tile walk the case claims at n CUs; -> (B, tiles, grid, trips -> workgroups, images per one-trip sub-batch)."""
    B = dw7_batch(n)
    nt, grid = DW7_TILES * B, 2 * n
    assert B % 2 == 0 and nt >= 4 * n + 1 and nt % 8 != 0
    trips = [len(range(g, nt, grid)) for g in range(grid)]
    assert max(trips) >= 3 and min(trips) < max(trips), "three trips and a ragged last round"
    sub = grid // DW7_TILES
    assert sub >= 1 and sub * DW7_TILES <= grid, "a sub-batch must be one tile per workgroup"
    walks = [[xcd_order(lin, nt) // DW7_TILES for lin in range(g, nt, grid)] for g in range(grid)]        # images of a workgroup's tiles
    assert sorted(xcd_order(lin, nt) for lin in range(nt)) == list(range(nt))
    assert any(a != b for w in walks for a, b in zip(w, w[1:])), "no workgroup changes image"
    if ipg:
        assert ipg == B // 2
        assert any(a // ipg != b // ipg for w in walks for a, b in zip(w, w[1:])), "no workgroup changes image group (weights and bias) between two of its tiles"
    return B, nt, grid, {t: trips.count(t) for t in sorted(set(trips))}, sub


def dw7_params(n, grouped):
    B = dw7_batch(n)
    return dict(DW7, B=B, bias=grouped, **({"ipg": B // 2} if grouped else {}))


# grid-stride kernels: op -> (case id, parameters, block cap, work units of the launch); a block is 256 units
# (gelu_gate reads [rows, 2 C]: an input of 68 MB, above the 50 MB the other cases keep to.  It cannot be smaller: passing the cap takes more than 8192 x 256 OUTPUT
#  float4s, 33.5 MB, and the input is twice the output.)
_EW = dict(B=2, H=128, W=128, HW=128 * 128, C=260)                    # 32768 rows x 65 float4: a row never ends on a block boundary
_GC = dict(B=2, G=52, cin_g=2, cout_g=5, H=128, W=128, k=1, act="none", bias=True)     # k = 1 WITH a bias: neither the MFMA nor the tiled kernel takes it
IM2COL = dict(B=2, Ctot=4, c0=1, Cin=3, H=728, W=728, p=4, Kpad=64)   # 2 x 182 x 182 patches; Kpad 64 > 3 * 4 * 4 = 48: sixteen zero columns per row
STRIDE = {
    "gelu_gate": ("walk-gg-128x128-c260", _EW, 8192, _EW["B"] * _EW["HW"] * (_EW["C"] // 4)),
    "ca_apply": ("walk-ca-128x128-c260", _EW, 8192, _EW["B"] * _EW["HW"] * (_EW["C"] // 4)),
    "lnhw": ("walk-lnhw-hw16384-c260", _EW, 8192, _EW["B"] * _EW["HW"] * (_EW["C"] // 4)),
    "gconv": ("walk-gc1-gen-bias-128x128-g52", _GC, 32768, _GC["B"] * _GC["H"] * _GC["W"] * _GC["G"] * _GC["cout_g"]),
    "im2col": ("walk-im2col-728-p4", IM2COL, 16384, IM2COL["B"] * (IM2COL["H"] // IM2COL["p"]) * (IM2COL["W"] // IM2COL["p"]) * IM2COL["Kpad"]),
}


def stride_facts(op, chunks):
    """More than cap x 256 units and less than twice that: the second trip exists and is partial; a chunk (1 / chunks of the launch) stays at one trip."""
    _, _, cap, units = STRIDE[op]
    assert cap * 256 < units < 2 * cap * 256, (op, units)
    assert units % chunks == 0 and units // chunks <= cap * 256, (op, units, chunks)
    return units - cap * 256


def bounded_cases(n):
    """(case id, op, parameters) of every case here that is held to a bound of tests/variant_ref.py."""
    return [(f"walk-dw7-blk-n{n}", "dwconv", dw7_params(n, False)), (f"walk-dw7-blk-ipg-n{n}", "dwconv", dw7_params(n, True))] + \
           [(STRIDE[op][0], op, STRIDE[op][1]) for op in ("gelu_gate", "ca_apply", "lnhw", "gconv")]


# ------------------------------------------------------------------------------------------------ fixtures
@pytest.fixture(scope="module")
def ops():
    import mmsa
    return mmsa.ops


@pytest.fixture(scope="module")
def cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


def assert_same_bits(a, b, what):
    same = bits(a) == bits(b)
    if not bool(same.all()):
        bad = ~same
        raise AssertionError(f"{what}: {int(bad.sum())} elements in {int(bad.any(1).sum())} rows differ, first at {bad.nonzero()[0].tolist()}")


class NanOut:
    """mmsa.ops with alloc_planes NaN-filled: every 16-bit word 0x7FFF -- a NaN as bf16 and as fp16, and both of its bytes NaNs as e5m2 -- so that a row the
    launch does not write decodes to NaN in every output format (run_fused allocates its output through ops.alloc_planes)."""

    def __init__(self, ops):
        self._ops = ops

    def __getattr__(self, name):
        return getattr(self._ops, name)

    def alloc_planes(self, *a, **kw):
        pl = self._ops.alloc_planes(*a, **kw)
        pl.p.fill_(0x7FFF)
        return pl


@pytest.fixture(scope="module")
def window_refs():
    """(geometry, vf) -> {image: (float64 reference on the CPU, max |logit|)}: computed by the first test of a (geometry, vf), shared by its output formats (the
    operands do not depend on the output format), never written to again, dropped with the module.  About 80 MB of host memory in all at 256 CUs."""
    refs = {}
    yield refs
    refs.clear()
    torch.cuda.empty_cache()


# ------------------------------------------------------------------------------------------------ 1. windowed attention
def window_walk(ops, refs, n, geom, vf, fmt):
    H, W, ws, heads, seed = WATTN[geom]
    B, items, grid, trips, mix = walk_facts(geom, n)
    T, scale, nops = H * W, HD ** -0.5, NanOut(ops)
    what = f"window walk {geom} heads={heads} n={n} B={B} items={items} vf={vf} out={FMT_NAME[fmt]}"
    print(f"{what}: grid {grid} by the restated cost model, trips -> workgroups {trips}, between consecutive items of a workgroup {mix}")
    qkv, bias, rph, rpw = make_problem(B, H, W, heads, HD, ws, seed)
    gw = torch.zeros(1, device=DEV)
    out, _, _, ao = run_fused(nops, "window", qkv, bias, rph, rpw, B, H, W, heads, HD, ws, scale, vf, fmt, guard=gw)
    assert out.shape == (B * T, heads * HD) and not bool(torch.isnan(out).any()), f"{what}: rows left unwritten (NaN)"
    # b. the guard changes no output bit
    ao2 = run_fused(nops, "window", qkv, bias, rph, rpw, B, H, W, heads, HD, ws, scale, vf, fmt)[3]
    assert torch.equal(ao.p, ao2.p), f"{what}: the output planes differ with and without the guard word"
    del ao, ao2
    mine = refs.setdefault((geom, vf), {})
    gmax, amax_all, worst = 0.0, 0.0, 0.0
    for b in range(B):
        gb = torch.zeros(1, device=DEV)
        one, (q64, b64), tabs, _ = run_fused(nops, "window", qkv[b * T:(b + 1) * T], bias, rph, rpw, 1, H, W, heads, HD, ws, scale, vf, fmt, guard=gb)
        # a. bit identity: image b of the batched launch against image b alone (one item per workgroup)
        assert_same_bits(out[b * T:(b + 1) * T], one, f"{what}: image {b} against its one-image launch")
        # c. float64 on the operands the kernel read, image by image, under the existing bounds
        if b not in mine:
            r, amax = ref_attention(q64, b64, *tabs, 1, H, W, heads, HD, ws, scale)
            mine[b] = (r.cpu(), amax)
        r, amax = mine[b]
        worst = max(worst, check_leaf(("window", vf, fmt), one, r, amax, f"{what} image {b}"))
        check_guard(gb, amax, vf, f"{what} image {b}")
        gmax, amax_all = max(gmax, gb.item()), max(amax_all, amax)
    # b. the batched guard word is the maximum of the per-image words, exactly, and agrees with float64
    assert gw.item() == gmax, f"{what}: guard {gw.item()!r} vs the largest one-image guard {gmax!r}"
    check_guard(gw, amax_all, vf, what)
    print(f"{what}: worst max_rel over {B} images {worst:.3e}, guard {gw.item():.4f} (float64 {amax_all:.4f})")


@pytest.mark.parametrize("fmt", [B3, H8C], ids=FMT_NAME.get)
@pytest.mark.parametrize("vf", [0, 2])
@pytest.mark.parametrize("geom", THREE_TRIPS)
def test_window_attention_third_trip(ops, window_refs, cus, geom, vf, fmt):
    """items >= 2n + 1: three trips under either grid, interior windows followed by overhanging ones; ws7_h3: the head changes between a workgroup's items, so
    `head` (the next item's, decoded behind barrier #2) and `head_cur` (the current store's) differ on every trip."""
    window_walk(ops, window_refs, cus, geom, vf, fmt)


@pytest.mark.parametrize("vf", [0, 2])
def test_window_attention_one_and_two_trips(ops, window_refs, cus, vf):
    """n < items < 2n, three heads: has_next is true in some workgroups and false in others at the same barrier, and those that go on change head."""
    window_walk(ops, window_refs, cus, "ws7_mixed", vf, H8C)


# ------------------------------------------------------------------------------------------------ 2. depthwise 7 x 7 block kernel
@pytest.mark.parametrize("grouped", [False, True], ids=["one-weight-set", "two-groups-bias"])
def test_dwconv7_block_walk(ops, cus, grouped):
    p = dw7_params(cus, grouped)
    Bn, nt, grid, trips, sub = dw7_facts(cus, p.get("ipg", 0))
    cid = f"walk-dw7-blk{'-ipg' if grouped else ''}-n{cus}"
    print(f"{cid}: B={Bn} tiles={nt} grid={grid} trips -> workgroups {trips}, one-trip sub-batches of {sub} images")
    i = V.make_dwconv(p, V.gen_for(cid))
    r, bnd = V.ref_dwconv(V.cast(i, torch.float64), p)
    y = run_dwconv(ops, i, p)["y"]                                    # NaN-filled output, one launch
    torch.cuda.synchronize()
    print(f"{cid}: worst |y - r| / bound = {V.assert_inside(y, r, bnd.double(), cid):.3f}")
    # the same images in launches of one tile per workgroup, each group with its own weights
    H, W, C, hw = p["H"], p["W"], p["C"], p["H"] * p["W"]
    x = dev(V.nhwc(i["x"]))
    w = dev(i["w"].reshape(-1, C, 49).transpose(1, 2))                 # [groups][tap][C]
    y1 = nanbuf(Bn * hw, C)
    per_group = p.get("ipg") or Bn
    for lo in range(0, Bn, per_group):
        gi = lo // per_group
        for s in range(lo, lo + per_group, sub):
            nb = min(sub, lo + per_group - s)
            assert nb * DW7_TILES <= grid
            ops.dwconv(x[s * hw:(s + 1) * hw], w[gi], dev(i["b"][gi]) if "b" in i else None, y1[s * hw:(s + 1) * hw], nb, H, W, 7)
    torch.cuda.synchronize()
    assert_same_bits(y, y1, f"{cid} against the one-tile-per-workgroup launches")


# ------------------------------------------------------------------------------------------------ 3. grid-stride kernels past their block cap
def _chunk_gelu_gate(ops, i, p, y, n):
    x, rows = dev(i["x"]), i["x"].shape[0] // n
    for k in range(n):
        ops.gelu_gate(x[k * rows:(k + 1) * rows], y[k * rows:(k + 1) * rows], p["C"])


def _chunk_ca_apply(ops, i, p, y, n, pl=None):
    z, att, hw, hpw = dev(i["z"]), dev(i["att"]), p["H"] * p["W"], p["H"] + p["W"]
    for b in range(n):
        ops.ca_apply(z[b * hw:(b + 1) * hw], att[b * hpw:(b + 1) * hpw], y[b * hw:(b + 1) * hw], 1, p["H"], p["W"], out_planes=pl.rows(b * hw, (b + 1) * hw))


def _chunk_lnhw(ops, i, p, y, n):
    x, hw = dev(i["x"]), p["HW"]
    m, rs, mu, w, b_ = (dev(i[k]) for k in ("mean", "rstd", "mult", "w", "b"))
    for b in range(n):
        ops.lnhw_apply(x[b * hw:(b + 1) * hw], m[b:b + 1], rs[b:b + 1], mu[b:b + 1], w, b_, y[b * hw:(b + 1) * hw], 1, hw)


def _chunk_gconv(ops, i, p, y, n):
    G, ci, co, hw = p["G"], p["cin_g"], p["cout_g"], p["H"] * p["W"]
    x, w, b_ = dev(V.nhwc(i["x"])), dev(i["w"].reshape(G, co, ci, 1).permute(0, 3, 2, 1)), dev(i["b"])
    for b in range(n):
        ops.gconv(x[b * hw:(b + 1) * hw], w, b_, y[b * hw:(b + 1) * hw], 1, p["H"], p["W"], G, ci, co, 1)


@pytest.mark.parametrize("op", ["gelu_gate", "ca_apply", "lnhw", "gconv"])
def test_grid_stride_second_trip(ops, op):
    """One launch past the block cap against float64 (variant_ref's bound) and, bit for bit, against the same rows done in launches below the cap."""
    cid, p, cap, units = STRIDE[op]
    chunks = 4 if op == "gelu_gate" else p["B"]
    print(f"{cid}: {units} units, {cap} blocks: {stride_facts(op, chunks)} units on a second trip")
    make, ref = V.OPS[op]
    i = make(p, V.gen_for(cid))
    r, bnd = ref(V.cast(i, torch.float64), p)
    first = {"gelu_gate": run_gelu_gate, "ca_apply": run_ca_apply, "lnhw": run_lnhw, "gconv": run_gconv}[op](ops, i, p)      # NaN-filled output
    torch.cuda.synchronize()
    y = first["y"]
    print(f"{cid}: worst |y - r| / bound = {V.assert_inside(y, r, bnd.double(), cid):.3f}")
    del r, bnd
    y1 = nanbuf(*y.shape)
    if op == "ca_apply":                                               # fp32 and bf16 hi/lo planes from the same launch
        pl = first["planes"][0]
        planes_equal_split(ops, pl, y, ops.FMT_B3)
        pl1 = ops.alloc_planes(y.shape[0], p["C"], DEV, zero=True)
        _chunk_ca_apply(ops, i, p, y1, chunks, pl1)
        torch.cuda.synchronize()
        assert torch.equal(pl.p, pl1.p), f"{cid}: the planes differ from those of the per-image launches"
    else:
        {"gelu_gate": _chunk_gelu_gate, "lnhw": _chunk_lnhw, "gconv": _chunk_gconv}[op](ops, i, p, y1, chunks)
        torch.cuda.synchronize()
    assert_same_bits(y, y1, f"{cid} against the launches below the cap")


def im2col_ref(x, p):
    """out[(b, ph, pw)][(c, kh, kw)] = x[b, c0 + c, ph p + kh, pw p + kw], columns from Cin p^2 on zero: a copy, so the reference is exact."""
    Bn, Cin, ps, Hp, Wp = p["B"], p["Cin"], p["p"], p["H"] // p["p"], p["W"] // p["p"]
    v = x[:, p["c0"]:p["c0"] + Cin].reshape(Bn, Cin, Hp, ps, Wp, ps).permute(0, 2, 4, 1, 3, 5).reshape(Bn * Hp * Wp, Cin * ps * ps)
    return torch.cat([v, v.new_zeros(v.shape[0], p["Kpad"] - v.shape[1])], 1)


def test_im2col_second_trip(ops):
    cid, p, cap, units = STRIDE["im2col"]
    print(f"{cid}: {units} elements, {cap} blocks: {stride_facts('im2col', p['B'])} elements on a second trip")
    assert p["Kpad"] > p["Cin"] * p["p"] ** 2
    x = torch.randn(p["B"], p["Ctot"], p["H"], p["W"], generator=V.gen_for(cid))
    want = im2col_ref(x, p)
    xd, rows = dev(x), want.shape[0] // p["B"]
    out = nanbuf(*want.shape)
    ops.im2col_nchw(xd, p["c0"], p["Cin"], p["p"], out)
    torch.cuda.synchronize()
    assert torch.equal(bits(out.cpu()), bits(want)), f"{cid}: not the exact copy with exact zeros"
    out1 = nanbuf(*want.shape)
    for b in range(p["B"]):
        ops.im2col_nchw(xd[b:b + 1], p["c0"], p["Cin"], p["p"], out1[b * rows:(b + 1) * rows])
    torch.cuda.synchronize()
    assert torch.equal(bits(out), bits(out1)), f"{cid}: differs from the per-image launches"
