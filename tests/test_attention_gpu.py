"""Operator-level parity of every attention kernel variant against float64 on the operands the kernel actually read.

csrc/attention.hip instantiates attn_kernel<HD, PL, FB, REL, VF> per head width (32 / 64 / 96), input kind (fp32 rows or planes), key
blocking (FB: a global W = 64, H % 4 == 0 grid), fused rel-pos and v format, and stores its output in one of four plane formats (B3 / F3 /
H8 / H8C); csrc/wattn.hip and the fused global entry add their own v-format x output-format choices.  The tests here compare the attention
output `ao` itself -- before any projection, which mixes channels and dilutes a per-head or per-channel error -- with `ref_attention`, a
plain float64 restatement of IE:465-551 (window partition with the pad keys reading the qkv bias row, scale q k^T + the decomposed rel-pos
terms of the oracle's add_decomposed_rel_pos, softmax, @ v, unpartition) evaluated on planes_to_float of the kernel's input planes (or on
their fp16 hi parts where the kernel reads only those).

Tolerances (max |err| / max |ref| of `ao`, TOL below) were measured on the hd-64 leaves of each (entry, v format, output format) and are
2x that, so that a new head width or format must match its hd-64 sibling; the ceilings are 1e-4 for the hi/lo pair modes and 1e-3 for the
fp16 modes.  Every problem asserts that its max |logit| is at least 4: a near-uniform softmax would not see a scale or rel-pos error."""
import os

import numpy as np
import pytest
import torch

from oracle import ref_encoder as R
from tests.configs import CONFIGS, make_input, probe_index
from tests.weights import peaky_attention, seeded_state_dict
from tests.util import assert_close, max_rel

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

B3, H8, H8C, F3 = 0, 1, 2, 3          # ops.FMT_* (include/mmsa.h)
FMT_NAME = {B3: "b3", H8: "h8", H8C: "h8c", F3: "f3"}
ALL_FMTS = (B3, F3, H8, H8C)

# geometry: (name, B, H, W, window size); FB = global, W == 64, H % 4 == 0
GEOMS = {
    "win14_pad": (2, 20, 20, 14),     # windowed, 20 -> 28: pad keys in three of the four windows
    "win7_odd": (2, 9, 33, 7),        # windowed, odd grid: 9 -> 14, 33 -> 35
    "glob_fb64": (2, 64, 64, 0),      # global, FB (one key block = one image row)
    "glob_fb32": (2, 32, 64, 0),      # global, FB with H = 32
    "glob_nofb": (2, 20, 12, 0),      # global without FB
}

QK_STD = 1.1       # logits ~ N(0, QK_STD^4) before the rel-pos terms: max |logit| 6..9 on these grids
REL_STD = 0.5      # rel-pos terms ~ N(0, (QK_STD * REL_STD)^2) each (tables scaled by hd^-0.5)

# max_rel of `ao` against float64 on the kernel's operands, measured on the hd-64 leaves of each key (entry, v format, output format; the
# largest over the key's geometries, MI355X) -> TOL = 2x that: every leaf of the key (hd 32 / 96, padded widths) must stay within it
MEASURED_HD64 = {
    ("rows", 0, None): 1.9e-6,
    ("planes", 0, B3): 6.1e-6, ("planes", 0, F3): 1.7e-6, ("planes", 0, H8): 2.1e-5, ("planes", 0, H8C): 1.9e-5,
    ("planes", 1, B3): 9.6e-5, ("planes", 1, F3): 9.6e-5, ("planes", 1, H8): 9.6e-5, ("planes", 1, H8C): 9.4e-5,
    ("window", 0, B3): 4.6e-6, ("window", 0, F3): 6.2e-7, ("window", 0, H8): 2.3e-5, ("window", 0, H8C): 2.4e-5,
    ("window", 2, B3): 1.1e-4, ("window", 2, F3): 1.1e-4, ("window", 2, H8): 1.1e-4, ("window", 2, H8C): 1.1e-4,
    ("global", 0, B3): 4.6e-6, ("global", 0, F3): 1.2e-6, ("global", 0, H8): 2.0e-5, ("global", 0, H8C): 2.3e-5,
    ("global", 2, B3): 8.7e-5, ("global", 2, F3): 8.4e-5, ("global", 2, H8): 9.2e-5, ("global", 2, H8C): 8.7e-5,
}
TOL = {k: 2.0 * v for k, v in MEASURED_HD64.items()}
CEIL = {0: 1e-4, 1: 1e-3, 2: 1e-3}   # pair modes / fp16 P V / all-fp16


@pytest.fixture(scope="module")
def ops():
    import mmsa
    return mmsa.ops


def g(seed):
    return torch.Generator().manual_seed(seed)


def planes_to_float(p):
    import mmsa
    return mmsa.ops.planes_to_float(p)


def hi_part(pl, cols=None):
    """fp16 hi values of h8 planes (activation layout) as fp32 [rows, cols]: all the fp16 kernels read of them."""
    r, w = pl.p.shape
    blk = pl.p.contiguous().view(torch.uint8).view(r, w // 64, 128)
    return blk[:, :, :64].contiguous().view(torch.float16).float().reshape(r, w // 2)[:, :(pl.k if cols is None else cols)]


def kernel_operands(pl, vf, D):
    """The [rows, 3D] q | k | v values a kernel of v format `vf` reads from qkv (or bias) planes, float64: f3 pairs (vf 0); f3 q, k and the
    fp16 hi parts of the h8 v columns (vf 1); fp16 hi parts throughout (vf 2)."""
    import mmsa
    if vf == 2:
        x = hi_part(pl)
    elif vf == 1:
        vp = mmsa.ops.Planes(pl.p[:, 2 * pl.split:], pl.n, D, pl.kpad - pl.split, H8)
        x = torch.cat([planes_to_float(pl)[:, :2 * D], hi_part(vp, D)], 1)
    else:
        x = planes_to_float(pl)
    return x[:, :3 * D].double()


def ref_attention(qkv, bias, rph, rpw, B, H, W, heads, hd, ws, scale):
    """float64 attention of IE:465-551 on the operands given: qkv [B*H*W, 3D] (q | k | v, channel = head*hd + c), bias [3D] (pad tokens
    of a window: q, k, v = the qkv bias row, IE:401-407), rel-pos tables [2K-1, hd] (K = ws, or H / W).  -> (out [B*H*W, D], max |logit| over
    live queries and every key)."""
    D = heads * hd
    qkv = qkv.to(DEV, torch.float64)
    bias = bias.to(DEV, torch.float64).reshape(3 * D)
    rph, rpw = rph.to(DEV, torch.float64), rpw.to(DEV, torch.float64)
    x = qkv.view(B, H, W, 3 * D)
    if ws:
        Hp, Wp = -(-H // ws) * ws, -(-W // ws) * ws
        full = bias.view(1, 1, 1, 3 * D).expand(B, Hp, Wp, 3 * D).clone()
        full[:, :H, :W] = x
        live = torch.zeros(B, Hp, Wp, 1, dtype=torch.float64, device=DEV)
        live[:, :H, :W] = 1.0
        x, live = R.window_partition(full, ws)[0], R.window_partition(live, ws)[0]
        gh = gw = ws
    else:
        live = torch.ones(B, H, W, 1, dtype=torch.float64, device=DEV)
        gh, gw = H, W
    N, n = x.shape[0], gh * gw
    q, k, v = (x[..., i * D:(i + 1) * D].reshape(N, n, heads, hd).permute(0, 2, 1, 3).reshape(N * heads, n, hd) for i in range(3))
    lv = live.reshape(N, 1, n, 1).expand(N, heads, n, 1).reshape(N * heads, n, 1)
    out = torch.empty(N * heads, n, hd, dtype=torch.float64, device=DEV)
    amax = 0.0
    for i in range(0, N * heads, 4):   # chunks: a 64 x 64 global group is a [4096, 4096] logit matrix per head
        s = slice(i, i + 4)
        lg = (q[s] * scale) @ k[s].transpose(-2, -1)
        lg = R.add_decomposed_rel_pos(lg, q[s], rph, rpw, (gh, gw), (gh, gw))
        amax = max(amax, (lg.abs() * lv[s]).max().item())
        out[s] = lg.softmax(-1) @ v[s]
    out = out.view(N, heads, gh, gw, hd).permute(0, 2, 3, 1, 4).reshape(N, gh, gw, D)
    if ws:
        out = R.window_unpartition(out, ws, (Hp, Wp), (H, W))
    return out.reshape(B * H * W, D), amax


def make_problem(B, H, W, heads, hd, ws, seed):
    """Seeded fp32 operands: qkv [B*H*W, 3D], bias [3D], rel-pos tables [2K-1, hd]."""
    D, gen = heads * hd, g(seed)
    qkv = torch.randn(B * H * W, 3 * D, generator=gen)
    qkv[:, :2 * D] *= QK_STD
    bias = torch.randn(3 * D, generator=gen) * 0.5
    kh, kw = (ws, ws) if ws else (H, W)
    rph = torch.randn(2 * kh - 1, hd, generator=gen) * (REL_STD * hd ** -0.5)
    rpw = torch.randn(2 * kw - 1, hd, generator=gen) * (REL_STD * hd ** -0.5)
    return qkv, bias, rph, rpw


def qkv_planes(ops, qkv, bias, D, vf):
    """(qkv planes, bias planes) in the form of v format `vf`: f3 (0), f3 with the v columns as h8 planes (1), h8 throughout (2)."""
    row = bias.reshape(1, -1).contiguous().to(DEV)
    if vf == 1:
        return ops.split_planes_qkv(qkv.to(DEV), D), ops.split_planes_qkv(row, D)
    f = H8 if vf == 2 else F3
    return ops.split_planes(qkv.to(DEV), fmt=f), ops.split_planes(row, kpad=3 * D, fmt=f)


def rel_tables(H, W, ws, rph, rpw):
    import mmsa.backbone as bb
    kh, kw = (ws, ws) if ws else (H, W)
    return bb._rel_table(kh, rph.to(DEV)), bb._rel_table(kw, rpw.to(DEV))


def run_prepass(ops, qkv, bias, rph, rpw, B, H, W, heads, hd, ws, scale, vf=None, out_fmt=B3, guard=None):
    """mmsa_relpos_bias(_planes) + mmsa_attention(_planes).  vf None: fp32 rows in and out.  -> (ao as fp32 rows, kernel operands, rp)"""
    D, T = heads * hd, H * W
    rh, rw = rel_tables(H, W, ws, rph, rpw)
    rp = torch.empty(B * heads * T, (2 * ws) if ws else (H + W), device=DEV)
    if vf is None:
        q = qkv.to(DEV)
        ops.relpos_bias(q, rh, rw, rp, B, H, W, heads, hd, ws)
        out = torch.empty(B * T, D, device=DEV)
        ops.attention(q, bias.to(DEV), rp, out, B, H, W, heads, hd, ws, scale)
        return out.cpu(), (qkv.double(), bias.double()), rp
    qp, bp = qkv_planes(ops, qkv, bias, D, vf)
    ops.relpos_bias(qp, rh, rw, rp, B, H, W, heads, hd, ws)
    ao = ops.alloc_planes(B * T, D, DEV, fmt=out_fmt)
    ops.attention(qp, bp, rp, ao, B, H, W, heads, hd, ws, scale, max_logit=guard)
    return planes_to_float(ao).cpu(), (kernel_operands(qp, vf, D), kernel_operands(bp, vf, D)[0]), rp, ao


def run_fused(ops, entry, qkv, bias, rph, rpw, B, H, W, heads, hd, ws, scale, vf, out_fmt, guard=None):
    """mmsa_window_attention_planes / mmsa_global_attention_planes (rel-pos terms fused; hd 64).  -> (ao fp32 rows, operands, tables, ao)"""
    D, T = heads * hd, H * W
    qp, bp = qkv_planes(ops, qkv, bias, D, vf)
    f = H8 if vf == 2 else F3
    ao = ops.alloc_planes(B * T, D, DEV, fmt=out_fmt)
    if entry == "window":
        relp = ops.window_relpos_planes(rph.to(DEV), rpw.to(DEV), ws, fmt=f)
        lo_w = 32
        ops.window_attention(qp, bp, relp, ao, B, H, W, heads, hd, ws, scale, max_logit=guard)
    else:
        relp = ops.global_relpos_planes(rph.to(DEV), rpw.to(DEV), fmt=f)
        lo_w = 128
        ops.global_attention(qp, bp, relp, ao, B, H, W, heads, hd, scale, max_logit=guard)
    tab = (hi_part(relp) if vf == 2 else planes_to_float(relp)).double()
    tabs = (tab[:rph.shape[0]], tab[lo_w:lo_w + rpw.shape[0]])
    return planes_to_float(ao).cpu(), (kernel_operands(qp, vf, D), kernel_operands(bp, vf, D)[0]), tabs, ao


def check_leaf(key, got, ref, amax, what):
    tol = TOL[key]
    assert tol <= CEIL[key[1]], (key, tol)
    assert amax >= 4.0, f"{what}: max |logit| {amax:.2f} < 4 -- a near-uniform softmax cannot see a scale or rel-pos error"
    assert torch.isfinite(got).all(), f"{what}: non-finite values"
    m = max_rel(got, ref)
    print(f"LEAF {what} key={key} max_rel={m:.3e} amax={amax:.2f}")
    assert m <= tol, f"{what}: max_rel {m:.3e} > {tol:.1e}"
    return m


def check_guard(gw, want, vf, what):
    tol = 2e-3 if vf == 2 else 2e-5
    assert abs(gw.item() - want) <= tol * max(want, 1.0), f"{what}: guard {gw.item():.6f} vs float64 {want:.6f}"


# ------------------------------------------------------------------------------------------------------------------ the leaf matrix
@pytest.mark.parametrize("geom", list(GEOMS))
@pytest.mark.parametrize("hd", [32, 64, 96])
def test_attention_rows_vs_float64(ops, hd, geom):
    """mmsa_attention (fp32 rows in and out; rel-pos prepass mmsa_relpos_bias) against float64 on the fp32 operands.
    Measured max_rel: hd 64 2.9e-7 .. 1.9e-6, hd 32 2.9e-7 .. 1.7e-6, hd 96 3.9e-7 .. 1.1e-6 (bound 3.8e-6)."""
    B, H, W, ws = GEOMS[geom]
    heads = 3
    qkv, bias, rph, rpw = make_problem(B, H, W, heads, hd, ws, seed=hd + 7)
    out, (q64, b64), _ = run_prepass(ops, qkv, bias, rph, rpw, B, H, W, heads, hd, ws, hd ** -0.5)
    ref, amax = ref_attention(q64, b64, rph.double(), rpw.double(), B, H, W, heads, hd, ws, hd ** -0.5)
    check_leaf(("rows", 0, None), out, ref.cpu(), amax, f"rows hd={hd} {geom}")


@pytest.mark.parametrize("out_fmt", ALL_FMTS, ids=FMT_NAME.get)
@pytest.mark.parametrize("vf", [0, 1])
@pytest.mark.parametrize("geom", list(GEOMS))
@pytest.mark.parametrize("hd", [32, 64, 96])
def test_attention_planes_vs_float64(ops, hd, geom, vf, out_fmt):
    """mmsa_attention_planes (rel-pos prepass on the planes' q): f3 qkv planes (vf 0) or f3 q, k + h8 v (vf 1, fp16 P V), every output
    format, against float64 on the operands the kernel read; the guard word within 2e-5 of the float64 max |logit| over live queries.
    Measured max_rel (hd 64 / hd 32 / hd 96, worst geometry): vf 0 b3 6.1e-6 / 5.3e-6 / 5.8e-6, f3 1.7e-6 / 1.0e-6 / 2.4e-6, h8 2.1e-5 /
    2.4e-5 / 2.3e-5, h8c 1.9e-5 / 3.3e-5 / 1.9e-5; vf 1 (fp16 P) 9.6e-5 / 1.0e-4 / 1.2e-4 in every format."""
    B, H, W, ws = GEOMS[geom]
    heads = 3
    qkv, bias, rph, rpw = make_problem(B, H, W, heads, hd, ws, seed=hd + 11)
    gw = torch.zeros(1, device=DEV)
    out, (q64, b64), _, _ = run_prepass(ops, qkv, bias, rph, rpw, B, H, W, heads, hd, ws, hd ** -0.5, vf=vf, out_fmt=out_fmt, guard=gw)
    ref, amax = ref_attention(q64, b64, rph.double(), rpw.double(), B, H, W, heads, hd, ws, hd ** -0.5)
    what = f"planes hd={hd} {geom} vf={vf} out={FMT_NAME[out_fmt]}"
    check_leaf(("planes", vf, out_fmt), out, ref.cpu(), amax, what)
    check_guard(gw, amax, vf, what)


@pytest.mark.parametrize("out_fmt", ALL_FMTS, ids=FMT_NAME.get)
@pytest.mark.parametrize("vf", [0, 2])
@pytest.mark.parametrize("geom", ["win14_pad", "win7_odd_b1"])
def test_window_attention_planes_vs_float64(ops, geom, vf, out_fmt):
    """mmsa_window_attention_planes (K/V-resident, rel-pos fused, hd 64): f3 (vf 0) or h8 planes throughout (vf 2), every output format.
    win7_odd_b1 = ONE 9 x 33 image: 297 rows, so the last h8c row pair is half empty and row pairs straddle image rows and windows.
    Measured max_rel (worst geometry): vf 0 b3 4.6e-6, f3 6.2e-7, h8 2.3e-5, h8c 2.4e-5; vf 2 1.1e-4 in every format."""
    B, H, W, ws = (1, 9, 33, 7) if geom == "win7_odd_b1" else GEOMS[geom]
    heads, hd = 3, 64
    qkv, bias, rph, rpw = make_problem(B, H, W, heads, hd, ws, seed=31)
    gw = torch.zeros(1, device=DEV)
    out, (q64, b64), tabs, _ = run_fused(ops, "window", qkv, bias, rph, rpw, B, H, W, heads, hd, ws, hd ** -0.5, vf, out_fmt, guard=gw)
    ref, amax = ref_attention(q64, b64, *tabs, B, H, W, heads, hd, ws, hd ** -0.5)
    what = f"window {geom} vf={vf} out={FMT_NAME[out_fmt]}"
    check_leaf(("window", vf, out_fmt), out, ref.cpu(), amax, what)
    check_guard(gw, amax, vf, what)


@pytest.mark.parametrize("out_fmt", ALL_FMTS, ids=FMT_NAME.get)
@pytest.mark.parametrize("vf", [0, 2])
@pytest.mark.parametrize("H", [64, 32, 4])
def test_global_attention_planes_vs_float64(ops, H, vf, out_fmt):
    """mmsa_global_attention_planes (rel-pos terms computed in the prologue, W = 64, hd 64): vf 0 / 2, every output format.
    Measured max_rel (worst H): vf 0 b3 4.6e-6, f3 1.2e-6, h8 2.0e-5, h8c 2.3e-5; vf 2 8.4e-5 .. 9.2e-5."""
    B, W, heads, hd = 2, 64, 3, 64
    qkv, bias, rph, rpw = make_problem(B, H, W, heads, hd, 0, seed=41 + H)
    gw = torch.zeros(1, device=DEV)
    out, (q64, b64), tabs, _ = run_fused(ops, "global", qkv, bias, rph, rpw, B, H, W, heads, hd, 0, hd ** -0.5, vf, out_fmt, guard=gw)
    ref, amax = ref_attention(q64, b64, *tabs, B, H, W, heads, hd, 0, hd ** -0.5)
    what = f"global H={H} vf={vf} out={FMT_NAME[out_fmt]}"
    check_leaf(("global", vf, out_fmt), out, ref.cpu(), amax, what)
    check_guard(gw, amax, vf, what)


@pytest.mark.parametrize("planes", [False, True])
@pytest.mark.parametrize("geom", ["win14_pad", "win7_odd", "glob_nofb", "glob_fb32"])
@pytest.mark.parametrize("hd", [64, 96])
def test_relpos_terms_vs_float64(ops, hd, geom, planes):
    """mmsa_relpos_bias / mmsa_relpos_bias_planes: rel_h[tok, kh] = q . Rh[qh, kh] and rel_w[tok, kw] = q . Rw[qw, kw] (IE:609-617; (qh, qw) =
    token coordinates in its window or image) against float64 on the q the kernel read, with Rh != Rw so that a swapped table shows.
    Measured max_rel: hd 64 1.2e-7 .. 2.0e-7, hd 96 1.3e-7 .. 2.4e-7 (bound 4e-7, 2x hd 64)."""
    B, H, W, ws = GEOMS[geom]
    heads = 3
    D, T = heads * hd, H * W
    qkv, _, rph, rpw = make_problem(B, H, W, heads, hd, ws, seed=hd + 51)
    rh, rw = rel_tables(H, W, ws, rph, rpw)
    kh, kw = (ws, ws) if ws else (H, W)
    rp = torch.empty(B * heads * T, kh + kw, device=DEV)
    if planes:
        qp = ops.split_planes(qkv.to(DEV), fmt=F3)
        ops.relpos_bias(qp, rh, rw, rp, B, H, W, heads, hd, ws)
        q = planes_to_float(qp)[:, :D].double().cpu()
    else:
        ops.relpos_bias(qkv.to(DEV), rh, rw, rp, B, H, W, heads, hd, ws)
        q = qkv[:, :D].double()
    Rh, Rw = R.get_rel_pos(kh, kh, rph.double()), R.get_rel_pos(kw, kw, rpw.double())     # [K, K, hd]
    qi = torch.arange(H) % ws if ws else torch.arange(H)
    wi = torch.arange(W) % ws if ws else torch.arange(W)
    qv = q.view(B, H, W, heads, hd).permute(0, 3, 1, 2, 4)
    rel_h = torch.einsum("bnhwc,hkc->bnhwk", qv, Rh[qi])
    rel_w = torch.einsum("bnhwc,wkc->bnhwk", qv, Rw[wi])
    got = rp.cpu().view(B, heads, H, W, kh + kw)
    mh, mw = max_rel(got[..., :kh], rel_h), max_rel(got[..., kh:], rel_w)
    print(f"RELPOS hd={hd} {geom} planes={planes} rel_h={mh:.3e} rel_w={mw:.3e}")
    assert mh <= 4e-7 and mw <= 4e-7, f"relpos hd={hd} {geom} planes={planes}: rel_h {mh:.3e} rel_w {mw:.3e}"


# ------------------------------------------------------------------------------------------------- output formats agree with each other
def ulp_step(x, fmt):
    """An upper bound of the spacing of a format's decoded values around x: one unit of the lo part's last place (hi/lo formats: |lo| <= half an
    ulp of hi).  B3 bf16 hi/lo: 2^(e-14); F3 fp16 hi/lo: 2^(e-21), at least fp16's 2^-24; H8 / H8C: e5m2 lo (3 significant bits) 2^(e-13)."""
    e = torch.frexp(x.abs().double())[1].double() - 1
    if fmt == B3:
        return torch.exp2(e - 14)
    if fmt == F3:
        return torch.clamp(torch.exp2(e - 21), min=2.0 ** -24)
    return torch.clamp(torch.exp2(e - 13), min=2.0 ** -27)


def check_formats_agree(ops, aos, what):
    """aos: output planes of ONE launch configuration per output format.  The B3 result holds the kernel's fp32 output to one unit of B3's
    last place; each format X, re-split from it on the host, must agree with the kernel's X planes to one unit of X's last place plus that:
    only a rounding boundary crossed by B3's own error can move a value, any other difference is the X store path."""
    b3 = planes_to_float(aos[B3])
    for fmt in (F3, H8, H8C):
        resplit = planes_to_float(ops.split_planes(b3.contiguous(), fmt=fmt)).double()
        got = planes_to_float(aos[fmt]).double()
        assert got.shape == resplit.shape
        mag = torch.maximum(got.abs(), resplit.abs())
        bound = ulp_step(mag, fmt) + ulp_step(mag, B3)
        bad = (got - resplit).abs() > bound
        assert not bad.any(), (f"{what}: {FMT_NAME[fmt]} output differs from the re-split B3 output in {int(bad.sum())} elements, first at "
                               f"{bad.nonzero()[0].tolist()}: {got[bad][0].item()!r} vs {resplit[bad][0].item()!r}")


@pytest.mark.parametrize("case", ["prepass_hd96_win7_b1", "prepass_hd96_fb32_vf1", "prepass_hd32_nofb", "window_vf0_b1", "window_vf2_b1",
                                  "global_vf0", "global_vf2"])
def test_output_formats_agree(ops, case):
    """One launch configuration per entry, run once per output format: B3 / F3 / H8 / H8C planes of the same fp32 values (the format is a
    store-path choice only).  Odd row counts (297 rows: a half-empty last h8c row pair) and D = 96 / 288 (h8c width padded to 128 / 320)."""
    aos = {}
    for fmt in ALL_FMTS:
        if case.startswith("prepass"):
            hd = 96 if "hd96" in case else 32
            B, H, W, ws = {"win7_b1": (1, 9, 33, 7), "fb32_vf1": (2, 32, 64, 0), "nofb": (2, 20, 12, 0)}[case.split("_", 2)[2]]
            vf = 1 if case.endswith("vf1") else 0
            prob = make_problem(B, H, W, 3, hd, ws, seed=61)
            aos[fmt] = run_prepass(ops, *prob, B, H, W, 3, hd, ws, hd ** -0.5, vf=vf, out_fmt=fmt)[3]
        elif case.startswith("window"):
            B, H, W, ws = 1, 9, 33, 7
            prob = make_problem(B, H, W, 3, 64, ws, seed=62)
            aos[fmt] = run_fused(ops, "window", *prob, B, H, W, 3, 64, ws, 0.125, int(case.split("vf")[1][0]), fmt)[3]
        else:
            B, H, W = 2, 32, 64
            prob = make_problem(B, H, W, 3, 64, 0, seed=63)
            aos[fmt] = run_fused(ops, "global", *prob, B, H, W, 3, 64, 0, 0.125, int(case.split("vf")[1][0]), fmt)[3]
    check_formats_agree(ops, aos, case)


# ------------------------------------------------------------------------------------------------------- zero padding per head is exact
def pad_heads(x, heads, hd_t, hd_p):
    """[N, groups*heads*hd_t] -> [N, groups*heads*hd_p], zero channels appended per head (backbone._pack's pad_head_rows, on columns)."""
    n = x.shape[0]
    v = x.reshape(n, -1, heads, hd_t)
    out = x.new_zeros(n, v.shape[1], heads, hd_p)
    out[..., :hd_t] = v
    return out.reshape(n, -1)


def pad_problem(prob, heads, hd_t, hd_p):
    qkv, bias, rph, rpw = prob
    pc = lambda t: torch.cat([t, t.new_zeros(t.shape[0], hd_p - hd_t)], 1)   # noqa: E731  (backbone._pack's pad_cols)
    return pad_heads(qkv, heads, hd_t, hd_p), pad_heads(bias.view(1, -1), heads, hd_t, hd_p).view(-1), pc(rph), pc(rpw)


def real_channels(x, heads, hd_t, hd_p):
    return x.reshape(x.shape[0], heads, hd_p)[..., :hd_t].reshape(x.shape[0], heads * hd_t)


def pad_channels(x, heads, hd_t, hd_p):
    return x.reshape(x.shape[0], heads, hd_p)[..., hd_t:]


@pytest.mark.parametrize("geom", ["win7_odd", "glob_fb32"])
@pytest.mark.parametrize("hd_t,hd_p", [(80, 96), (48, 64), (20, 32)])
def test_zero_padded_heads(ops, hd_t, hd_p, geom):
    """A problem of true head width hd_t run at hd_p the way backbone._pack pads it (zero q / k / v channels and bias per head, zero rel-pos
    columns, scale = hd_t^-0.5): the pad channels of `ao` are exactly 0.0 in every output format, and the real channels match float64 of the
    UNPADDED problem on the same operands.  Measured max_rel of the real channels: rows 3.4e-7 .. 1.5e-6; planes vf 0 within the hd-64
    values of test_attention_planes_vs_float64 (b3 <= 4.1e-6, h8c <= 2.1e-5); vf 1 6.7e-5 .. 1.3e-4."""
    B, H, W, ws = GEOMS[geom]
    heads = 3
    scale = hd_t ** -0.5
    prob = make_problem(B, H, W, heads, hd_t, ws, seed=hd_t + 71)
    pprob = pad_problem(prob, heads, hd_t, hd_p)
    ref, amax = ref_attention(prob[0].double(), prob[1].double(), prob[2].double(), prob[3].double(), B, H, W, heads, hd_t, ws, scale)
    out = run_prepass(ops, *pprob, B, H, W, heads, hd_p, ws, scale)[0]
    assert torch.all(pad_channels(out, heads, hd_t, hd_p) == 0.0), "rows: pad channels"
    check_leaf(("rows", 0, None), real_channels(out, heads, hd_t, hd_p), ref.cpu(), amax, f"rows hd {hd_t}->{hd_p} {geom}")
    for vf in (0, 1):
        for fmt in ALL_FMTS:
            gw = torch.zeros(1, device=DEV)
            out, (q64, b64), _, _ = run_prepass(ops, *pprob, B, H, W, heads, hd_p, ws, scale, vf=vf, out_fmt=fmt, guard=gw)
            what = f"planes hd {hd_t}->{hd_p} {geom} vf={vf} out={FMT_NAME[fmt]}"
            assert torch.all(pad_channels(out, heads, hd_t, hd_p) == 0.0), f"{what}: pad channels"
            # the same problem unpadded, on the operands the kernel read (their real channels)
            ref, amax = ref_attention(torch.cat([real_channels(q64[:, i * heads * hd_p:(i + 1) * heads * hd_p], heads, hd_t, hd_p)
                                                 for i in range(3)], 1),
                                      real_channels(b64.view(3, -1), heads, hd_t, hd_p).reshape(-1),
                                      prob[2].double(), prob[3].double(), B, H, W, heads, hd_t, ws, scale)
            check_leaf(("planes", vf, fmt), real_channels(out, heads, hd_t, hd_p), ref.cpu(), amax, what)
            check_guard(gw, amax, vf, what)


@pytest.mark.parametrize("geom", ["win14_pad", "glob_fb64", "glob_nofb"])
def test_hd64_padded_to_96_is_bit_identical(ops, geom):
    """The design's claim, stated directly: every term the padding adds is an exact zero.  A hd-64 problem padded to 96 per head gives
    bit-identical real channels to the same problem run at hd 64 -- the rel-pos prepass output, the fp32-rows kernel and the planes kernel
    (vf 0 and 1) -- with both kernels streaming keys in the same 64-key blocks (the K/V staging and the LDS sizing do not depend on HD; the
    extra MFMA k-step and d tiles only add zeros)."""
    B, H, W, ws = GEOMS[geom]
    heads, scale = 3, 64 ** -0.5
    prob = make_problem(B, H, W, heads, 64, ws, seed=81)
    pprob = pad_problem(prob, heads, 64, 96)
    o64, _, rp64 = run_prepass(ops, *prob, B, H, W, heads, 64, ws, scale)
    o96, _, rp96 = run_prepass(ops, *pprob, B, H, W, heads, 96, ws, scale)
    assert torch.equal(rp64, rp96), "rel-pos prepass: hd 96 (padded) != hd 64"
    assert torch.equal(o64, real_channels(o96, heads, 64, 96)), "fp32 rows: hd 96 (padded) != hd 64"
    for vf in (0, 1):
        a = run_prepass(ops, *prob, B, H, W, heads, 64, ws, scale, vf=vf, out_fmt=F3)
        b = run_prepass(ops, *pprob, B, H, W, heads, 96, ws, scale, vf=vf, out_fmt=F3)
        assert torch.equal(a[2], b[2]), f"planes rel-pos prepass vf={vf}: hd 96 (padded) != hd 64"
        assert torch.equal(a[0], real_channels(b[0], heads, 64, 96)), f"planes vf={vf}: hd 96 (padded) != hd 64"


def test_unsupported_widths_and_h8c_strides_are_refused(ops):
    """hd 80 and 128 unpadded are refused by every entry (the caller pads: backbone._pack); so is an h8c output whose row-pair stride is below
    3 * pad64(D).  Buffers are sized for the requested shapes, with slack rows, so that nothing is out of bounds even if a check were missing."""
    import mmsa
    B, H, W, heads = 1, 8, 8, 2
    T = H * W
    for hd in (80, 128):
        D = heads * hd
        qkv = torch.randn(B * T, 3 * D, device=DEV)
        rp = torch.zeros(B * heads * T, H + W, device=DEV)
        tab = torch.zeros(H, H, hd, device=DEV)
        with pytest.raises(RuntimeError):
            ops.relpos_bias(qkv, tab, tab, rp, B, H, W, heads, hd, 0)
        with pytest.raises(RuntimeError):
            ops.attention(qkv, torch.zeros(3 * D, device=DEV), rp, torch.empty(B * T, D, device=DEV), B, H, W, heads, hd, 0, hd ** -0.5)
        qp, bp = qkv_planes(ops, qkv.cpu(), torch.zeros(3 * D), D, 0)
        with pytest.raises(RuntimeError):
            ops.relpos_bias(qp, tab, tab, rp, B, H, W, heads, hd, 0)
        with pytest.raises(RuntimeError):
            ops.attention(qp, bp, rp, ops.alloc_planes(B * T, D, DEV), B, H, W, heads, hd, 0, hd ** -0.5)
    # fused entries: head_dim 64 only
    D = heads * 96
    qp, bp = qkv_planes(ops, torch.randn(B * T, 3 * D), torch.zeros(3 * D), D, 0)
    with pytest.raises(RuntimeError):
        ops.window_attention(qp, bp, ops.window_relpos_planes(torch.zeros(13, 96, device=DEV), torch.zeros(13, 96, device=DEV), 7, fmt=F3),
                             ops.alloc_planes(B * T, D, DEV), B, H, W, heads, 96, 7, 96 ** -0.5)
    with pytest.raises(RuntimeError):
        ops.global_attention(qp, bp, ops.global_relpos_planes(torch.zeros(15, 96, device=DEV), torch.zeros(15, 96, device=DEV), fmt=F3),
                             ops.alloc_planes(B * T, D, DEV), B, H, W, heads, 96, 96 ** -0.5)
    # h8c output with a pair stride of 3 * (pad64(D) - 64): accepted by the Python wrapper (kpad declared 64 short), refused by the library
    for hd, heads_ in ((96, 3), (64, 3)):
        D = heads_ * hd
        kp = ops.pad64(D) - 64
        n = B * T + 1                        # odd row count
        short = mmsa.ops.Planes(torch.zeros((n + 1) // 2 + 16, 3 * kp, dtype=torch.int16, device=DEV), n, D, kp, H8C)
        qkv, bias, rph, rpw = make_problem(B, 1, n, heads_, hd, 0, seed=91)
        qp, bp = qkv_planes(ops, qkv, bias, D, 0)
        rp = torch.zeros(B * heads_ * n, 1 + n, device=DEV)
        with pytest.raises(RuntimeError):
            ops.attention(qp, bp, rp, short, B, 1, n, heads_, hd, 0, hd ** -0.5)
        if hd == 64:
            with pytest.raises(RuntimeError):
                ops.window_attention(qp, bp, ops.window_relpos_planes(torch.zeros(13, 64, device=DEV), torch.zeros(13, 64, device=DEV), 7, fmt=F3),
                                     short, B, 1, n, heads_, hd, 7, 0.125)
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ model level at a padded head width
@pytest.mark.parametrize("name", ["hd80_256", "hd80_256_peaky"])
def test_padded_head_width_model(golden_dir, name):
    """embed 320 / 4 heads = head_dim 80, run zero-padded to 96 per head (as ViT-H), MSDA heads of 40 channels, against the fp32 oracle (full
    tensors) and the imported reference's probes (tests/golden/model_<name>.npz).  The seeded weights keep every block on fp16 attention
    (max |logit| ~3); with q / k x 3 (peaky_attention, max |logit| ~21-24) the guard moves every block to fp16 hi/lo pairs.  The packed
    weights hold exact zeros in the pad rows (qkv) and pad columns (proj) and the rel-pos tables in their pad columns."""
    import mmsa
    cfg = CONFIGS[name]
    kw = cfg["kwargs"]
    D, heads = kw["embed_dim"], kw["num_heads"]
    torch.manual_seed(0)
    orc = R.OracleEncoder(**kw)
    sd = seeded_state_dict(orc, seed=cfg["seed"])
    if cfg.get("qk_scale"):
        sd = peaky_attention(sd, D, cfg["qk_scale"])
    orc.load_state_dict(sd)
    m = mmsa.build_backbone(dict(type="SAMAdapterbimodalMixModNewInTwinConvNEW", **kw))
    m.load_state_dict(sd, strict=True)
    x = make_input(cfg)
    fs, _ = m(x.to(DEV))
    torch.cuda.synchronize()
    assert (m._hd_true, m._hd_pad) == (80, 96)
    modes = m.attention_modes()
    if cfg.get("qk_scale"):
        assert all(mode == "b3" and lg > 2 * m.ATTN_F16_MAX_LOGIT for mode, lg in modes), modes
    else:
        assert all(mode == "f16" and 0.0 < lg <= m.ATTN_F16_MAX_LOGIT for mode, lg in modes), modes
    with torch.no_grad():
        ref, _ = orc(x)
    gold = np.load(os.path.join(golden_dir, f"model_{name}.npz"))
    for i, (f, r) in enumerate(zip(fs, ref)):
        assert_close(f, r, what=f"{name} f{i+1} vs oracle")
        pi = probe_index(f.numel(), 2048, seed=100 + i)
        assert_close(f.flatten()[pi.to(DEV)].cpu(), torch.from_numpy(gold[f"f{i+1}_probe"]), what=f"{name} f{i+1} probes")
        st = gold[f"f{i+1}_stats"]
        assert abs(f.double().pow(2).sum().sqrt().item() - st[3]) <= 1e-3 * st[3], f"{name} f{i+1} norm"
    for bp in m._packed["blocks"]:
        qkv_w = planes_to_float(bp["qkv"])[:3 * heads * 96].reshape(3, heads, 96, -1)
        assert torch.all(qkv_w[:, :, 80:] == 0.0) and torch.any(qkv_w[:, :, :80] != 0.0), "qkv planes: pad rows"
        for key in ("qkv_b", "qkv_bf"):
            if bp.get(key) is not None:
                assert torch.all(bp[key].reshape(3, heads, 96)[:, :, 80:] == 0.0), f"{key}: pad rows"
        proj_w = planes_to_float(bp["proj"])[:D, :heads * 96].reshape(D, heads, 96)
        assert torch.all(proj_w[:, :, 80:] == 0.0) and torch.any(proj_w[:, :, :80] != 0.0), "proj planes: pad columns"
        assert torch.all(bp["rph"][:, 80:] == 0.0) and torch.all(bp["rpw"][:, 80:] == 0.0), "rel-pos tables: pad columns"
