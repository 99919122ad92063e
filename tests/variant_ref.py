"""Float64 restatements of the conv / norm / neck / tail / head, LayerNorm-rows, row-statistics and deformable-attention (forward and backward) operations and the per-element bound the kernel-variant tests hold the
device to (tests/test_kernel_variants_gpu.py; tests/test_kernel_variants_cpu.py keeps the bound itself honest).

Every `ref_<op>(i, p)` takes the case's inputs `i` (a dict of CPU tensors, all of ONE floating dtype) and its parameters `p` and returns
(r, bnd) in the layout the device writes: evaluated on float64 inputs, r is the reference and bnd the bound; evaluated on the float32 inputs
it is torch's own fp32 evaluation of the same operation (bnd is then ignored).

The bound.  A result formed as a sum of n products with magnitude sum s = sum |x_i| |w_i| + |bias| passes when, element by element,
    |y - r| <= (n + 4) * 2^-24 * s + a
-- the standard fp32 accumulation bound (n + 4 roundings of relative size 2^-24 on every path through the sum) plus the activation's own absolute
error a, scaled by whatever multiplies the activation.  Nothing measured goes into the first term.

The LayerNorm-rows, row-statistics and deformable-attention (MSDA) operations have bounds of their own, derived here; u = 2^-24.

layernorm_rows (csrc/norm.hip).  Reference, per row: mu and the biased variance over C, rho = 1 / sqrt(var + eps), y = (x - mu) rho w_g + b_g, y2 = y + x;
eps is the fp32 value the launcher receives.  Let Dp be the longest chain of additions behind the row sum: two inside a float4, NV - 1 across a lane's
float4s, six (one row per wave) or five (two rows per wave) butterfly steps; a = mean_c |x_c|, d_c = x_c - mu.
    mean        the sum carries Dp roundings on every path, the division one more:                 delta_mu = (Dp + 1) u a
    difference  the device's d_c is off by the mean's error plus its own rounding:                 e_c = delta_mu + u (|d_c| + delta_mu)
    variance    squares, the same sum, the division: (Dp + 3) u var; d^2 moves by 2 |d_c| e_c:     delta_sigma2 = (Dp + 3) u var + 2 mean_c(|d_c| e_c)
    rstd        relative: the variance's error through 1 / sqrt, and three correctly rounded operations (eps add, sqrt, divide -- the build uses neither
                fast-math nor approximate division):                                               E_rho = delta_sigma2 / (2 (var + eps)) + 3 u
    y           d rho w + b, three roundings on the product, two on the sum:
                                                                   bnd_y = |w| rho (e_c + |d_c| (E_rho + 3 u)) + 2 u (|w rho d_c| + |b|)
    y2          one more addition:                                                                 bnd_y2 = bnd_y + u |y2|

rowstats (rowstats_finalize_kernel).  From the given fp32 strip sums, in float64 on the device as here: mean = s1 / D, var = max(s2 / D - mean^2, 0), rstd =
1 / sqrt(var + eps).  The device's double arithmetic adds `strips` terms and a handful of operations (2^-53 each, amplified by the cancellation
(s2 / D) / (var + eps)) and rounds once to fp32:        mean: u |mean|;       rstd: rstd (u + 2^-53 (strips + 4) (s2 / D) / (var + eps)).

msda / msda_fused (csrc/msda.hip).  Reference: a direct gather.  pixel = loc * (W, H) - 0.5; a sample counts iff -1 < h < H and -1 < w < W; four taps, a
tap outside the map is zero; out = sum over l, p of weight * bilinear.  The fused form first computes loc = ref + off / (W_l, H_l) and weights = softmax
over L * P of the logits.  Per sample s: A_s the weight, c_k the float64 bilinear weights, v_k the tap values.
    S1 = sum_s |A_s| sum_k c_k |v_k|,  T_s = sum over the existing taps of |v_k|
    eps_h = 2 u (|ly H| + 0.5), eps_w = 2 u (|lx W| + 0.5): the product and the subtraction behind a pixel coordinate (the fused form has the division
    and the addition in front of them: 4 u (|r H| + |off| + 0.5)); a coordinate's error moves the bilinear value by at most that times T_s
    bnd = (n + 12) u S1 + sum_s |A_s| (eps_h + eps_w) T_s
    n = the terms accumulated per element: L P (msda_kernel, msda_scalar_kernel), 4 L P (msda_planes_kernel<false>), 8 L P (<true>); the 12 covers the
    roundings of lh, hh, the tap weight products and the multiplication by the sample weight.
The position term holds only while both evaluations take the same four taps, so make_msda* moves every drawn sample whose float64 pixel coordinate lies
within 2^-12 of an integer (-1, H and W are integers) a quarter pixel away from it, to the side it lay on; the exact coordinates are the business of the
dyadic cases, whose every coordinate is exact in fp32 and whose position term is therefore zero.
Fused weights: exp(logit - max) / sum: the subtraction (u |logit - max| on the exponent), the exponential, L P additions, the division, the
product with the reciprocal: relative (L P + 6 + max |logit - max|) u, times S1 -- plus what the runtime's expf adds, which the source cannot tell:
EXPF_EXCESS below, handled like SIGMOID_EXCESS (measured against float64 on an MI355X, twice the measured value allowed, relative to S1).
Scalar kernels: f16 computes in fp32 on the fp16 inputs as given and rounds once: the fp32 bound + 2^-11 |r| + 2^-24; f64: the formula with u = 2^-53.
Planes-only outputs: bnd + FMT_REL |r|.

msda_bwd (msda_bwd_kernel<T, SHFL>).  Reference: the three gradients of the gather above, stated directly (the comment above the kernel).  Per sample
s = (b, q, m, l, p) inside the map, with the fractions lh, lw of its pixel coordinate, hh = 1 - lh, hw = 1 - lw, the four taps k = (dy, dx) with bilinear
weights c_k = (lh | hh)(lw | hw), tap values v_k (zero outside the map), A_s the attention weight and g_c = grad_output[b, q, m, c]:
    grad_value[tap k, c]     += c_k A_s g_c                                            over every sample and tap that lands on the element
    grad_attn_weight[s]       = sum_c g_c sum_k c_k v_k
    grad_sampling_loc[s, x]   = W_l A_s sum_c g_c sum_k (+-)(lh | hh) v_k              (+ for dx = 1, - for dx = 0; the factor is the tap's row weight)
    grad_sampling_loc[s, y]   = H_l A_s sum_c g_c sum_k (+-)(lw | hw) v_k              (+ for dy = 1, - for dy = 0; the factor is the tap's column weight)
A sample outside the map contributes nothing and has gradient zero.  The device forms the pixel coordinate as above (error eps_h, eps_w), then lh by a
subtraction of the floor (one rounding when the coordinate is negative) and hh = 1 - lh (one more): every one of lh, hh carries at most
e_h = eps_h + 2 u, every one of lw, hw at most e_w = eps_w + 2 u, absolute, and all four lie in [0, 1].  T_c = the sum of |v_k| over the existing taps of
channel c, as T_s above.
    grad_value element e.  n_e = the number of (sample, tap) contributions that land on it, S_e = sum c_k |A_s| |g_c| over them.  An addend is
        fl(fl(hh hw) fl(g A)): three roundings relative to itself, and the weight c_k moves by at most hw e_h + hh e_w <= e_h + e_w; the n_e addends
        meet in atomics, n_e - 1 roundings on any path whatever the order (the first lands on the memset zero, exactly); two more u absorb the second-order
        terms (n_e stays below 2^10):                   bnd = (n_e + 4) u S_e + sum |A_s g_c| (e_h + e_w)
        An element no sample touches: r = 0, bnd = 0 -- the device must leave the memset zero.
    grad_attn_weight[s].  Per channel: the weight product and the product with v_k (2 u on each term), three additions over the taps, the product with
        g_c; then D channels meet (log2 D shuffle steps, or D - 1 atomic additions: D bounds both):
                                                        bnd = (D + 8) u sum_c |g_c| sum_k c_k |v_k| + sum_c |g_c| (e_h + e_w) T_c
    grad_sampling_loc[s, x].  Per channel: one product per tap, three additions, the roundings of g A, of W_l dw and of their product; D channels meet;
        the coefficients (lh | hh) carry e_h:           bnd = (D + 8) u W_l |A_s| sum_c |g_c| sum_k (lh | hh) |v_k| + W_l |A_s| e_h sum_c |g_c| T_c
        and [s, y] likewise with H_l, (lw | hw) and e_w.  A sample outside the map: r = 0, bnd = 0.
In the dyadic cases every coordinate, fraction and weight product is exact, so e_h = e_w = 0 there.  f64: the same formulas with u = 2^-53.
f16: the inputs are the fp16 numbers as given and the arithmetic is fp32, so the fp32 bound b32 holds for what the device has before it stores.
    shuffle path, grad_sampling_loc and grad_attn_weight: one rounding to fp16:          b32 + 2^-11 |r| + 2^-24   (inside the map; outside r = bnd = 0)
    atomics path, and grad_value always: every addend is rounded to fp16 and so is every partial sum (global_atomic_pk_add_f16).  With n addends
    (n_e, or D for a sample inside the map) of magnitude sum S' <= S + b32, n roundings of relative size 2^-11 lie on any path:
                                                        b32 + ((1 + 2^-11)^n - 1) (S + b32) + n (2^-14 + 2^-24)
    The last term is the one thing the source cannot tell: whether the packed fp16 atomic keeps subnormal addends and sums or flushes them to zero.
    It is NOT measured: 2^-14, the smallest normal fp16 number, is the most a flush can cost per addend, and 2^-24 covers the conversion's rounding in the
    subnormal range when they are kept."""
import zlib

import torch
import torch.nn.functional as F

U = 2.0 ** -24
GELU_ABS = 3.3e-7          # csrc/common.h: the fp32 evaluation of the degree-7 erfc polynomial, absolute
# sigmoid and hswish go through the runtime's expf / division: their error is not derivable from the source.  The figure is the largest excess of
# |y - r| over the accumulation term against float64 on an MI355X, over every sigmoid / hswish case of the table (fp32 outputs); twice it is allowed.
SIGMOID_EXCESS = 2.0e-8    # measured 1.99977671e-08 (dw3-nhwc-1x7-c64-sigmoid-b0); every other sigmoid case stays below the accumulation term
HSWISH_EXCESS = 0.0        # measured: no excess, the closest case stays 6.04e-09 BELOW the accumulation term (dw3-nhwc-1x7-c36-hswish-b0)
ACT_ABS = {"none": 0.0, "relu": 0.0, "relu6": 0.0, "gelu": GELU_ABS, "sigmoid": 2 * SIGMOID_EXCESS, "hswish": 2 * HSWISH_EXCESS}
# msda_kernel<true> / msda_planes_kernel form their softmax weights with the runtime's expf.  The figure is the largest excess of |y - r| over the derived
# part of the bound, relative to S1 (the magnitude sum the weight errors scale with; O(1) at the magnitudes of the table), against float64 on an MI355X
# over every msda_fused case (fp32 outputs); twice it is allowed.
EXPF_EXCESS = 0.0          # measured: no excess, the closest case stays 2.07e-06 S1 BELOW the derived part (msda-dyadic-fused; ref_msda_fused(parts=True))
assert max(max(ACT_ABS.values()), 2 * EXPF_EXCESS) <= 1e-6   # a larger allowance would be a finding about the kernel, not a tolerance
# rounding of the operand formats themselves (relative to |r|), where only planes can be compared: bf16 hi/lo, fp16 hi/lo, fp16 hi + e5m2 lo (h8c: the
# same arithmetic as h8 on 3 bytes per element)
FMT_REL = {"b3": 2.0 ** -16, "f3": 2.0 ** -22, "h8": 2.0 ** -14, "h8c": 2.0 ** -14}
ACTS = ("none", "gelu", "relu", "relu6", "hswish", "sigmoid")


def act_fn(name):
    return {"none": lambda t: t, "gelu": F.gelu, "relu": F.relu, "relu6": F.relu6, "hswish": lambda t: t * F.relu6(t + 3) / 6,
            "sigmoid": torch.sigmoid}[name]


def gen_for(case_id):
    return torch.Generator().manual_seed(zlib.crc32(case_id.encode()))


def nhwc(t):
    b, c, h, w = t.shape
    return t.permute(0, 2, 3, 1).reshape(b * h * w, c).contiguous()


def bound(n, s, a=0.0):
    return (n + 4) * U * s + a


def violations(y, r, bnd):
    """Boolean tensor of the elements outside the bound (NaN counts as outside)."""
    return ~((y.double() - r.double()).abs() <= bnd.double())


def assert_inside(y, r, bnd, what):
    y = y.detach().cpu()
    assert y.shape == r.shape, f"{what}: shape {tuple(y.shape)} vs {tuple(r.shape)}"
    bad = violations(y, r, bnd)
    err = (y.double() - r.double()).abs()
    ratio = float((err / bnd.double().clamp_min(1e-300)).max()) if err.numel() else 0.0
    if bool(bad.any()):
        k = int(torch.argmax((err / bnd.double().clamp_min(1e-300)).flatten().nan_to_num(float("inf"))))
        idx = tuple(int(v) for v in torch.unravel_index(torch.tensor(k), y.shape))
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.numel()} elements outside the bound; worst at {idx}: got {float(y[idx])!r}, "
                             f"reference {float(r[idx])!r}, bound {float(bnd[idx]):.3e}")
    return ratio


def cast(i, dt):
    """The case's fp32 inputs in dtype `dt`; inputs the device takes as double (statistics, Gram matrices) stay double."""
    o = {k: (v.to(dt) if torch.is_tensor(v) and v.dtype == torch.float32 else v) for k, v in i.items()}
    o["_dt"] = dt
    return o


# ------------------------------------------------------------------------------------------------ convs
def make_dwconv(p, g):
    B, C, H, W, k = p["B"], p["C"], p["H"], p["W"], p["k"]
    ng = B // p["ipg"] if p.get("ipg") else 1
    i = dict(x=torch.randn(B, C, H, W, generator=g), w=torch.randn(ng, C, 1, k, k, generator=g) / k)
    if p.get("bias"):
        i["b"] = torch.randn(ng, C, generator=g)
    return i


def ref_dwconv(i, p):
    x, w, k = i["x"], i["w"], p["k"]
    B, C = x.shape[:2]
    ng = w.shape[0]
    pre, s = [], []
    for gi in range(ng):
        xs = x[gi * (B // ng):(gi + 1) * (B // ng)]
        b = i["b"][gi] if "b" in i else None
        pre.append(F.conv2d(xs, w[gi], b, padding=k // 2, groups=C))
        s.append(F.conv2d(xs.abs(), w[gi].abs(), None if b is None else b.abs(), padding=k // 2, groups=C))
    pre, s = torch.cat(pre), torch.cat(s)
    return nhwc(act_fn(p["act"])(pre)), nhwc(bound(k * k, s, ACT_ABS[p["act"]]))


def make_gconv(p, g):
    B, G, ci, co, H, W, k = p["B"], p["G"], p["cin_g"], p["cout_g"], p["H"], p["W"], p["k"]
    i = dict(x=torch.randn(B, G * ci, H, W, generator=g), w=torch.randn(G * co, ci, k, k, generator=g) / (ci * k * k) ** 0.5)
    if p.get("bias"):
        i["b"] = torch.randn(G * co, generator=g)
    return i


def ref_gconv(i, p):
    k, G = p["k"], p["G"]
    b = i.get("b")
    pre = F.conv2d(i["x"], i["w"], b, padding=k // 2, groups=G)
    s = F.conv2d(i["x"].abs(), i["w"].abs(), None if b is None else b.abs(), padding=k // 2, groups=G)
    return nhwc(act_fn(p["act"])(pre)), nhwc(bound(k * k * p["cin_g"], s, ACT_ABS[p["act"]]))


def make_gfe_qkv(p, g):
    B, G, ci, co, H, W = p["B"], p["G"], p["cin_g"], p["cout_g"], p["H"], p["W"]
    return dict(x=torch.randn(B, G * ci, H, W, generator=g), q1=torch.randn(G * co, ci, 1, 1, generator=g) / ci ** 0.5,
                q2=torch.randn(G * co, co, 3, 3, generator=g) / (9 * co) ** 0.5)


def ref_gfe_qkv(i, p):
    """qkv2(qkv1(x)).  The device contracts x with the folded weights W_eff (float64 fold, one rounding to fp32: inside the + 4)."""
    G, ci, co = p["G"], p["cin_g"], p["cout_g"]
    r = F.conv2d(F.conv2d(i["x"], i["q1"], groups=G), i["q2"], padding=1, groups=G)
    weff = torch.einsum("gmi,gomhw->goihw", i["q1"].reshape(G, co, ci), i["q2"].reshape(G, co, co, 3, 3)).reshape(G * co, ci, 3, 3)
    s = F.conv2d(i["x"].abs(), weff.abs(), padding=1, groups=G)
    return nhwc(r), nhwc(bound(9 * ci, s))


def make_dwpair_gate(p, g):
    B, C, H, W = p["B"], p["C"], p["H"], p["W"]
    return dict(x=torch.randn(B, 2 * C, H, W, generator=g), w=torch.randn(2 * C, 2, 3, 3, generator=g) / 18 ** 0.5)


def ref_dwpair_gate(i, p):
    """gelu(a1) * a2 with (a1 | a2) = the 2-in / 2-out grouped 3x3 conv of x: n = 18 products behind each factor; the GELU error is scaled by |a2|."""
    C = p["C"]
    a = F.conv2d(i["x"], i["w"], padding=1, groups=C)
    s = F.conv2d(i["x"].abs(), i["w"].abs(), padding=1, groups=C)
    g1, a2 = F.gelu(a[:, :C]), a[:, C:]
    return nhwc(g1 * a2), nhwc(bound(18, s[:, :C] * a2.abs() + g1.abs() * s[:, C:], GELU_ABS * a2.abs()))


# ------------------------------------------------------------------------------------------------ neck element-wise / pooling
def make_ca_apply(p, g):
    B, C, H, W = p["B"], p["C"], p["H"], p["W"]
    return dict(z=torch.randn(B * H * W, C, generator=g), att=torch.rand(B * (H + W), C, generator=g))


def ref_ca_apply(i, p):
    B, C, H, W = p["B"], p["C"], p["H"], p["W"]
    z = i["z"].view(B, H, W, C)
    att = i["att"].view(B, H + W, C)
    t = z * att[:, H:, None, :].transpose(1, 2) * att[:, :H, None, :]      # a_w[b, w, c] * a_h[b, h, c]
    return (z + t).reshape(B * H * W, C), bound(2, z.abs() + t.abs()).reshape(B * H * W, C)


def make_gelu_gate(p, g):
    return dict(x=torch.randn(p["B"] * p["H"] * p["W"], 2 * p["C"], generator=g) * 2)


def ref_gelu_gate(i, p):
    C = p["C"]
    x1, x2 = i["x"][:, :C], i["x"][:, C:]
    r = F.gelu(x1) * x2
    return r, bound(1, r.abs(), GELU_ABS * x2.abs())


def make_pool_hw(p, g):
    return dict(z=torch.randn(p["B"] * p["H"] * p["W"], p["C"], generator=g) + 0.3)


def ref_pool_hw(i, p):
    B, C, H, W = p["B"], p["C"], p["H"], p["W"]
    z = i["z"].view(B, H, W, C)
    r = torch.cat([z.mean(2), z.mean(1)], 1).reshape(B * (H + W), C)
    s = torch.cat([z.abs().mean(2), z.abs().mean(1)], 1)
    n = torch.cat([torch.full((H,), float(W)), torch.full((W,), float(H))]).to(torch.float64)[None, :, None]
    return r, ((n + 4) * U * s.double()).reshape(B * (H + W), C)


# ------------------------------------------------------------------------------------------------ colstats -> ffrm_finalize -> lnhw_apply
def make_colstats(p, g):
    B, C, HW = p["B"], p["C"], p["HW"]
    i = dict(x=torch.randn(B * HW, C, generator=g) * 2 + 0.5)
    if p["wrow"]:
        i["wrow"] = torch.randn(HW, generator=g) * 0.2 + 1
    return i


def ref_colstats(i, p):
    """[B*3, C] double: sum x, sum x^2, sum wrow x.  The device adds at most 8 rows in fp32 before it continues in double: n = 8."""
    B, C, HW = p["B"], p["C"], p["HW"]
    x = i["x"].view(B, HW, C)
    w = i["wrow"].view(1, HW, 1) if "wrow" in i else torch.zeros(1, HW, 1, dtype=x.dtype)
    r = torch.stack([x.sum(1), (x * x).sum(1), (w * x).sum(1)], 1)
    s = torch.stack([x.abs().sum(1), (x * x).sum(1), (w * x).abs().sum(1)], 1)
    return r.reshape(B * 3, C), bound(8, s).reshape(B * 3, C)


def make_ffrm(p, g):
    B, C, HW = p["B"], p["C"], p["HW"]
    x = torch.randn(B, HW, C, generator=g) * 2 + 0.5
    lw = torch.randn(HW, generator=g) * 0.2 + 1
    st = torch.stack([x.double().sum(1), (x.double() ** 2).sum(1), (lw.double().view(1, HW, 1) * x.double()).sum(1)], 1)   # exact statistics in
    return dict(stats=st.reshape(B * 3, C), wc=torch.randn(C, C, generator=g) / C ** 0.5, gn_w=torch.randn(C, generator=g) * 0.5 + 1,
                gn_b=torch.randn(C, generator=g) * 0.5, mean_w=float(lw.double().mean()), mean_b=0.125)


def ref_ffrm(i, p):
    """(mean | rstd | mult), [3*B, C], from the SAME double statistics.  mean and rstd are one rounding of a double result (4 u allowed).  mult =
    1 + sigmoid(relu(GroupNorm32(Wc avg))): the matvec's accumulation error E (n = C, plus the rounding of avg) passes through the group norm,
    whose derivative is at most |gn_w| / sigma * (2 + cg) in the group's largest E; the norm's own fp32 evaluation adds (cg + 8) u (|t - gn_b| + |gn_b|)
    and (cg + 2) u max|z| on the centred value; the sigmoid has slope <= 1/4.  In the fp32 evaluation only the statistics (mean, rstd, avg) are formed
    in double, as on the device, which receives them as double; the matvec, the group norm and the gate run in fp32."""
    B, C, HW = p["B"], p["C"], p["HW"]
    st = i["stats"].double().view(B, 3, C)
    dt = i["_dt"]
    m = st[:, 0] / HW
    rs = 1.0 / torch.sqrt((st[:, 1] / HW - m * m).clamp_min(0) + 1e-5)
    avg = (rs * (st[:, 2] / HW - m * i["mean_w"]) + i["mean_b"]).to(dt)
    z = avg @ i["wc"].t()
    cg = C // 32
    zg = z.view(B, 32, cg)
    d = zg - zg.mean(2, keepdim=True)
    sig = torch.sqrt((d * d).mean(2, keepdim=True) + 1e-5)
    t = ((d / sig).reshape(B, C) * i["gn_w"] + i["gn_b"])
    mult = 1 + torch.sigmoid(F.relu(t))
    ez = bound(C, avg.abs() @ i["wc"].abs().t()) + (cg + 2) * U * zg.abs().amax(2, keepdim=True).expand(B, 32, cg).reshape(B, C)
    eg = ez.view(B, 32, cg).amax(2, keepdim=True).expand(B, 32, cg).reshape(B, C)
    et = i["gn_w"].abs() / sig.expand(B, 32, cg).reshape(B, C) * (2 + cg) * eg + (cg + 8) * U * ((t - i["gn_b"]).abs() + i["gn_b"].abs())
    r = torch.cat([m.to(dt), rs.to(dt), mult], 0)
    return r, torch.cat([4 * U * m.abs(), 4 * U * rs.abs(), et / 4 + ACT_ABS["sigmoid"] + 4 * U * mult.abs()], 0)


def make_lnhw(p, g):
    B, C, HW = p["B"], p["C"], p["HW"]
    return dict(x=torch.randn(B * HW, C, generator=g) * 2 + 0.5, mean=torch.randn(B, C, generator=g) * 0.3 + 0.5, rstd=torch.rand(B, C, generator=g) + 0.3,
                mult=torch.rand(B, C, generator=g) + 1, w=torch.randn(HW, generator=g) * 0.2 + 1, b=torch.randn(HW, generator=g) * 0.1)


def ref_lnhw(i, p):
    """((x - mean) rstd w[p] + bias[p]) mult: two terms behind five roundings (n = 2)."""
    B, C, HW = p["B"], p["C"], p["HW"]
    x = i["x"].view(B, HW, C)
    m, rs, mu = (i[k].view(B, 1, C) for k in ("mean", "rstd", "mult"))
    w, b = i["w"].view(1, HW, 1), i["b"].view(1, HW, 1)
    r = ((x - m) * rs * w + b) * mu
    s = ((x.abs() + m.abs()) * (rs * w).abs() + b.abs()) * mu.abs()
    return r.reshape(B * HW, C), bound(2, s).reshape(B * HW, C)


# ------------------------------------------------------------------------------------------------ gram and the two plane builders
def make_gram(p, g):
    return dict(xy=torch.randn(p["B"] * p["P"], 2 * p["c"], generator=g))


def gram_mask(c, nblk):
    """Entries of G that gram_tn defines: all of them, or (nblk > 1) the diagonal head blocks."""
    h = torch.arange(c) // (c // nblk)
    return h[:, None] == h[None, :]


def ref_gram(i, p):
    """G[b] = X[b]^T Y[b], [B*c, c] double; fp32 on the matrix pipe inside one 256-row slice, slices added in double: n = 256."""
    B, P, c = p["B"], p["P"], p["c"]
    xy = i["xy"].view(B, P, 2 * c)
    x, y = xy[..., :c], xy[..., c:]
    r = torch.einsum("bpi,bpj->bij", x, y)
    s = torch.einsum("bpi,bpj->bij", x.abs(), y.abs())
    return r.reshape(B * c, c), bound(min(P, 256), s).reshape(B * c, c)


def make_chanattn(p, g):
    B, c, heads = p["B"], p["c"], p["heads"]
    P = 64
    q, k = torch.randn(B, P, c, generator=g), torch.randn(B, P, c, generator=g)
    k = k + 0.7 * q                                                             # correlated channels: logits that are not all alike
    return dict(G=torch.einsum("bpi,bpj->bij", q.double(), k.double()).reshape(B * c, c), sq=(q.double() ** 2).sum(1), sk=(k.double() ** 2).sum(1),
                temp=torch.rand(heads, generator=g) * 2 + 0.5, wp=torch.randn(c, c, generator=g) / c ** 0.5)


def ref_chanattn(i, p):
    """Wcomb[b][o][j] = sum_i Wp[o][i] attn[b][i][j], attn = per-head softmax_j(G_ij / (|q_i| |k_j|) * temp_h), from the SAME double Gram matrix.
    Planes only (bf16 hi/lo).  The fp32 logit carries <= 9 roundings (|logit| <= temp), on itself and on the row maximum it is shifted by: the
    softmax value is off by at most (18 temp + ch + 12) u relative (exponent argument, exponential, the ch-term sum, the division); the product
    sum over the head's ch channels adds (ch + 4) u; both scale with s = sum |Wp| attn.  The format rounds the result: 2^-16 |r|."""
    B, c, heads = p["B"], p["c"], p["heads"]
    ch = c // heads
    dt = i["_dt"]
    Gm = i["G"].double().view(B, c, c)
    nq, nk = i["sq"].double().sqrt().clamp_min(1e-12), i["sk"].double().sqrt().clamp_min(1e-12)
    tfull = i["temp"].double().repeat_interleave(ch)
    # the cosine is a double quotient of double inputs on the device too; from its rounding to the working type on, everything is in that type
    logit = (Gm / (nq[:, :, None] * nk[:, None, :])).to(dt) * i["temp"].repeat_interleave(ch)[None, :, None]
    same = gram_mask(c, heads)
    attn = torch.softmax(logit.masked_fill(~same, float("-inf")), -1)
    r = torch.einsum("oi,bij->boj", i["wp"], attn)
    s = torch.einsum("oi,bij->boj", i["wp"].abs(), attn)
    eps = ((18 * tfull.abs().max() + ch + 12) + (ch + 4)) * U
    return r.reshape(B * c, c), (eps * s + FMT_REL["b3"] * r.abs()).reshape(B * c, c)


def make_gffm(p, g):
    B, c = p["B"], p["c"]
    return dict(E=(torch.randn(B, c, c, generator=g).double() * 4).reshape(B * c, c))


def ref_gffm(i, p):
    """(softmax_j E[i][j] | softmax_j E[j][i]) as [2*B*c, c], planes only.  The exponent argument E - max is one fp32 rounding of a double
    difference d (|d| u absolute), the exponential, the c-term sum and the division add (c + 12) u relative; the format rounds: 2^-16 |r|."""
    B, c = p["B"], p["c"]
    E = i["E"].double().view(B, c, c)
    out, bnd = [], []
    for e in (E, E.transpose(1, 2)):
        d = e - e.float().amax(-1, keepdim=True).double()
        r = torch.softmax(e, -1)
        out.append(torch.softmax(e.to(i["_dt"]), -1).reshape(B * c, c))
        bnd.append((((d.abs() + c + 12) * U + FMT_REL["b3"]) * r).reshape(B * c, c))
    return torch.cat(out), torch.cat(bnd)


# ------------------------------------------------------------------------------------------------ tail and head
def _bilinear(x, size):
    return x if tuple(x.shape[2:]) == tuple(size) else F.interpolate(x, size=size, mode="bilinear", align_corners=False)


def make_tail(p, g):
    B, C = p["B"], p["C"]
    i = dict(cm=torch.randn(B, C, p["Hc"], p["Wc"], generator=g), scale=torch.randn(C, generator=g), shift=torch.randn(C, generator=g))
    if p["xtok"]:
        i["xt"] = torch.randn(B, C, p["Hx"], p["Wx"], generator=g)
    return i


def ref_tail(i, p):
    """(cmap + bilinear(xtok)) * scale + shift as NCHW: the four taps' products, the two adds and the affine are 8 roundings (n = 4).  The source
    coordinates are exact in fp32 for the power-of-two scale factors the encoder uses."""
    cm, sc, sh = i["cm"], i["scale"].view(1, -1, 1, 1), i["shift"].view(1, -1, 1, 1)
    up = _bilinear(i["xt"], cm.shape[2:]) if "xt" in i else torch.zeros_like(cm)
    ups = _bilinear(i["xt"].abs(), cm.shape[2:]) if "xt" in i else torch.zeros_like(cm)
    return (cm + up) * sc + sh, bound(4, (cm.abs() + ups) * sc.abs() + sh.abs())


def make_nchw_to_planes(p, g):
    return dict(x=torch.randn(p["B"], p["C"], p["HW"], generator=g))


def ref_nchw_to_planes(i, p):
    """[B, C, HW] -> [B*HW, C] bf16 hi/lo planes: no arithmetic, the format's rounding only."""
    r = i["x"].permute(0, 2, 1).reshape(p["B"] * p["HW"], p["C"])
    return r, bound(0, r.abs()) + FMT_REL["b3"] * r.abs()


def make_tokens_to_nchw(p, g):
    return dict(x=torch.randn(p["B"] * p["HW"], p["C"], generator=g))


def ref_tokens_to_nchw(i, p):
    r = i["x"].view(p["B"], p["HW"], p["C"]).permute(0, 2, 1).contiguous()
    return r, bound(0, r.abs())


def make_head_fuse(p, g):
    B, C = p["B"], p["C"]
    i = dict(scale=torch.randn(C, generator=g), shift=torch.randn(C, generator=g))
    for l, (h, w) in enumerate(p["sizes"]):
        i[f"z{l}"] = torch.randn(B, C, h, w, generator=g)
    return i


def ref_head_fuse(i, p):
    """relu((z0 + sum_l bilinear(z_l)) * scale + shift), [B*H*W, C].  A resized level is a sum of n = 4 tap products; here three resized levels and z0
    meet in ONE sum of 3 * 4 + 1 = 13 products before the affine, so the n of the bound is the 12 taps of that sum (n = 4 per resized level, as
    tail_fuse with its single level uses n = 4), not a looser figure for one resize.  The level sizes are power-of-two ratios of the output size, so
    the source coordinates are exact in fp32."""
    size = i["z0"].shape[2:]
    sc, sh = i["scale"].view(1, -1, 1, 1), i["shift"].view(1, -1, 1, 1)
    nl = len(p["sizes"]) - 1
    tot = i["z0"] + sum(_bilinear(i[f"z{l}"], size) for l in range(1, nl + 1))
    s = i["z0"].abs() + sum(_bilinear(i[f"z{l}"].abs(), size) for l in range(1, nl + 1))
    return nhwc(F.relu(tot * sc + sh)), nhwc(bound(4 * nl, s * sc.abs() + sh.abs()))


# ------------------------------------------------------------------------------------------------ layernorm_rows
def ln_variant(C):
    """(NV, RPW) of the layernorm_rows_kernel instantiation the launcher selects for C channels."""
    return (1, 2) if C <= 128 else (1, 1) if C <= 256 else (2, 1) if C <= 512 else (4, 1) if C <= 1024 else (8, 1) if C <= 2048 else (16, 1)


def ln_out_shape(p):
    rows, C, gr = p["rows"], p["C"], p.get("group_rows", 0)
    if p.get("patchify"):
        return rows // 4, 4 * C
    return (gr if gr and p.get("wrap") else rows), C + ((rows // gr - 1) * p.get("gcol", 0) if gr else 0)


def ln_place(t, p):
    """Where row `row` of the [rows, C] result goes: patchify sends token (b, h, w) to row (b, h/2, w/2), column block (h&1)*2 + (w&1); group
    g = row / group_rows writes at column g * y_gcol, and at row % group_rows when wrapping."""
    rows, C = t.shape
    r = torch.arange(rows)
    gr = p.get("group_rows", 0)
    g = r // gr if gr else torch.zeros_like(r)
    orow = r - g * gr if gr and p.get("wrap") else r
    ocol = g * p.get("gcol", 0)
    if p.get("patchify"):
        H, W = p["patchify"]
        w_, h_, b_ = r % W, (r // W) % H, r // (W * H)
        orow = (b_ * (H // 2) + h_ // 2) * (W // 2) + w_ // 2
        ocol = ocol + ((h_ & 1) * 2 + (w_ & 1)) * C
    out = t.new_zeros(ln_out_shape(p))
    out[orow[:, None], ocol[:, None] + torch.arange(C)[None, :]] = t
    return out


def make_layernorm_rows(p, g):
    rows, C = p["rows"], p["C"]
    G = rows // p["group_rows"] if p.get("group_rows") else 1
    x = torch.randn(rows, C, generator=g) * 3 + 1
    x[4::5] *= 100                                                                      # every fifth row: large magnitudes
    x[6::7] = 1.5 + 1e-3 * torch.randn(x[6::7].shape, generator=g)                      # every seventh: variance near eps, eps matters
    s = p.get("wscale", 1.0)                                                            # (clamp-watch cases: |y| beyond the fp16 formats' range)
    return dict(x=x, w=(torch.randn(G, C, generator=g) * 0.5 + 1) * s, b=torch.randn(G, C, generator=g) * 0.5 * s)


def ref_layernorm_rows(i, p, mut=None):
    """(y | y2) in the launch's output layout ([.., C] or [.., 2 C] with y2 next to y).  `mut`: a deliberately wrong restatement (the CPU companion)."""
    x, w, b = i["x"], i["w"], i["b"]
    rows, C = x.shape
    eps = float(torch.tensor(p["eps"], dtype=torch.float32))        # the launcher receives eps as fp32
    if mut == "eps":
        eps = 1e-5 if p["eps"] < 5e-6 else 1e-6
    gr = p.get("group_rows", 0)
    grp = torch.arange(rows) // gr if gr and mut != "group0" else torch.zeros(rows, dtype=torch.long)
    wg, bg = w[grp], b[grp]
    mu = x[:, :C - 4].sum(1, keepdim=True) / C if mut == "mean_drop4" else x.mean(1, keepdim=True)
    d = x - mu
    var = (d * d).sum(1, keepdim=True) / (C - 1 if mut == "var_cm1" else C)
    rho = 1 / torch.sqrt(var + eps)
    y = d * rho * wg + bg
    out = [ln_place(y, p)] + ([y + x] if p.get("y2") else [])
    if x.dtype != torch.float64 or mut:
        return torch.cat(out, 1), None
    nv, rpw = ln_variant(C)
    dp = 2 + (nv - 1) + (6 if rpw == 1 else 5)
    a = x.abs().mean(1, keepdim=True)
    dmu = (dp + 1) * U * a
    e = dmu + U * (d.abs() + dmu)
    dsig = (dp + 3) * U * var + 2 * (d.abs() * e).mean(1, keepdim=True)
    erho = dsig / (2 * (var + eps)) + 3 * U
    by = wg.abs() * rho * (e + d.abs() * (erho + 3 * U)) + 2 * U * ((wg * rho * d).abs() + bg.abs())
    bnd = [ln_place(by, p)] + ([by + U * (y + x).abs()] if p.get("y2") else [])
    return torch.cat(out, 1), torch.cat(bnd, 1)


# ------------------------------------------------------------------------------------------------ rowstats_finalize
def make_rowstats(p, g):
    """Strip sums (sum x, sum x^2 per 64-column strip): the float64 sums of drawn rows, rounded to fp32 -- kept as float64 tensors that hold fp32 values,
    because the device, like the reference, continues in double from them."""
    rows, strips = p["rows"], p["strips"]
    x = (torch.randn(rows, strips, 64, generator=g) * 2 + 0.5).double()
    if rows > 3:
        x[3] = 1.25                                                  # a constant row: the variance clamps to 0, rstd = 1 / sqrt(eps)
    return dict(rs=torch.stack([x.sum(2), (x * x).sum(2)], 2).float().double())


def ref_rowstats(i, p):
    """(mean, rstd) per row, [rows, 2]; double arithmetic on either side, one rounding to the working type."""
    rs, D = i["rs"].double(), 64 * p["strips"]
    eps = float(torch.tensor(p["eps"], dtype=torch.float32))
    s1, s2 = rs[..., 0].sum(1), rs[..., 1].sum(1)
    mean = s1 / D
    var = (s2 / D - mean * mean).clamp_min(0)
    rstd = 1 / torch.sqrt(var + eps)
    bnd = torch.stack([U * mean.abs(), rstd * (U + 2.0 ** -53 * (p["strips"] + 4) * (s2 / D) / (var + eps))], 1)
    return torch.stack([mean, rstd], 1).to(i["_dt"]), bnd


# ------------------------------------------------------------------------------------------------ deformable attention
NEAR = 2.0 ** -12


def msda_geometry(p):
    levels = p["levels"]
    starts = [sum(h * w for h, w in levels[:l]) for l in range(len(levels))]
    return levels, starts, sum(h * w for h, w in levels)


def _size(levels, dt=torch.float64):
    return torch.tensor([[w, h] for h, w in levels], dtype=dt).view(1, 1, 1, len(levels), 1, 2)     # (W, H): locations are (x, y)


def _off_integers(pix):
    """Pixel coordinates within 2^-12 of an integer (-1, H and W among them) move a quarter pixel away from it, to the side they lay on."""
    k = torch.round(pix)
    near = (pix - k).abs() < NEAR
    return torch.where(near, k + torch.where(pix >= k, 0.25, -0.25), pix), near


def _dyadic_pixels(levels, shape, g):
    """Exact pixel coordinates (x, y) per level that hit -1 (excluded), -0.5, 0, size - 1 (the upper taps are zero) and size (excluded), and a few
    dyadic interior points.  shape = [B, Lq, M, L, P]."""
    pix = torch.empty(*shape, 2, dtype=torch.float64)
    for l, (H, W) in enumerate(levels):
        for ax, n in ((0, W), (1, H)):
            cand = torch.tensor([-1.0, -0.5, 0.0, 0.25, 0.5, n - 1.5, n - 1.0, n - 0.5, float(n)], dtype=torch.float64)
            pix[:, :, :, l, :, ax] = cand[torch.randint(0, len(cand), pix[:, :, :, l, :, ax].shape, generator=g)]
    return pix


def _value(p, g, S):
    return torch.randn(p["B"], S, p["M"], p["D"], generator=g) * p.get("vscale", 1.0)


def make_msda(p, g):
    levels, _, S = msda_geometry(p)
    Bn, M, Lq, P, L = p["B"], p["M"], p["Lq"], p["P"], len(levels)
    rnd = (lambda t: t.half().float()) if p.get("dtype") == "f16" else (lambda t: t.float())       # f16: the inputs are fp16 numbers as given
    size = _size(levels)
    if p.get("dyadic"):
        loc = rnd((_dyadic_pixels(levels, (Bn, Lq, M, L, P), g) + 0.5) / size)                    # power-of-two sizes: exact
        assert bool((loc.double() * size - 0.5 == (loc * size.float() - 0.5).double()).all())
    else:
        loc = rnd(torch.rand(Bn, Lq, M, L, P, 2, generator=g) * 1.2 - 0.1)                         # roughly a quarter of the samples leave the map
        for _ in range(8):
            pix, near = _off_integers(loc.double() * size - 0.5)
            if not bool(near.any()):
                break
            loc = rnd((pix + 0.5) / size)
        assert not bool(near.any())
    aw = torch.softmax(torch.randn(Bn, Lq, M, L * P, generator=g), -1).view(Bn, Lq, M, L, P)
    return dict(value=rnd(_value(p, g, S)), loc=loc, aw=rnd(aw))


def _gather(value, levels, starts, loc, wgt, mut=None):
    """out[b, q, m, :] = sum_{l, p} wgt * bilinear(value_l at loc) as [B, Lq, M, D], with S1 and the per-sample tap sums T [B, Lq, M, L, P, D]."""
    Bn, S, M, D = value.shape
    Lq, L, P = loc.shape[1], loc.shape[3], loc.shape[4]
    if mut == "start":                                       # the second level's start index one row too late
        starts = [s + (levels[1][1] if l >= 1 else 0) for l, s in enumerate(starts)]
        value = torch.cat([value, value.new_zeros(Bn, levels[1][1], M, D)], 1)
    out = value.new_zeros(Bn, Lq, M, D)
    s1 = value.new_zeros(Bn, Lq, M, D)
    T = value.new_zeros(Bn, Lq, M, L, P, D)
    for l, (H, W) in enumerate(levels):
        vl = value[:, starts[l]:starts[l] + H * W].permute(0, 2, 1, 3)                             # [B, M, HW, D]
        sx, sy = (H, W) if mut == "swap" else (W, H)
        half = 0.0 if mut == "nohalf" else 0.5
        x, y = loc[:, :, :, l, :, 0] * sx - half, loc[:, :, :, l, :, 1] * sy - half                 # [B, Lq, M, P]
        inside = (y > -1) & (x > -1) & (y < H) & (x < W)
        y0, x0 = torch.floor(y), torch.floor(x)
        ly, lx = y - y0, x - x0
        a = wgt[:, :, :, l, :]
        for dy, dx, cw in ((0, 0, (1 - ly) * (1 - lx)), (0, 1, (1 - ly) * lx), (1, 0, ly * (1 - lx)), (1, 1, ly * lx)):
            yy, xx = y0 + dy, x0 + dx
            ok = inside & (yy >= 0) & (yy <= H - 1) & (xx >= 0) & (xx <= W - 1)
            idx = (yy.clamp(0, H - 1) * W + xx.clamp(0, W - 1)).long().permute(0, 2, 1, 3).reshape(Bn, M, Lq * P, 1)
            v = torch.gather(vl, 2, idx.expand(Bn, M, Lq * P, D)).view(Bn, M, Lq, P, D).permute(0, 2, 1, 3, 4) * ok[..., None]
            out = out + ((a * cw)[..., None] * v).sum(3)
            s1 = s1 + ((a.abs() * cw.abs())[..., None] * v.abs()).sum(3)
            T[:, :, :, l] += v.abs()
    return out, s1, T


def _msda_u(p):
    return 2.0 ** -53 if p.get("dtype") == "f64" else U


def ref_msda(i, p, mut=None):
    levels, starts, _ = msda_geometry(p)
    value, loc, aw = i["value"], i["loc"], i["aw"]
    if p.get("dtype") == "f64":                              # the device computes this case in double: so does its plain torch statement
        value, loc, aw = value.double(), loc.double(), aw.double()
    Bn, Lq, M, D = p["B"], p["Lq"], p["M"], p["D"]
    out, s1, T = _gather(value, levels, starts, loc, aw, mut)
    r = out.reshape(Bn * Lq, M * D)
    if i["_dt"] != torch.float64 or mut:
        return r, None
    u = _msda_u(p)
    pos = 0.0
    if not p.get("dyadic"):
        e = (2 * u * ((loc * _size(levels)).abs() + 0.5)).sum(-1)                                   # eps_w + eps_h, [B, Lq, M, L, P]
        pos = ((aw.abs() * e)[..., None] * T).sum((3, 4))
    bnd = ((len(levels) * p["P"] + 12) * u * s1 + pos).reshape(Bn * Lq, M * D)
    if p.get("dtype") == "f16":
        bnd = bnd + 2.0 ** -11 * r.abs() + 2.0 ** -24
    return r, bnd


def make_msda_bwd(p, g):
    """make_msda's value, loc and aw (the same draws) and a grad_output of O(1), [B, Lq, M, D]."""
    i = make_msda(p, g)
    gout = torch.randn(p["B"], p["Lq"], p["M"], p["D"], generator=g)
    i["gout"] = gout.half().float() if p.get("dtype") == "f16" else gout
    return i


def msda_bwd_shfl(p):
    """The launcher's choice: the xor-shuffle tree when D is a power of two <= 64, atomics into zeroed buffers for any other D."""
    return p["D"] <= 64 and p["D"] & (p["D"] - 1) == 0


def msda_bwd_slices(p):
    """Where (grad_value [B, S, M, D] | grad_sampling_loc [B, Lq, M, L, P, 2] | grad_attn_weight [B, Lq, M, L, P]) lie in the flat result."""
    _, _, S = msda_geometry(p)
    ns = p["B"] * p["Lq"] * p["M"] * len(p["levels"]) * p["P"]
    nv = p["B"] * S * p["M"] * p["D"]
    return {"gvalue": slice(0, nv), "gloc": slice(nv, nv + 2 * ns), "gaw": slice(nv + 2 * ns, nv + 3 * ns)}


def ref_msda_bwd(i, p, mut=None):
    """The three gradients, flattened and concatenated (msda_bwd_slices).  `mut`: swapWH (W and H exchanged in the scale of grad_sampling_loc), noaw
    (grad_sampling_loc without the attention weight), awaw (grad_attn_weight times the attention weight), dhsign (the sign of the first tap's dh
    flipped), start (the second level's start index one row too late)."""
    levels, starts, S = msda_geometry(p)
    value, loc, aw, g = i["value"], i["loc"], i["aw"], i["gout"]
    if p.get("dtype") == "f64":                              # the device computes this case in double: so does its plain torch statement
        value, loc, aw, g = value.double(), loc.double(), aw.double(), g.double()
    dt = value.dtype
    Bn, M, D, Lq, P, L = p["B"], p["M"], p["D"], p["Lq"], p["P"], len(levels)
    want = i["_dt"] == torch.float64 and not mut
    Sx = S
    if mut == "start":
        starts = [s + (levels[1][1] if l >= 1 else 0) for l, s in enumerate(starts)]
        Sx = S + levels[1][1]
        value = torch.cat([value, value.new_zeros(Bn, levels[1][1], M, D)], 1)
    vbm = value.permute(0, 2, 1, 3).reshape(Bn * M * Sx, D)                                       # rows (b, m, s)
    bm = (torch.arange(Bn).view(Bn, 1, 1, 1) * M + torch.arange(M).view(1, 1, M, 1)) * Sx
    u = _msda_u(p)
    gv = value.new_zeros(Bn * M * Sx, D)
    gl = value.new_zeros(Bn, Lq, M, L, P, 2)
    ga = value.new_zeros(Bn, Lq, M, L, P)
    n_v, s_v, pos_v = value.new_zeros(Bn * M * Sx), torch.zeros_like(gv), torch.zeros_like(gv)
    s_l, pos_l, s_a, pos_a = torch.zeros_like(gl), torch.zeros_like(gl), torch.zeros_like(ga), torch.zeros_like(ga)
    ins = torch.zeros(Bn, Lq, M, L, P, dtype=torch.bool)
    gq = g[:, :, :, None, :]                                                                      # [B, Lq, M, 1, D]
    for l, (H, W) in enumerate(levels):
        x, y = loc[:, :, :, l, :, 0] * W - 0.5, loc[:, :, :, l, :, 1] * H - 0.5                    # [B, Lq, M, P]
        inside = (y > -1) & (x > -1) & (y < H) & (x < W)
        ins[:, :, :, l] = inside
        y0, x0 = torch.floor(y), torch.floor(x)
        lh, lw = y - y0, x - x0
        hh, hw = 1 - lh, 1 - lw
        a = aw[:, :, :, l, :]
        ag = a[..., None] * gq                                                                    # [B, Lq, M, P, D]
        if p.get("dyadic"):
            e_h = e_w = torch.zeros_like(x)
        else:
            e_h, e_w = 2 * u * ((loc[:, :, :, l, :, 1] * H).abs() + 0.5) + 2 * u, 2 * u * ((loc[:, :, :, l, :, 0] * W).abs() + 0.5) + 2 * u
        val, dh, dw = (value.new_zeros(Bn, Lq, M, P, D) for _ in range(3))
        sval, sdh, sdw, T = (value.new_zeros(Bn, Lq, M, P, D) for _ in range(4))
        for dy, dx in ((0, 0), (0, 1), (1, 0), (1, 1)):
            wy, wx = (lh if dy else hh), (lw if dx else hw)
            cw = wy * wx
            yy, xx = y0 + dy, x0 + dx
            ok = inside & (yy >= 0) & (yy <= H - 1) & (xx >= 0) & (xx <= W - 1)
            okf = ok.to(dt)
            row = (bm + starts[l] + (yy.clamp(0, H - 1) * W + xx.clamp(0, W - 1)).long()).flatten()
            v = vbm[row].view(Bn, Lq, M, P, D) * okf[..., None]
            val = val + cw[..., None] * v
            dh = dh + (-1 if (dy == 0) != (mut == "dhsign" and (dy, dx) == (0, 0)) else 1) * wx[..., None] * v
            dw = dw + (1 if dx else -1) * wy[..., None] * v
            gv.index_add_(0, row, ((cw * okf)[..., None] * ag).reshape(-1, D))
            if want:
                n_v.index_add_(0, row, okf.flatten())
                s_v.index_add_(0, row, ((cw * okf)[..., None] * ag.abs()).reshape(-1, D))
                pos_v.index_add_(0, row, ((okf * (e_h + e_w))[..., None] * ag.abs()).reshape(-1, D))
                sval, sdh, sdw, T = sval + cw[..., None] * v.abs(), sdh + wx[..., None] * v.abs(), sdw + wy[..., None] * v.abs(), T + v.abs()
        ga[:, :, :, l] = (gq * val).sum(-1) * (a if mut == "awaw" else 1)
        sx, sy = (H, W) if mut == "swapWH" else (W, H)
        al = 1 if mut == "noaw" else a
        gl[:, :, :, l, :, 0] = (gq * dw).sum(-1) * al * sx
        gl[:, :, :, l, :, 1] = (gq * dh).sum(-1) * al * sy
        if want:
            gT = (gq.abs() * T).sum(-1)
            s_a[:, :, :, l], pos_a[:, :, :, l] = (gq.abs() * sval).sum(-1), (e_h + e_w) * gT
            s_l[:, :, :, l, :, 0], pos_l[:, :, :, l, :, 0] = W * a.abs() * (gq.abs() * sdw).sum(-1), W * a.abs() * e_h * gT
            s_l[:, :, :, l, :, 1], pos_l[:, :, :, l, :, 1] = H * a.abs() * (gq.abs() * sdh).sum(-1), H * a.abs() * e_w * gT

    def v_layout(t):
        return t.view(Bn, M, Sx, -1)[:, :, :S].permute(0, 2, 1, 3).expand(Bn, S, M, D).reshape(-1)
    r = torch.cat([v_layout(gv), gl.reshape(-1), ga.reshape(-1)])
    if not want:
        return r, None
    n_v = v_layout(n_v)
    b_v = (n_v + 4) * u * v_layout(s_v) + v_layout(pos_v)
    b_l, b_a = ((D + 8) * u * s + pos for s, pos in ((s_l, pos_l), (s_a, pos_a)))
    if p.get("dtype") == "f16":
        h, sub = 2.0 ** -11, 2.0 ** -14 + 2.0 ** -24

        def atomics16(b32, s, n):
            return b32 + ((1 + h) ** n - 1) * (s + b32) + n * sub
        b_v = atomics16(b_v, v_layout(s_v), n_v)
        if msda_bwd_shfl(p):
            b_l = b_l + h * gl.abs() + 2.0 ** -24 * ins[..., None]
            b_a = b_a + h * ga.abs() + 2.0 ** -24 * ins
        else:
            b_l, b_a = atomics16(b_l, s_l, D * ins[..., None].to(dt)), atomics16(b_a, s_a, D * ins.to(dt))
    return r, torch.cat([b_v, b_l.reshape(-1), b_a.reshape(-1)])


def h8_exact(t, g):
    """(h, h + l / 2048): values the h8 planes hold exactly.  h is an fp16 number (|h| >= 2^-4), l an e5m2 number of h's sign with |l| < 2^e (2^e <= |h|):
    |l / 2048| stays below half an ulp of h, so fp16 rounding returns h and the remainder is l / 2048 exactly; the sum spans 15 bits: exact in fp32."""
    h = t.half().float()
    h = torch.where(h.abs() < 2.0 ** -4, torch.where(h < 0, -(2.0 ** -4), 2.0 ** -4), h)
    e = torch.floor(torch.log2(h.abs().double())).float()
    k = torch.randint(0, 5, h.shape, generator=g).float()
    l = torch.where(k == 0, torch.zeros_like(h), torch.sign(h) * (1 + (k - 1) / 4) * torch.exp2(e - 1))
    v = h + l / 2048
    assert bool((v.double() == h.double() + l.double() / 2048).all()) and bool((v.half().float() == h).all())
    return h, v


def make_msda_fused(p, g):
    levels, _, S = msda_geometry(p)
    Bn, M, D, Lq, P, L = p["B"], p["M"], p["D"], p["Lq"], p["P"], len(levels)
    size = _size(levels)
    if p.get("dyadic"):
        ref = torch.randint(0, 9, (Lq, 2), generator=g).double() / 8
        off = _dyadic_pixels(levels, (Bn, Lq, M, L, P), g) + 0.5 - ref.view(1, Lq, 1, 1, 1, 2) * size   # exact: power-of-two sizes, ref in eighths
        assert bool((off.float().double() == off).all())
        off = off.float()
    else:
        ref = torch.rand(Lq, 2, generator=g).double()
        rr = ref.view(1, Lq, 1, 1, 1, 2)
        off = (((torch.rand(Bn, Lq, M, L, P, 2, generator=g) * 1.2 - 0.1).double() - rr) * size).float()   # loc uniform over [-0.1, 1.1]
        for _ in range(8):
            pix, near = _off_integers((ref.float().double().view(1, Lq, 1, 1, 1, 2) + off.double() / size) * size - 0.5)
            if not bool(near.any()):
                break
            off = (pix + 0.5 - ref.float().double().view(1, Lq, 1, 1, 1, 2) * size).float()
        assert not bool(near.any())
    logit = torch.randn(Bn, Lq, M, L * P, generator=g) * 2
    raw = torch.cat([off.reshape(Bn * Lq, M * L * P * 2), logit.reshape(Bn * Lq, M * L * P)], 1)
    i = dict(raw=raw, ref=ref.float())
    v = _value(p, g, S) * 3
    if p.get("value") == "h8":
        i["vhi"], i["value"] = (t.reshape(Bn * S, M * D) for t in h8_exact(v, g))
    else:
        i["value"] = v.reshape(Bn * S, M * D)
    return i


def ref_msda_fused(i, p, mut=None, parts=False):
    """parts: (r, the derived part of the bound, S1) -- what EXPF_EXCESS (top of the module) is measured with: max over the elements of
    (|y - r| - derived) / S1."""
    levels, starts, S = msda_geometry(p)
    Bn, M, D, Lq, P, L = p["B"], p["M"], p["D"], p["Lq"], p["P"], len(levels)
    LP = L * P
    raw, ref = i["raw"], i["ref"]
    dt = raw.dtype
    off = raw[:, :M * LP * 2].reshape(Bn, Lq, M, L, P, 2)
    logit = raw[:, M * LP * 2:].reshape(Bn, Lq, M, LP)
    wgt = (torch.softmax(logit.view(Bn, Lq, M, L, P), -1) if mut == "softmaxP" else torch.softmax(logit, -1).view(Bn, Lq, M, L, P))
    size = _size(levels, dt)
    rr = ref.view(1, Lq, 1, 1, 1, 2)
    loc = rr + off / size
    planes = p.get("value") == "h8"
    value = (i["vhi"] if planes and not p.get("lo_bytes") else i["value"]).view(Bn, S, M, D)
    out, s1, T = _gather(value, levels, starts, loc, wgt, mut)
    r = out.reshape(Bn * Lq, M * D)
    if dt != torch.float64 or mut:
        return r, None
    pos = 0.0
    if not p.get("dyadic"):
        e = (4 * U * ((rr * size).abs() + off.abs() + 0.5)).sum(-1)
        pos = ((wgt * e)[..., None] * T).sum((3, 4))
    n = LP * ((8 if p.get("lo_bytes") else 4) if planes else 1)
    wrel = (LP + 6 + (logit - logit.amax(-1, keepdim=True)).abs().amax(-1)) * U                      # [B, Lq, M]
    derived = ((n + 12) * U * s1 + wrel[..., None] * s1 + pos).reshape(Bn * Lq, M * D)
    s1 = s1.reshape(Bn * Lq, M * D)
    if parts:
        return r, derived, s1
    return r, derived + 2 * EXPF_EXCESS * s1


OPS = {
    "layernorm_rows": (make_layernorm_rows, ref_layernorm_rows), "rowstats": (make_rowstats, ref_rowstats), "msda": (make_msda, ref_msda),
    "msda_fused": (make_msda_fused, ref_msda_fused), "msda_bwd": (make_msda_bwd, ref_msda_bwd),
    "dwconv": (make_dwconv, ref_dwconv), "gconv": (make_gconv, ref_gconv), "gfe_qkv": (make_gfe_qkv, ref_gfe_qkv),
    "dwpair_gate": (make_dwpair_gate, ref_dwpair_gate), "ca_apply": (make_ca_apply, ref_ca_apply), "gelu_gate": (make_gelu_gate, ref_gelu_gate),
    "pool_hw": (make_pool_hw, ref_pool_hw), "colstats": (make_colstats, ref_colstats), "ffrm": (make_ffrm, ref_ffrm), "lnhw": (make_lnhw, ref_lnhw),
    "gram": (make_gram, ref_gram), "chanattn": (make_chanattn, ref_chanattn), "gffm": (make_gffm, ref_gffm), "tail": (make_tail, ref_tail),
    "nchw_to_planes": (make_nchw_to_planes, ref_nchw_to_planes), "tokens_to_nchw": (make_tokens_to_nchw, ref_tokens_to_nchw),
    "head_fuse": (make_head_fuse, ref_head_fuse),
}

_CACHE = {}


def case_data(case_id, op, p):
    """(fp32 inputs, float64 reference, bound) of a case: computed once, shared by the tests that need it, never written to."""
    if case_id not in _CACHE:
        make, ref = OPS[op]
        i = make(p, gen_for(case_id))
        r, bnd = ref(cast(i, torch.float64), p)
        _CACHE[case_id] = (i, r, bnd.double())
    return _CACHE[case_id]


def fp32_eval(op, i, p):
    """torch's own fp32 evaluation of the same statement."""
    return OPS[op][1](cast(i, torch.float32), p)[0]
