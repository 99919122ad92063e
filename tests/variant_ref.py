"""Float64 restatements of the conv / norm / neck / tail / head operations and the per-element bound the kernel-variant tests hold the
device to (tests/test_kernel_variants_gpu.py; tests/test_kernel_variants_cpu.py keeps the bound itself honest).

Every `ref_<op>(i, p)` takes the case's inputs `i` (a dict of CPU tensors, all of ONE floating dtype) and its parameters `p` and returns
(r, bnd) in the layout the device writes: evaluated on float64 inputs, r is the reference and bnd the bound; evaluated on the float32 inputs
it is torch's own fp32 evaluation of the same operation (bnd is then ignored).

The bound.  A result formed as a sum of n products with magnitude sum s = sum |x_i| |w_i| + |bias| passes when, element by element,
    |y - r| <= (n + 4) * 2^-24 * s + a
-- the standard fp32 accumulation bound (n + 4 roundings of relative size 2^-24 on every path through the sum) plus the activation's own absolute
error a, scaled by whatever multiplies the activation.  Nothing measured goes into the first term."""
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
assert max(ACT_ABS.values()) <= 1e-6   # a larger allowance would be a finding about the kernel, not a tolerance
# rounding of the operand formats themselves (relative to |r|), where only planes can be compared: bf16 hi/lo, fp16 hi/lo, fp16 hi + e5m2 lo
FMT_REL = {"b3": 2.0 ** -16, "f3": 2.0 ** -22, "h8": 2.0 ** -14}
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


OPS = {
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
