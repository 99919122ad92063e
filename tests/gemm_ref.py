"""Float64 restatements of the GEMM family (csrc/gemm_split3.hip, gemm_v2.hip, gemm_h8c*.hip, gemm_stream.hip, mlp_fused.hip), the operand planes as
torch casts build them, and the per-element bound tests/test_gemm_variants_gpu.py holds the device to (tests/test_gemm_variants_cpu.py keeps the bound
itself honest).  Runs on the CPU; does not import mmsa.

Operands.  `split(x, fmt)` restates csrc/common.h with torch casts, `planes_words` lays the parts out as the int16 tensor behind ops.Planes:
    b3    hi = bf16(x), lo = bf16(x - hi)                                   (round to nearest even; x - hi is exact in fp32)
    f3    x clamped to +-65504; hi = fp16(x), lo = fp16(x - hi)
    h8    x clamped to +-57344; hi = fp16(x); the planes also hold ql = e5m2((x - hi) 2^11) and qh = e5m2(hi)
    h8c   as h8 with ql = e5m2((x - hi) 2^11 1.09375) (one fp32 product) and qh = the fp16 hi value's top byte (truncation), taken in registers
    w8    W = 2^e_n e4m3(code): exact in fp16; qw = the fp16 value's top byte
The reference of a case is the float64 sum of exactly the products the kernel forms from those parts -- not the float64 product of the fp32 inputs,
whose distance from it is the format's own error and no kernel fault:
    b3, f3 (planes, or an fp32 A that gemm_split3_kernel<false, ..> splits while it stages it)   sum_k a_hi w_hi + a_hi w_lo + a_lo w_hi      n = 3 K
    h8, h8c                                  sum_k a_hi w_hi + (qh_a ql_w + ql_a qh_w) / 2^11                                               n = 3 K
    w8   (csrc/gemm_h8c_w8.hip)              sum_k a_hi w + ql_a qw / 2^11                                                                   n = 2 K
    gemm_tiny_kernel                         sum_k a (w_hi + w_lo): fp32 FMAs on the fp32 A; the weight sum is exact in fp32 (16 bits)          n = K
(the lo.lo term is dropped, as in the kernels; the block scale of the fp8 MFMA undoes the 2^11 exactly).

The bound, element by element; u = 2^-24, s_p = the sum of the absolute values of the same products.
    accumulator      n exact products (8 x 8, 11 x 11 or 3 x 3 significant bits: exact in fp32) meet in an fp32 sum of unknown order: at most n - 1 roundings
                     on any path, (n + 4) u s with s = s_p + |bias| covers them and the few below; MFMA_EXCESS s_p on top (see the constant)
    bias add         pre = acc + bias: one rounding, u |pre|
    row-normalising  pre = fma(rstd, fma(-mean, colsum, acc), bias): s = s_p + |mean colsum|; the inner rounding is inside the + 4, the accumulator error is
                     scaled by |rstd|, the outer rounding is u |pre| <= u (|rstd| s + |bias|):      |rstd| ((n + 4) u s + MFMA_EXCESS s_p) + u (|rstd| s + |bias|)
    activation       y = act(pre): L_act bnd_pre + the activation's own error.  L: 1 for relu / relu6 (exact operations), 1/4 for sigmoid; gelu'(x) = Phi(x) +
                     x phi(x) peaks at x = sqrt 2: 0.92135 + 0.20755 = 1.1289 -> 1.13; hswish'(x) = (2 x + 3) / 6 on (-3, 3), 1 beyond: 1.5.
                     Own error: gelu GELU_ABS (the fp32 evaluation of common.h's polynomial, absolute); hswish x * (clamp(x + 3) / 6): the addition moves the
                     clamp's argument by u (|x| + 3), i.e. the result by u (|x| + 3) |x| / 6, the division and the product are 2 u |y|; sigmoid 1 / (1 + expf(-x)):
                     the addition and the division are 2 u |y|, a one-ulp expf another u |y| -- plus, for both, the measured excess of variant_ref.ACT_ABS
    scale            cv = colscale * alpha is one rounded product, y * cv another: |cv| bnd + 2 u |y cv|
    residual         beta * resid and the addition (or one fma): u |beta resid| + u |result|
    planes only      + FMT_REL[fmt] |r| (added by the test, as for every planes-only output)
A case marked `exact` (every K > 128) has operands on a grid: integer hi parts, lo parts of +-2^-9 (b3) / +-2^-12 (the fp16 formats) or 0, which the planes
hold exactly (make_gemm asserts it), bias and residual on the grid of the products.  While sum |terms| + |bias| + |resid| < 2^24 x (grid step) every partial
sum in any order is exact in fp32, so the accumulator term is ZERO: with no activation or relu, no scale and beta = 1 the device must equal the float64
reference bit for bit; otherwise the epilogue terms above are all that is allowed.

mlp_fused (x <- x + gamma (gelu(A W1^T + b1) W2^T + b2), csrc/mlp_fused.hip).  h = gelu(pre) with bnd_h = 1.13 bnd_pre + GELU_ABS (bnd_pre as above, zero for
exact-grid A / W1 / b1).  The kernel splits its h' to planes in LDS and contracts (h_hi, h_lo) with (w_hi, w_lo) in three products; the reference is
sum_j h_j (w_hi + w_lo)_j on the float64 h.  Between the two: h' - h (bnd_h), the rounding of the split (FMT_REL |h|), the dropped h_lo w_lo (|h_lo| <=
HI_REL |h|: 2^-9 for bf16, 2^-12 for fp16 hi parts), and the accumulation of n = 3 * 4C products:
    bnd_acc = sum_j (|w_hi| + |w_lo|)_j (bnd_h + FMT_REL |h|)_j + HI_REL sum_j |h_j| |w_lo,j| + (12 C + 4) u (1 + 2^-8) sum_j |h_j| (|w_hi| + |w_lo|)_j
    out = x + gamma (acc + b2): |gamma| (bnd_acc + u |acc + b2|) + u |gamma (acc + b2)| + u |out|"""
import torch

from tests.variant_ref import ACT_ABS, FMT_REL, GELU_ABS, U, act_fn, gen_for, violations  # noqa: F401  (re-exported for the tests)

# What the matrix pipe adds to the derived accumulator term (its internal alignment / rounding of a 32-term dot product is stated in no source here),
# relative to s_p.  Measured on an MI355X against the float64 reference over every case of the table: none.  No case leaves the derived bound -- a random-data
# fp32 output of the MFMA kernels stays at 0.018 of it at most (h8c-rs-ragged-m257n192k64) -- and every exact-grid case with a linear epilogue equals the
# reference bit for bit, in all five operand formats, K up to 384.  Nothing is allowed (profiles/README.md, "Kernel variants of the GEMM sources").
MFMA_EXCESS = 0.0
assert MFMA_EXCESS == 0.0 or MFMA_EXCESS <= 4 * U      # above 1 x the derived term of the shallowest case (n + 4 >= 36) it would be a finding, not a tolerance
HI_REL = {"b3": 2.0 ** -9, "f3": 2.0 ** -12}
LIP = {"none": 1.0, "relu": 1.0, "relu6": 1.0, "sigmoid": 0.25, "gelu": 1.13, "hswish": 1.5}
H8C_LO_COMP = 1.09375
POISON = 30000.0      # what the rows / columns a launch must not read are filled with (finite in every format)


# ------------------------------------------------------------------------------------------------ operands
def _e5m2(t):
    return t.to(torch.float8_e5m2)


def _top_byte(h16):
    return (h16.view(torch.int16) & -256).view(torch.float16).float()


def split(x, fmt):
    """The parts the planes of `fmt` hold of the fp32 matrix x (fp32 tensors; *8: the e5m2 bytes)."""
    x = x.float()
    if fmt == "b3":
        hi = x.to(torch.bfloat16).float()
        return dict(fmt=fmt, hi=hi, lo=(x - hi).to(torch.bfloat16).float())
    if fmt == "f3":
        x = x.clamp(-65504.0, 65504.0)
        hi = x.half().float()
        return dict(fmt=fmt, hi=hi, lo=(x - hi).half().float())
    x = x.clamp(-57344.0, 57344.0)
    h = x.half()
    hi = h.float()
    ql8 = _e5m2((x - hi) * (2048.0 * H8C_LO_COMP if fmt == "h8c" else 2048.0))
    qh8 = _e5m2(hi)
    return dict(fmt=fmt, hi=hi, ql8=ql8, ql=ql8.float(), qh8=qh8, qh=_top_byte(h) if fmt == "h8c" else qh8.float())


def value(o):
    """The fp32 value the planes stand for (what ops.planes_to_float decodes)."""
    if o["fmt"] in ("b3", "f3"):
        return o["hi"] + o["lo"]
    return o["hi"] + o["ql"] / (2048.0 * H8C_LO_COMP if o["fmt"] == "h8c" else 2048.0)


def w8_quantize(w):
    """[N, K] -> the W8 weight 2^e_n e4m3(code) nearest to it (e_n: the smallest exponent in [-15, 7] with max_k |w| <= 448 2^e_n), as fp32: exact in fp16."""
    amax = w.double().abs().amax(1).clamp_min(2.0 ** -30)
    e = torch.ceil(torch.log2(amax / 448.0)).clamp(-15, 7)
    sc = torch.exp2(e)[:, None]
    q = (w.double() / sc).float().to(torch.float8_e4m3fn).float().double() * sc
    q = q + 0.0      # (no negative zeros: a code's sign bit is set for non-zero values only)
    assert bool((q.float().half().double() == q).all())
    return q.float()


def split_w8(w):
    assert bool((w8_quantize(w) == w).all()), "not a W8 weight"
    return dict(fmt="w8", w=w.float(), qw=_top_byte(w.half()))


def pad32(k):
    return (k + 31) // 32 * 32


def pad64(k):
    return (k + 63) // 64 * 64


def _pad_cols(t, kp):
    return torch.cat([t, t.new_zeros(t.shape[0], kp - t.shape[1])], 1) if kp > t.shape[1] else t


def _bits16(t, fmt):
    return (t.view(torch.int32) >> 16).to(torch.int16) if fmt == "b3" else t.half().view(torch.int16)


def planes_words(o, kpad=None, weight=False):
    """The int16 tensor behind ops.Planes of the operand `o` (csrc/common.h): [rows, 2 kpad]; h8c: [ceil(rows / 2), 3 kpad] by row pairs, zero where nothing is stored."""
    fmt = o["fmt"]
    rows, k = o["hi"].shape
    kp = kpad or (pad64(k) if fmt == "h8c" else pad32(k))
    if fmt in ("b3", "f3"):       # per 32-wide k-block: the 32 hi values, then the 32 lo values
        hi, lo = (_pad_cols(_bits16(o[n], fmt), kp).view(rows, kp // 32, 1, 32) for n in ("hi", "lo"))
        return torch.cat([hi, lo], 2).reshape(rows, 2 * kp)
    hi = _pad_cols(o["hi"].half().view(torch.int16), kp)
    ql, qh = (_pad_cols(o[n].view(torch.uint8), kp) for n in ("ql8", "qh8"))
    if fmt == "h8":               # per k-block 128 bytes: 32 fp16 hi, then four 16-byte chunks g: (8 lo | 8 q(hi)) bytes of k = 8g .. 8g+7; weights: (q(hi) | lo)
        hb = hi.view(rows, kp // 32, 32).contiguous().view(torch.uint8).view(rows, kp // 32, 64)
        pair = (qh, ql) if weight else (ql, qh)
        ch = torch.stack([t.view(rows, kp // 32, 4, 8) for t in pair], 3).reshape(rows, kp // 32, 64)
        return torch.cat([hb, ch], 2).reshape(rows, kp * 4).contiguous().view(torch.int16).view(rows, 2 * kp)
    # h8c: pair j = [row 2j: kp fp16][row 2j+1: kp fp16][kp / 64 lines of 128 lo bytes: row 2j's 64 | row 2j+1's 64; a row's 64 = 4 groups g of (k = 64c + 8g .. +7 | k = 64c + 32 + 8g .. +7)]
    pr = (rows + 1) // 2
    hi2 = torch.zeros(2 * pr, kp, dtype=torch.int16)
    hi2[:rows] = hi
    ql2 = torch.zeros(2 * pr, kp, dtype=torch.uint8)
    ql2[:rows] = ql
    lo = ql2.view(pr, 2, kp // 64, 2, 4, 8).permute(0, 2, 1, 4, 3, 5).reshape(pr, 2 * kp)      # [pair, row, chunk, t, g, e] -> [pair, chunk, row, g, t, e]
    return torch.cat([hi2.view(pr, 2 * kp), lo.contiguous().view(torch.int16)], 1)


def _h8_emulated_product(a, w):
    """What the h8 kernels compute, restated with torch casts: hi.hi exactly + the two cross terms with e5m2-rounded operands (tests/test_planes_gpu.py)."""
    ah = a.clamp(-57344, 57344).half().float()
    wh = w.clamp(-57344, 57344).half().float()
    al, wl = (a - ah) * 2048, (w - wh) * 2048
    q = lambda t: t.to(torch.float8_e5m2).float()
    return ah.double() @ wh.double().t() + (q(ah).double() @ q(wl).double().t() + q(al).double() @ q(wh).double().t()) / 2048


def _h8c_emulated_product(a, w):
    """hi.hi exactly + the two cross terms with q(hi) = the fp16 hi value truncated to its top byte (an e5m2) and lo rounded to e5m2 after the
    scaling by 2^11 x 1.09375 that makes up for the truncation's mean (csrc/common.h MMSA_H8C_LO_COMP; the MFMA's block scale undoes the 2^11)."""
    ah = a.clamp(-57344, 57344).half()
    wh = w.clamp(-57344, 57344).half()
    al, wl = (a - ah.float()) * (2048 * H8C_LO_COMP), (w - wh.float()) * (2048 * H8C_LO_COMP)
    q = lambda t: t.to(torch.float8_e5m2).float()
    trunc = lambda h: (h.view(torch.int16) & -256).view(torch.float16).float()
    return ah.double() @ wh.double().t() + (trunc(ah).double() @ q(wl).double().t() + q(al).double() @ trunc(wh).double().t()) / 2048


# ------------------------------------------------------------------------------------------------ the contraction
def _terms(A, W, kind, mut=None):
    """[(a part, w part, scale)] of the products the kernel forms."""
    if kind == "tiny":
        wsum = W["hi"] + W["lo"]
        assert bool((wsum.double() == W["hi"].double() + W["lo"].double()).all()), "hi + lo of a bf16 pair is exact in fp32"
        return [(A, wsum, 1.0)]
    if kind in ("b3", "f3"):
        t = [(A["hi"], W["hi"], 1.0), (A["hi"], W["lo"], 1.0), (A["lo"], W["hi"], 1.0)]
        if mut == "lohi8":                      # the lo . hi term without the last 8 columns of K
            al = A["lo"].clone()
            al[:, -8:] = 0
            t[2] = (al, W["hi"], 1.0)
        return t
    if kind == "w8":
        return [(A["hi"], W["w"], 1.0), (A["ql"], W["w"] if mut == "w8_code" else W["qw"], 1.0 / 2048)]
    aq, wq = (A["qh"], W["qh"]) if mut != "h8c_round" else (A["qh8"].float(), W["qh8"].float())
    t = [(A["hi"], W["hi"], 1.0), (aq, W["ql"], 1.0 / 2048), (A["ql"], wq, 1.0 / 2048)]
    if mut == "lohi8":
        al = A["ql"].clone()
        al[:, -8:] = 0
        t[2] = (al, wq, 1.0 / 2048)
    return t


def contract(A, W, kind, dt, mut=None):
    """(sum of the products, sum of their absolute values, n) in dtype dt."""
    terms = _terms(A, W, kind, mut)
    r = s = 0.0
    for a, w, sc in terms:
        a = a.to(dt)
        if mut == "ktile128" and a.shape[0] > 128:      # rows >= 128 without their last k-tile
            a = a.clone()
            a[128:, -32:] = 0
        r = r + (a @ w.to(dt).t()) * sc
        s = s + (a.abs() @ w.to(dt).abs().t()) * sc
    return r, s, len(terms) * terms[0][0].shape[1]


def _act(act, x):
    """act(x) in x's dtype.  GELU in the fp32 evaluation is the correctly rounded value (float64, rounded once): torch's own fp32 erf form loses 1 + erf(x / sqrt 2) to
    cancellation for x < -3 (7.6e-7 absolute at x = -3.4), an error of that formula and not of the polynomial the kernels evaluate, which GELU_ABS describes."""
    return act_fn(act)(x.double()).to(x.dtype) if act == "gelu" else act_fn(act)(x)


def _act_own(act, x, y):
    if act == "gelu":
        return GELU_ABS
    if act == "hswish":
        return U * (x.abs() + 3) * x.abs() / 6 + 2 * U * y.abs() + ACT_ABS["hswish"]
    if act == "sigmoid":
        return 3 * U * y.abs() + ACT_ABS["sigmoid"]
    return 0.0


# ------------------------------------------------------------------------------------------------ inputs
def _grid(fmt):
    """(lo step of an exact-grid operand, grid step of its products)."""
    return (2.0 ** -9, 2.0 ** -9) if fmt == "b3" else (2.0 ** -12, 2.0 ** -16 if fmt == "w8" else 2.0 ** -12)


def _exact_operand(shape, fmt, g, hmax, lo=True):
    """hi + lo with hi an integer in [-hmax, hmax] and lo = +-step or 0 (0 where hi is 0): held exactly by planes of `fmt`."""
    hi = torch.randint(-hmax, hmax + 1, shape, generator=g).float()
    x = hi + (torch.randint(-1, 2, shape, generator=g).float() * _grid(fmt)[0] * (hi != 0) if lo else 0.0)
    return x


def _ramp(n):
    return ((torch.arange(n) % 61) - 30).float()


def make_gemm(p, g):
    """The case's fp32 inputs: a [B, M, K], w [Bw, N, K], bias / colscale / colsum [B, .], resid [B, rows, cols], mr [B, M, 2]."""
    B, M, N, K, fmt = p.get("batch", 1), p["M"], p["N"], p["K"], p["fmt"]
    kind = p.get("kind", fmt)
    ps = p.get("ps")
    rows, cols = (4 * M, ps[2]) if ps else (M, N)
    i = {}
    if p.get("exact"):
        step = _grid(fmt)[1]
        hmax = p.get("hmax", 4 if fmt == "b3" else 3 if K <= 384 else 1)
        i["a"] = _exact_operand((B, M, K), "b3" if kind == "tiny" else fmt, g, 1 if fmt == "w8" else hmax, lo=kind != "tiny")
        if fmt == "w8":      # e4m3 values with all three mantissa bits in use: the truncated top byte differs from the value
            mant = (8 + torch.randint(0, 8, (B, N, K), generator=g)).float() / 16 * torch.randint(1, 3, (B, N, K), generator=g).float() / 2
            i["w"] = mant * (torch.randint(0, 2, (B, N, K), generator=g).float() * 2 - 1)
            i["w"][:, :, 1] = 0.9375          # every row's largest value: e_n = -8 for every row; |w| = m / 32 or m / 16 (m = 8 .. 15), its top byte a multiple of 2^-4
        else:
            i["w"] = _exact_operand((B, N, K), fmt, g, hmax)
            i["w"][:, :, 0] = _ramp(N)[None]  # an asymmetric ramp: row / column swaps show
        i["a"][:, :, 0] = torch.where(i["a"][:, :, 0].abs() < 1, torch.ones(B, M), i["a"][:, :, 0])     # (its partner column never all zero)
        ongrid = lambda *s: torch.randint(-8, 9, s, generator=g).float() + torch.randint(-1, 2, s, generator=g).float() * step
        if p.get("bias", True):
            i["bias"] = ongrid(B, N)
        if p.get("resid"):
            i["resid"] = ongrid(B, p.get("resid_mod") or rows, cols)
    else:
        i["a"] = torch.randn(B, M, K, generator=g) * 1.3
        i["w"] = torch.randn(B, N, K, generator=g) / K ** 0.5
        if fmt == "w8":
            i["w"] = torch.stack([w8_quantize(w) for w in i["w"]])
        if p.get("bias", True):
            i["bias"] = torch.randn(B, N, generator=g)
        if p.get("resid"):
            i["resid"] = torch.randn(B, p.get("resid_mod") or rows, cols, generator=g)
    if p.get("colscale"):
        i["colscale"] = 0.5 + torch.rand(B, cols, generator=g)
    if p.get("rn"):
        i["mr"] = torch.stack([torch.randn(B, M, generator=g) * 0.2, 0.5 + torch.rand(B, M, generator=g)], 2).contiguous()
        i["colsum"] = torch.randn(B, N, generator=g)
    if p.get("exact"):      # the planes hold every value exactly: integer hi parts, the lo parts as drawn
        for b in range(B):
            A, W, _ = _operands(i, p, b)
            for o, x in ((A, i["a"][b]), (W, i["w"][b])):
                if not isinstance(o, dict) or o["fmt"] == "w8":
                    continue
                assert bool((o["hi"] == torch.round(x)).all()), "an exact-grid hi part is not the integer"
                assert bool(((o["lo"] if "lo" in o else o["ql"] / 2048) == x - o["hi"]).all()), "an exact-grid lo part is not held exactly"
    return i


def _operands(i, p, b):
    fmt, kind = p["fmt"], p.get("kind", p["fmt"])
    a, w = i["a"][b], i["w"][min(b, i["w"].shape[0] - 1)]
    A = a if kind == "tiny" else split(a, "h8c" if fmt == "w8" else fmt)
    W = split_w8(w) if fmt == "w8" else split(w, fmt)
    return A, W, kind


def exact_margin(i, p):
    """(largest sum |terms| + |bias| + |resid| over the elements, 2^24 x grid step) of an exact-grid case."""
    worst = 0.0
    for b in range(p.get("batch", 1)):
        A, W, kind = _operands(i, p, b)
        _, s, _ = contract(A, W, kind, torch.float64)
        worst = max(worst, float(s.max()) + (float(i["bias"].abs().max()) if "bias" in i else 0.0) + (float(i["resid"].abs().max()) if "resid" in i else 0.0))
    return worst, 2.0 ** 24 * _grid(p["fmt"])[1]


# ------------------------------------------------------------------------------------------------ gemm: product + epilogue
def dest_index(p, M, N, mut=None):
    """(destination row [M, N], destination column [M, N], residual row [M, N]) of out / out_planes = epilogue(a @ w^T)."""
    m = torch.arange(M)[:, None].expand(M, N)
    n = torch.arange(N)[None, :].expand(M, N)
    drow, dcol = m, n
    if p.get("ps"):      # 2 x 2 pixel-shuffle store: row (b, h, w), column (i, j, c) -> row (b, 2h + i, 2w + j), column c
        H, W, C = p["ps"]
        ij, dcol = n // C, n % C
        qi, qj = (ij & 1, ij >> 1) if mut == "ps_swap" else (ij >> 1, ij & 1)
        w_, h_, b_ = m % W, (m // W) % H, m // (W * H)
        drow = (b_ * 2 * H + 2 * h_ + qi) * (2 * W) + 2 * w_ + qj
    rmod = p.get("resid_mod", 0)
    rrow = ((m if mut == "rmod_src" else drow) % rmod) if rmod else drow
    return drow, dcol, rrow


def ref_gemm(i, p, dt=torch.float64, mut=None):
    """(r, bnd) as [B, rows, cols] in the launch's output layout; dt = float32: torch's own fp32 evaluation of the same statement (bnd None)."""
    B, M, N, K = p.get("batch", 1), p["M"], p["N"], p["K"]
    act, alpha, beta = p.get("act", "none"), p.get("alpha", 1.0), p.get("beta", 1.0)
    rows, cols = (4 * M, p["ps"][2]) if p.get("ps") else (M, N)
    drow, dcol, rrow = dest_index(p, M, N, mut)
    want_bnd = dt == torch.float64 and mut is None
    outs, bnds = [], []
    for b in range(B):
        A, W, kind = _operands(i, p, b)
        acc, s_p, n = contract(A, W, kind, dt, mut)
        bias = i["bias"][b].to(dt) if "bias" in i else torch.zeros(N, dtype=dt)
        if mut == "bias_col":
            bias = bias[torch.arange(N).clamp_max(N - 2)]
        if p.get("rn") and mut != "no_rn":
            mu, rs = i["mr"][b, :, 0:1].to(dt), i["mr"][b, :, 1:2].to(dt)
            cs = i["colsum"][0 if mut == "colsum_b0" else b].to(dt)
            pre = rs * (acc - mu * cs) + bias
            s = s_p + (mu * cs).abs()
            bnd = rs.abs() * ((n + 4) * U * s + MFMA_EXCESS * s_p) + U * (rs.abs() * s + bias.abs())
        else:
            pre = acc + bias
            bnd = (n + 4) * U * (s_p + bias.abs()) + MFMA_EXCESS * s_p + (U * pre.abs() if "bias" in i else 0.0)
        if p.get("exact"):
            bnd = torch.zeros_like(pre)
        y = _act(act, pre)
        bnd = LIP[act] * bnd + _act_own(act, pre, y)
        scaled = "colscale" in i or alpha != 1.0
        if scaled:
            cv = (i["colscale"][0 if mut == "colscale_b0" else b].to(dt)[dcol] if "colscale" in i else torch.ones((), dtype=dt)) * torch.tensor(alpha, dtype=torch.float32).to(dt)
            y = y * cv
            bnd = cv.abs() * bnd + 2 * U * y.abs()
        if "resid" in i:
            rr = torch.tensor(beta, dtype=torch.float32).to(dt) * i["resid"][b].to(dt)[rrow, dcol]
            y = y + rr
            if not (p.get("exact") and beta == 1.0 and not scaled and act in ("none", "relu")):
                bnd = bnd + U * rr.abs() + U * y.abs()
        o = torch.zeros(rows, cols, dtype=dt)
        o[drow, dcol] = y
        outs.append(o)
        if want_bnd:
            ob = torch.zeros(rows, cols, dtype=dt)
            ob[drow, dcol] = bnd + torch.zeros_like(y)
            bnds.append(ob)
    return torch.stack(outs), (torch.stack(bnds) if want_bnd else None)


# ------------------------------------------------------------------------------------------------ mlp_fused
def make_mlp(p, g):
    B, M, fmt, C = p.get("batch", 1), p["M"], p["fmt"], 96
    step = _grid(fmt)[1]
    ongrid = lambda *s: torch.randint(-4, 5, s, generator=g).float() / 2 + torch.randint(-1, 2, s, generator=g).float() * step
    i = dict(a=_exact_operand((B, M, C), fmt, g, 1), w1=_exact_operand((B, 4 * C, C), fmt, g, 1), b1=ongrid(B, 4 * C))      # |pre| of a few units: gelu's curved part
    i["w1"][:, :, 0] = (_ramp(4 * C) % 3)[None]
    i["w2"] = torch.randn(B, C, 4 * C, generator=g) / (4 * C) ** 0.5
    i["b2"], i["gamma"], i["x"] = torch.randn(B, C, generator=g), 0.5 + torch.rand(B, C, generator=g), torch.randn(B, M, C, generator=g)
    return i


def mlp_exact_margin(i, p):
    worst = 0.0
    for b in range(p.get("batch", 1)):
        _, s, _ = contract(split(i["a"][b], p["fmt"]), split(i["w1"][b], p["fmt"]), p["fmt"], torch.float64)
        worst = max(worst, float(s.max()) + float(i["b1"].abs().max()))
    return worst, 2.0 ** 24 * _grid(p["fmt"])[1]


def ref_mlp(i, p, dt=torch.float64, mut=None):
    B, fmt, C = p.get("batch", 1), p["fmt"], 96
    want_bnd = dt == torch.float64 and mut is None
    outs, bnds = [], []
    for b in range(B):
        pre, _, _ = contract(split(i["a"][b], fmt), split(i["w1"][b], fmt), fmt, dt)
        pre = pre + i["b1"][b].to(dt)
        h = _act("gelu", pre)
        W2 = split(i["w2"][b], fmt)
        w2 = W2["hi"].to(dt) + W2["lo"].to(dt)
        acc = h @ w2.t()
        gam, b2, x = i["gamma"][b].to(dt), i["b2"][b].to(dt), i["x"][b].to(dt)
        o = x + gam * acc + b2 if mut == "b2_outside" else x + gam * (acc + b2)
        outs.append(o)
        if want_bnd:
            w2abs = W2["hi"].double().abs() + W2["lo"].double().abs()
            bnd_h = GELU_ABS          # exact-grid A, W1, b1: the pre-activation is exact (mlp_exact_margin)
            bacc = (bnd_h + FMT_REL[fmt] * h.abs()) @ w2abs.t() + HI_REL[fmt] * (h.abs() @ W2["lo"].double().abs().t()) \
                + (12 * C + 4) * U * (1 + 2.0 ** -8) * (h.abs() @ w2abs.t())
            bnds.append(gam.abs() * (bacc + U * (acc + b2).abs()) + U * (gam * (acc + b2)).abs() + U * o.abs())
    return torch.stack(outs), (torch.stack(bnds) if want_bnd else None)


# ------------------------------------------------------------------------------------------------ split_planes
SPLIT_KINDS = (("b3", False), ("f3", False), ("h8", False), ("h8", True), ("h8c", False))      # mmsa_split_planes kinds 0, 4, 1, 2, 3


def make_split(rows, cols, g):
    x = torch.randn(rows, cols, generator=g) * 3
    sp = torch.tensor([0.0, 1e-6, -3e-5, 6.0e4, -7.0e4, 1.0e5, 57344.0, 65504.0, 1.0 + 2.0 ** -12, -(1.0 - 2.0 ** -12), 2.0 ** -14, 1000.3])
    flat = x.view(-1)
    n = min(flat.numel(), sp.numel())
    flat[torch.randperm(flat.numel(), generator=g)[:n]] = sp[:n]
    return x


# the kernel families of the table: every op name must have a case (tests/test_gemm_variants_cpu.py)
OPS = {name: (make_gemm, ref_gemm) for name in ("tiny", "split3", "v2_b3w8", "v2_b3w4", "v2_h8", "v2_f3", "h8c", "h8c4", "w8", "stream")}
OPS["mlp_fused"] = (make_mlp, ref_mlp)

_CACHE = {}


def case_data(case_id, op, p):
    """(fp32 inputs, float64 reference, bound) of a case: computed once, shared by the tests that need it, never written to."""
    if case_id not in _CACHE:
        make, ref = OPS[op]
        i = make(p, gen_for(case_id))
        r, bnd = ref(i, p)
        _CACHE[case_id] = (i, r, bnd)
    return _CACHE[case_id]


def fp32_eval(op, i, p):
    return OPS[op][1](i, p, dt=torch.float32)[0]
