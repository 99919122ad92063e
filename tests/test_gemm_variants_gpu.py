"""Every kernel a GEMM launch can select (csrc/gemm_split3.hip, gemm_v2.hip, gemm_h8c.hip, gemm_h8c4.hip, gemm_h8c_w8.hip, gemm_stream.hip, mlp_fused.hip), at the
smallest shapes that select it, element by element against the float64 reference and bound of tests/gemm_ref.py.  As in tests/test_kernel_variants_gpu.py:
fp32 outputs NaN-filled and planes zero-initialised before the launch, row strides / batch strides larger than dense with the gaps checked, every launch run
twice with identical bits, planes next to an fp32 output = split_planes of that output over the whole buffer, pad columns zero.  Before a case launches, the
planes ops.split_planes makes of its operands are compared byte for byte with the planes gemm_ref builds with torch casts (test_split_planes_bytes does the
same for split_planes_kernel alone at cols = 1, 31, 33, 100, odd rows, ld > cols): the reference is on the operands the kernel sees.

Random data only at K <= 128; every K > 128 runs exact-grid operands (gemm_ref: bound 0, or the epilogue's terms alone).  Case id = family-what-m<M>n<N>k<K>.

  family     kernel(s)                                            selected by (mmsa_gemm_split3 / mmsa_gemm_v2_launch)
  tiny       gemm_tiny_kernel                                     fp32 A, fp32 C only, N <= 64 or K <= 64: N = 1, 7, 8, 9, 64 x K = 32, 256, 288 (second lane pass partial), N = 130 at
                                                                  K = 64, M = 1 / 5, the six activations, colscale x alpha, resid x beta, batch 2, lda > K
  split3     gemm_split3_kernel<false,false> / <false,false,true> fp32 A (b3 / f3 weights): M = 1, 127, 129, N = 28 (a planes output beside it, or f3, keeps it off the tiny kernel), 130
                                                                  (N & 3: element-wise), 132; K = 96
             <false,true> / <false,true,true>                     the same with a pixel-shuffle store ((5, 7) and (4, 8), batch 2, in-place residual) or resid_mod = 103 at M = 515
             <true,false> / <true,true>                           b3 A planes with M < 128: M = 1, 77, 127
  v2_b3w4    gemm_v2_kernel<.., false, 4, B3>                     b3 planes, M >= 128, K <= 256 and no grid cap -- or flavour 4 (the deep-K and several-tiles cases)
  v2_b3w8    gemm_v2_kernel<.., true, 8, B3>                      b3 planes, K > 256, or flavour 8, a grid cap, row statistics or row normalisation
  v2_h8      gemm_v2_kernel<.., true, 8, H8>                      h8 line planes;   v2_f3: <.., true, 8, F3> f3 planes
  h8c        gemm_h8c_kernel   h8c4: gemm_h8c4_kernel (flavour 4, plain epilogue; also bit for bit against h8c)   w8: gemm_h8c_w8_kernel (K = 128, 256, 384)
     each of these crossed (_family below) with the six (GEN, ACT) pairs of V2_EPI_TABLE -- none / gelu / relu listed, runtime relu6 / hswish / sigmoid, GEN + none, GEN + an
     activation -- and: one tile; M = tile +- 1; N = 130, 132; ldc % 4 != 0; GEMM_MAX_GRID = 1 over 6 tiles; a 4 x 8 tile grid (blocked order); k-tile counts on both sides of the
     straight-line threshold (nk = 5 / 6; h8c, w8: 1 .. 6 chunks of 64); register epilogue "planes" and "rows" forms, scaled and unscaled; the `direct` planes-only path with
     and without row_norm, with relu, and declined by a misaligned colscale; 96-column tiles (N = 96, 192, 288, fp32 only); both outputs in every planes format and the output
     split; rowstats_out; row_norm onto planes (ragged M) and onto fp32 (M = 256, 512; rn-C-n384: the shape that took 96-column tiles); pixel-shuffle with (8, 8) and (5, 7),
     ps_C = 32 (element-wise planes) and 64; resid_mod = 103; batch 2 with every stride larger than dense; A as a column slice
  stream     gemm_stream_kernel<6,6,..> / <12,3,..> x F16 x RES   (N, K) = (96, 192), (192, 96), M = 16384 / 16391, b3 / f3, GEMM_MAX_GRID = 16 (every wave walks several blocks) and
                                                                  uncapped, none / relu / relu6, planes into a column slice; what it declines (192 x 192, gelu, h8 planes out, M = 16383)
                                                                  runs the tiled kernel: v2_* ids `declined-*`
  mlp_fused  mlp_fused_kernel<false|true>                         M = 1, 127, 129, 300, batch 2, GEMM_MAX_GRID = 1 over 5 tiles, ldx > C
test_variant_refused: what the launchers must refuse (RuntimeError, NaN-filled output untouched); ids say what."""
import pytest
import torch

from tests import gemm_ref as G
from tests.variant_ref import assert_inside
from tests.test_kernel_variants_gpu import DEV, bits, h8c_untouched_zero, nanbuf, pads_zero, planes_equal_split

pytestmark = pytest.mark.gpu
ACTS = ("none", "gelu", "relu", "relu6", "hswish", "sigmoid")

CASES = []     # (id, family, params)
RAISES = []    # (id, params)


def _c(op, tag, **p):
    p.setdefault("a", "planes")
    p.setdefault("out", "C")
    if p["K"] > 128:
        p["exact"] = True
    CASES.append((f"{op}-{tag}-m{p['M']}n{p['N']}k{p['K']}", op, p))


# ---- tiny
n = 0
for N in (1, 7, 8, 9, 64):
    for K in (32, 256, 288):
        kw = dict(kind="tiny", fmt="b3", a="fp32", M=1 if n % 3 == 0 else 5, N=N, K=K, act=ACTS[n % 6] if K == 32 else ("none", "relu")[n % 2])
        if n % 2:
            kw.update(colscale=True, alpha=0.75)
        if n % 3 == 1:
            kw.update(resid=True, beta=0.5 if n % 2 else 1.0)
        if n % 4 == 0:
            kw["batch"] = 2
        if n % 5 == 0:
            kw["lda_pad"] = 4
        _c("tiny", f"{kw['act']}{n}", **kw)
        n += 1
for n, act in enumerate(ACTS):
    _c("tiny", f"k64-{act}", kind="tiny", fmt="b3", a="fp32", M=5, N=130, K=64, act=act, bias=n % 2 == 0, ldc_pad=n % 2)
_c("tiny", "exact-gelu", kind="tiny", fmt="b3", a="fp32", M=5, N=9, K=288, act="gelu", colscale=True)
_c("tiny", "batch2-colscale", kind="tiny", fmt="b3", a="fp32", M=5, N=9, K=32, act="hswish", colscale=True, alpha=1.5, batch=2, resid=True, ldr_pad=3)

# ---- gemm_split3_kernel
for fmt, outs in (("b3", ("CP", "C", "CP", "C", "P")), ("f3", ("C",) * 5)):
    for n, (M, N, out) in enumerate(zip((1, 127, 129, 129, 127), (28, 130, 132, 132, 28), outs)):
        kw = dict(fmt=fmt, a="fp32", M=M, N=N, K=96, out=out, act=ACTS[n], pfmt=("b3", "h8", "f3")[n % 3])
        if n == 3:
            kw.update(ldc_pad=1, resid=True, ldr_pad=3, beta=0.5)
        if n == 2:
            kw.update(colscale=True, alpha=1.5, batch=2, lda_pad=8)
        _c("split3", f"{fmt}-fp32A-{out}{n}", **kw)
    pk = dict(out="CP", pfmt="b3") if fmt == "b3" else {}
    _c("split3", f"{fmt}-fp32A-ps5x7", fmt=fmt, a="fp32", M=70, N=144, K=96, ps=(5, 7, 36), batch=2, resid="inplace", act="sigmoid", colscale=True, **pk)
    _c("split3", f"{fmt}-fp32A-ps4x8", fmt=fmt, a="fp32", M=64, N=128, K=96, ps=(4, 8, 32), batch=2, resid="inplace", **pk)
    _c("split3", f"{fmt}-fp32A-rmod103", fmt=fmt, a="fp32", M=515, N=132, K=96, resid=True, resid_mod=103, act="relu")
    _c("split3", f"{fmt}-fp32A-ps-rmod", fmt=fmt, a="fp32", M=70, N=144, K=96, ps=(5, 7, 36), resid=True, resid_mod=103)
for n, M in enumerate((1, 77, 127)):
    _c("split3", f"b3-planesA-{n}", fmt="b3", M=M, N=(130, 132, 28)[n], K=96, out=("C", "CP", "P")[n], pfmt=("b3", "h8", "f3")[n], act=ACTS[n + 3], batch=1 + n % 2, a_slice=n == 1,
       colscale=n == 2)
_c("split3", "b3-planesA-split", fmt="b3", M=77, N=132, K=96, out="CP", pfmt="b3", psplit=64)
_c("split3", "b3-planesA-ps5x7", fmt="b3", M=70, N=144, K=96, ps=(5, 7, 36), batch=2, resid="inplace", out="CP", pfmt="h8")
_c("split3", "b3-planesA-rmod50", fmt="b3", M=77, N=132, K=96, resid=True, resid_mod=50, act="hswish")


# ---- the LDS-DMA families
def _family(op, fmt, bm, k0, kdeep, kthr, force=None, batch_ok=True, n96=True):
    """The epilogue / tile coverage every LDS-DMA kernel gets.  bm: rows per tile; k0: a shallow K (random data); kdeep: exact-grid Ks; kthr: the two Ks around the
    straight-line threshold; force: the GEMM_FLAVOUR the family needs where the shape alone would select another kernel."""
    f = dict(fmt=fmt, flavour=force) if force else dict(fmt=fmt)
    def c(tag, **p):
        if op == "v2_b3w4" and p.get("max_grid"):      # (a grid cap alone would select the 8-wave kernel)
            p["flavour"] = 4
        _c(op, tag, **{**f, **p})

    mm1 = bm - 1 if op != "v2_b3w4" else 2 * bm - 1       # (b3 planes with M < 128 run gemm_split3_kernel<true, ..>)
    own = fmt if fmt != "w8" else "h8c"
    # one tile, the six (GEN, ACT) pairs: rows form (none), staged (the others); GEN through resid_mod / pixel-shuffle
    for n, act in enumerate(ACTS):
        c(f"1tile-{act}", M=bm, N=128, K=k0, act=act, bias=n != 3)
    c("gen-none", M=bm, N=128, K=k0, resid=True, resid_mod=103)
    c("gen-relu6", M=2 * bm + 3, N=128, K=k0, resid=True, resid_mod=103, act="relu6", out="CP", pfmt=own)
    c("gen-gelu-ps8x8", M=bm, N=128, K=k0, ps=(8, 8, 32), act="gelu", out="CP", pfmt=own, colscale=True)
    c("gen-ps5x7", M=140 if bm == 128 else 280, N=256, K=k0, ps=(5, 7, 64), out="CP", pfmt="b3", resid="inplace", batch=2 if batch_ok else 1)
    c("gen-ps8x8-c64", M=bm, N=256, K=k0, ps=(8, 8, 64), out="P", pfmt=own)
    c("gen-ps-rmod", M=bm, N=128, K=k0, ps=(8, 8, 32), resid=True, resid_mod=103, act="relu")
    # register epilogue, planes form / rows form, scaled and unscaled; direct; direct declined
    c("regs-P-gelu", M=bm, N=128, K=k0, out="P", pfmt=own, act="gelu")
    c("regs-P-none", M=2 * bm, N=256, K=k0, out="P", pfmt=own, bias=False)
    c("rows-scaled-resid", M=bm, N=128, K=k0, colscale=True, alpha=0.75, resid=True, beta=0.5, ldr_pad=4)
    c("rows-resid", M=bm, N=256, K=k0, resid="inplace")
    c("rows-alpha", M=bm, N=128, K=k0, alpha=0.5)
    c("direct-scaled", M=bm, N=128, K=k0, out="P", pfmt=own, colscale=True, alpha=0.75, act="gelu")
    c("direct-relu", M=bm + 1, N=128, K=k0, out="P", pfmt=own, act="relu")
    c("direct-declined", M=bm, N=128, K=k0, out="P", pfmt=own, colscale="misaligned")
    for pf in ("b3", "h8", "f3", "h8c"):
        c(f"direct-{pf}", M=mm1, N=128, K=k0, out="P", pfmt=pf)
        c(f"both-{pf}", M=bm + 1, N=128, K=k0, out="CP", pfmt=pf, act="gelu", resid=True)
    c("both-split", M=bm, N=128, K=k0, out="CP", pfmt="f3" if fmt == "f3" else "b3", psplit=64)
    c("P-split", M=bm + 1, N=192, K=k0, out="P", pfmt="b3", psplit=128)
    # ragged tiles, unaligned leading dimensions
    c("ragged-m+1", M=bm + 1, N=128, K=k0, act="hswish")
    c("ragged-m-1", M=mm1, N=128, K=k0, resid=True)
    c("ragged-n130", M=bm, N=130, K=k0, out="CP", pfmt=own, act="relu")
    c("ragged-n132", M=bm + 1, N=132, K=k0, out="CP", pfmt=own, colscale=True)
    c("ldc-odd", M=bm, N=128, K=k0, ldc_pad=1, resid=True, ldr_pad=2, act="sigmoid")
    if op not in ("v2_b3w4", "v2_b3w8"):
        c("m-odd", M=77, N=128, K=k0, out="CP", pfmt=own)
    # several tiles per workgroup; blocked tile order; batches; A as a column slice
    c("grid1-6tiles", M=3 * bm, N=256, K=k0, max_grid=1)
    c("grid2-12tiles", M=3 * bm - 1, N=512, K=k0, max_grid=2, out="CP", pfmt=own, act="gelu")
    c("blocked-4x8", M=4 * bm, N=1024, K=k0)
    if batch_ok:
        c("batch2", M=bm + 1, N=132, K=k0, batch=2, colscale=True, resid=True, act="relu")
        c("batch2-P", M=bm, N=128, K=k0, batch=2, out="P", pfmt=own, colscale=True)
    if fmt in ("b3", "f3", "h8"):
        c("a-slice", M=bm, N=128, K=k0, a_slice=True)
    # 96-column tiles (fp32 only; h8c / w8: the same shapes run ragged 128-column tiles)
    for N in (96, 192, 288):
        c("n96", M=bm, N=N, K=k0, resid=N == 192, colscale=N == 288)
    c("n96-ragged", M=bm + 1, N=192, K=k0, act="relu")
    # row statistics; row normalisation onto planes and onto fp32
    if op != "v2_b3w4":
        c("rs-C", M=256, N=128, K=k0, rs=True)
        c("rs-CP-resid", M=512, N=128, K=k0, rs=True, out="CP", pfmt="h8c", resid="inplace")
        c("rs-CP-scaled", M=256, N=256, K=k0, rs=True, out="CP", pfmt="f3" if fmt == "f3" else "h8c", resid=True, colscale=True)
        c("rs-ragged", M=257, N=192, K=k0, rs=True, out="CP", pfmt=own)
        for n, pf in enumerate(("h8c", "h8", own if own not in ("h8", "h8c") else "b3")):
            c(f"rn-P-{pf}", M=257, N=128, K=k0, rn=True, out="P", pfmt=pf, act=("gelu", "none", "relu")[n])
        if batch_ok:
            c("rn-P-batch2", M=256, N=128, K=k0, rn=True, out="P", pfmt=own, batch=2, act="gelu")
            c("rn-C-batch2", M=256, N=128, K=k0, rn=True, batch=2)
        c("rn-C", M=512, N=128, K=k0, rn=True)
        c("rn-C-n384", M=256, N=384, K=k0, rn=True)       # fp32 only, N % 96 == 0: the 96-column-tile choice did not exclude row normalisation
    # k-tile counts
    for K in kthr:
        c("kthr", M=bm, N=128, K=K, resid=True)
        c("kthr-n96", M=bm + 1, N=192, K=K)
    for K in kdeep:
        c("deep", M=2 * bm + 1, N=256, K=K, out="CP", pfmt=own, act="relu")
        c("deep-gelu", M=bm, N=128, K=K, act="gelu", colscale=True, out="P", pfmt=own)


_family("v2_b3w4", "b3", 128, 64, (256,), (160, 192))
_c("v2_b3w4", "deep-flavour4", fmt="b3", flavour=4, M=257, N=256, K=288, out="CP", pfmt="b3")
_c("v2_b3w4", "deep-flavour4-n96", fmt="b3", flavour=4, M=128, N=192, K=320, resid=True)
_family("v2_b3w8", "b3", 256, 64, (288,), (160, 192), force=8)
_c("v2_b3w8", "natural-k288", fmt="b3", M=257, N=132, K=288, out="CP", pfmt="h8")
_family("v2_h8", "h8", 256, 64, (320,), (128, 192))
_family("v2_f3", "f3", 256, 64, (288,), (160, 192))
_family("h8c", "h8c", 256, 64, (256, 320, 384), (128, 192))
_family("w8", "w8", 256, 128, (256, 384), (128, 256), batch_ok=False)
for n, (M, N, K) in enumerate(((256, 128, 64), (257, 132, 128), (512, 256, 192), (1024, 1024, 64), (255, 96, 256))):
    _c("h8c4", f"plain{n}", fmt="h8c", flavour=4, M=M, N=N, K=K, out=("C", "CP", "P", "C", "CP")[n], pfmt="h8c", resid=n in (1, 3), colscale=n == 2, batch=2 if n == 1 else 1,
       **(dict(max_grid=2) if n == 3 else {}))

# ---- gemm_stream_kernel: <6, 6> = (N, K) = (96, 192), <12, 3> = (192, 96); x F16 x RES
n = 0
for (N, K) in ((96, 192), (192, 96)):
    for fmt in ("b3", "f3"):
        for res in (False, True):
            po = n % 3 == 2      # planes only, into a column slice; exact-grid there (K = 192): scaled by a power of two, so that the result stays on the grid the planes hold
            _c("stream", f"{fmt}-res{int(res)}", fmt=fmt, M=16391 if n % 2 else 16384, N=N, K=K, resid=res, beta=0.5 if n % 4 == 1 else 1.0, act=("none", "relu", "relu6")[n % 3], max_grid=16,
               out=("C", "CP", "P")[n % 3], pfmt=fmt, p_slice=po, colscale=n % 2 == 0 and not (po and K > 128), alpha=(0.5 if po and K > 128 else 0.75) if n % 4 == 2 else 1.0,
               ldc_pad=4 if n % 2 else 0)
            n += 1
_c("stream", "uncapped-b3", fmt="b3", M=16391, N=192, K=96, act="relu6", resid=True, out="CP", pfmt="b3")
_c("stream", "uncapped-f3", fmt="f3", M=16384, N=96, K=192, bias=False)
# declined by the streaming kernel: the tiled kernel's cases
_c("v2_b3w4", "declined-192x192", fmt="b3", M=16384, N=192, K=192, act="relu")
_c("v2_b3w4", "declined-gelu", fmt="b3", M=16384, N=192, K=96, act="gelu")
_c("v2_b3w4", "declined-h8-planes", fmt="b3", M=16384, N=192, K=96, out="P", pfmt="h8")
_c("v2_f3", "declined-m16383", fmt="f3", M=16383, N=96, K=192, act="relu")

# ---- mlp_fused_kernel
for fmt in ("b3", "f3"):
    for n, M in enumerate((1, 127, 129, 300)):
        CASES.append((f"mlp_fused-{fmt}-m{M}", "mlp_fused", dict(fmt=fmt, M=M, batch=1 + n % 2, ldx_pad=4 * (n % 2))))
    CASES.append((f"mlp_fused-{fmt}-grid1-m600", "mlp_fused", dict(fmt=fmt, M=600, max_grid=1, ldx_pad=8)))
del n, kw, pk
assert len({c[0] for c in CASES}) == len(CASES)


# ---- what the launchers must refuse
def _r(tag, **p):
    p.setdefault("a", "planes")
    p.setdefault("out", "C")
    p.setdefault("fmt", "b3")
    RAISES.append((f"refused-{tag}", p))


_r("k48", a="fp32", M=129, N=132, K=48, raw_k=True)
_r("h8-fp32A", fmt="h8", a="fp32", M=129, N=132, K=64)
_r("h8c-fp32A", fmt="h8c", a="fp32", M=129, N=132, K=64)
_r("f3-fp32A-planes-out", fmt="f3", a="fp32", M=129, N=132, K=96, out="CP", pfmt="f3")
_r("w8-k192", fmt="w8", M=256, N=128, K=192, raw_w8=True)
_r("w8-batch2", fmt="w8", M=256, N=128, K=128, batch=2)
_r("planes-lda-short", fmt="b3", M=256, N=128, K=64, short_lda=True)
_r("h8c-lda-short", fmt="h8c", M=256, N=128, K=64, short_lda=True)
_r("A-misaligned", a="fp32", M=129, N=132, K=96, a_misalign=True)
_r("rs-act", M=256, N=128, K=64, rs=True, act="gelu")
_r("rs-n96", M=256, N=96, K=64, rs=True)
_r("rs-m127", M=127, N=128, K=64, rs=True)
_r("rn-resid", M=256, N=128, K=64, rn=True, out="P", pfmt="b3", resid=True)
_r("rn-n192", M=256, N=192, K=64, rn=True, out="P", pfmt="b3")
_r("rn-C-m200", M=200, N=128, K=64, rn=True)
_r("rn-C-colscale", M=256, N=128, K=64, rn=True, colscale=True)
_r("h8c-planes-from-fp32A", a="fp32", M=129, N=132, K=96, out="CP", pfmt="h8c")
_r("ps-n-not-4c", M=128, N=128, K=64, ps=(8, 8, 36))
_r("ps-c-not-4", a="fp32", M=64, N=24, K=96, ps=(8, 8, 6))
_r("split-beyond-n", M=128, N=128, K=64, out="CP", pfmt="b3", psplit=128, raw_split=True)
_r("split-h8c", M=128, N=128, K=64, out="CP", pfmt="h8c", psplit=64, raw_split=True)
_r("flavour5", M=128, N=128, K=64, flavour=5)
MLP_RAISES = [("refused-mlp-c64", dict(fmt="b3", M=129, C=64)), ("refused-mlp-batch6", dict(fmt="b3", M=1, batch=6))]


# ------------------------------------------------------------------------------------------------ fixtures and helpers
@pytest.fixture(scope="module")
def ops():
    import mmsa
    return mmsa.ops


@pytest.fixture(autouse=True)
def knobs_restored(ops):
    yield
    assert ops.GEMM_FLAVOUR == 0 and ops.GEMM_MAX_GRID == 0, "a test left GEMM_FLAVOUR / GEMM_MAX_GRID set"


def dev(t):
    return t.contiguous().to(DEV)


def fmt_id(ops, name):
    return {"b3": ops.FMT_B3, "h8": ops.FMT_H8, "f3": ops.FMT_F3, "h8c": ops.FMT_H8C}[name]


def checked_planes(ops, x, fmt, weight=False):
    """ops.split_planes of the fp32 matrix x (CPU) -- byte for byte the planes gemm_ref builds with torch casts."""
    pl = ops.split_planes(dev(x), fmt=fmt_id(ops, fmt), weight=weight)
    torch.cuda.synchronize()
    want = G.planes_words(G.split(x, fmt), weight=weight)
    assert pl.p.shape == want.shape, f"planes shape {tuple(pl.p.shape)} vs {tuple(want.shape)}"
    assert torch.equal(pl.p.cpu(), want), f"split_planes ({fmt}, weight={weight}) differs from the torch-cast planes"
    return pl


def _stack_rows(t, rows, pad):
    """[B, rows, k] -> [B * (rows + pad), k] with the pad rows poisoned."""
    Bn, _, k = t.shape
    o = torch.full((Bn, rows + pad, k), G.POISON)
    o[:, :rows] = t
    return o.reshape(Bn * (rows + pad), k)


def prepare_gemm(ops, i, p):
    """The case's operands on the device, built and checked once."""
    B, M, N, K, fmt = p.get("batch", 1), p["M"], p["N"], p["K"], p["fmt"]
    d = {}
    npad = 2 if B > 1 else 0
    if fmt == "w8":
        d["w"] = ops.w8_planes(dev(i["w"][0]))
        torch.cuda.synchronize()
        assert torch.equal(bits(ops.planes_to_float(d["w"]).cpu()), bits(i["w"][0])), "fp8_dequantize of the packed codes is not the case's weight"
        d["stride_w"] = 0
    else:
        wall = checked_planes(ops, _stack_rows(i["w"], N, npad), fmt, weight=fmt == "h8")
        d["w"] = ops.Planes(wall.p, N, K, wall.kpad, wall.fmt, wall.weight)
        d["stride_w"] = wall.batch_stride(N + npad) if B > 1 else 0
    mpad = (2 + M % 2) if B > 1 else 0
    d["mpad"] = mpad
    arows = _stack_rows(i["a"], M, mpad)
    if p["a"] == "fp32":
        lda = K + p.get("lda_pad", 0)
        off = 1 if p.get("a_misalign") else 0
        buf = nanbuf(off + arows.shape[0] * lda + 3)
        av = buf[off:off + arows.shape[0] * lda].view(arows.shape[0], lda)
        av[:, :K] = dev(arows)
        d["a"], d["stride_a"], d["keep"] = av[:, :K], (M + mpad) * lda, buf
    else:
        afmt = "h8c" if fmt == "w8" else fmt
        if p.get("a_slice"):      # columns 32 .. 32 + K of planes of a wider matrix
            wide = torch.full((arows.shape[0], K + 64), G.POISON)
            wide[:, 32:32 + K] = arows
            apl = checked_planes(ops, wide, afmt)
            d["a"], d["stride_a"] = apl.cols(32, 32 + K), (M + mpad) * apl.p.stride(0)
        else:
            apl = checked_planes(ops, arows, afmt)
            d["a"], d["stride_a"] = apl, apl.batch_stride(M + mpad) if B > 1 else 0
            if p.get("short_lda"):
                d["a"] = ops.Planes(apl.p[:, :apl.p.shape[1] - 64].contiguous(), apl.n, K, apl.kpad, apl.fmt)
    sb = N + 4                                             # bias / colscale / colsum share one batch stride
    d["stride_bias"] = sb
    for name in ("bias", "colscale", "colsum"):
        if name in i:
            off = 1 if (name == "colscale" and p.get("colscale") == "misaligned") else 0
            buf = nanbuf(off + B * sb)
            v = i[name]
            buf[off:].view(B, sb)[:, :v.shape[1]] = dev(v)
            d[name] = buf[off:]
    if "mr" in i:
        d["mr"] = dev(i["mr"].reshape(B * M, 2))
    return d


def launch_gemm(ops, d, i, p, refuse=False):
    """One launch into fresh buffers.  Returns dict(y [B, rows, cols] or None, decoded, raw, ...) after the checks that need no reference.  refuse: the launcher
    must raise RuntimeError and leave every output as it was."""
    B, M, N, K = p.get("batch", 1), p["M"], p["N"], p["K"]
    rows, cols = (4 * M, p["ps"][2]) if p.get("ps") else (M, N)
    out = p["out"]
    kw = dict(bias=d.get("bias"), act=p.get("act", "none"), alpha=p.get("alpha", 1.0), colscale=d.get("colscale"), beta=p.get("beta", 1.0), resid_mod=p.get("resid_mod", 0),
              batch=B, m=M, stride_a=d["stride_a"], stride_w=d["stride_w"], stride_bias=d["stride_bias"], pixel_shuffle=p.get("ps"))
    opad = 1 if B > 1 else 0
    cbuf = cview = None
    if "C" in out:
        ldc = cols + p.get("ldc_pad", 0)
        cbuf = nanbuf(B, rows + opad, ldc)
        cview = cbuf[:, :rows, :cols]
        kw.update(out=cbuf.view(B * (rows + opad), ldc)[:rows, :cols], stride_c=(rows + opad) * ldc)
    rbuf = None
    if p.get("resid") == "inplace":
        cview.copy_(dev(i["resid"]))
        kw.update(resid=kw["out"], stride_r=kw["stride_c"])
    elif p.get("resid"):
        rr = p.get("resid_mod") or rows
        ldr = cols + p.get("ldr_pad", 0)
        rbuf = nanbuf(B, rr + opad, ldr)
        rbuf[:, :rr, :cols] = dev(i["resid"])
        kw.update(resid=rbuf.view(B * (rr + opad), ldr)[:rr, :cols], stride_r=(rr + opad) * ldr)
    pl = wide = None
    ppad = 0
    if "P" in out:
        pf = fmt_id(ops, p["pfmt"])
        ppad = (2 + rows % 2) if B > 1 else 0
        if p.get("p_slice"):      # the planes output is columns 32 .. 32 + cols of wider planes
            wide = ops.alloc_planes(B * (rows + ppad), cols + 32, DEV, zero=True, fmt=pf)
            pl = wide.cols(32, 32 + cols)
        elif p.get("raw_split"):
            pl = ops.alloc_planes(B * (rows + ppad), cols, DEV, zero=True, fmt=pf)
            pl.split = p["psplit"]
        else:
            pl = ops.alloc_planes(B * (rows + ppad), cols, DEV, zero=True, fmt=pf, split=p.get("psplit", 0))
        kw.update(out_planes=pl, stride_cp=(rows + ppad) * pl.p.stride(0) // (2 if pf == ops.FMT_H8C else 1) if B > 1 else 0)
    rs = None
    if p.get("rs"):
        rs = nanbuf(B * M + 3, 2 * max(N // 64, 1))
        kw["rowstats_out"] = rs
    if p.get("rn"):
        kw["row_norm"] = (d["mr"], d["colsum"])
    before = [t.clone() for t in (cbuf, pl.p if pl else None, rs) if t is not None] if refuse else None
    ops.GEMM_FLAVOUR, ops.GEMM_MAX_GRID = p.get("flavour") or 0, p.get("max_grid", 0)
    try:
        if refuse:
            with pytest.raises(RuntimeError):
                ops.gemm(d["a"], d["w"], **kw)
        else:
            ops.gemm(d["a"], d["w"], **kw)
    finally:
        ops.GEMM_FLAVOUR, ops.GEMM_MAX_GRID = 0, 0
    torch.cuda.synchronize()
    if refuse:
        for t, b in zip([t for t in (cbuf, pl.p if pl else None, rs) if t is not None], before):
            assert torch.equal(bits(t), bits(b)), "a refused launch wrote to its output"
        return None
    res = dict(raw=[t for t in (cbuf, wide.p if wide else (pl.p if pl else None), rs) if t is not None])
    if cbuf is not None:
        assert bool(torch.isnan(cbuf[:, rows:]).all()) and bool(torch.isnan(cbuf[:, :, cols:]).all()), "the gap behind an output row / between two batches was written"
        res["y"] = cview
    if rbuf is not None:
        assert bool(torch.isnan(rbuf[:, :, cols:]).all()) and bool(torch.isnan(rbuf[:, (p.get("resid_mod") or rows):]).all()), "the residual's gaps were written"
    if pl is not None:
        pc = pl if wide is None else ops.Planes(pl.p.contiguous(), pl.n, pl.k, pl.kpad, pl.fmt)
        if wide is not None:
            assert bool((wide.p[:, :64] == 0).all()), "planes columns in front of the output slice were written"
        h8c = pl.fmt == ops.FMT_H8C
        if cbuf is not None:      # the planes are the split of this launch's own fp32 output, over the whole buffer (pad rows and pad columns zero)
            ybig = torch.zeros(B, rows + ppad, cols, device=DEV)
            ybig[:, :rows] = cview
            ybig = ybig.view(B * (rows + ppad), cols)
            if p.get("psplit"):
                s = p["psplit"]
                lo = ops.split_planes(ybig[:, :s].contiguous(), fmt=pl.fmt)
                hi = ops.split_planes(ybig[:, s:].contiguous(), fmt=ops.FMT_H8)
                torch.cuda.synchronize()
                assert torch.equal(pc.p, torch.cat([lo.p, hi.p], 1)), "split-format planes differ from split_planes of the same launch's fp32 output"
            else:
                planes_equal_split(ops, pc, ybig, pl.fmt)
        else:
            dec = ops.planes_to_float(pc).view(B, rows + ppad, cols)
            assert bool((dec[:, rows:] == 0).all()), "planes rows between two batches were written"
            if not h8c and ppad:
                assert bool((pc.p.view(B, rows + ppad, -1)[:, rows:] == 0).all())
            rel = torch.full((cols,), G.FMT_REL[p["pfmt"]], dtype=torch.float64)
            if p.get("psplit"):
                rel[p["psplit"]:] = G.FMT_REL["h8"]
            else:
                assert h8c_untouched_zero(pc) if h8c else pads_zero(ops, pc)
            res["decoded"], res["rel"] = dec[:, :rows], rel
    if rs is not None:      # strip sums of the launch's own stored rows
        assert bool(torch.isnan(rs[B * M:]).all()), "row statistics beyond the last row were written"
        x = torch.stack([cview[b] for b in range(B)]).double().cpu().view(B * M, N // 64, 64)
        got = rs[:B * M].double().cpu().view(B * M, N // 64, 2)
        for k, (want, mag) in enumerate(((x.sum(2), x.abs().sum(2)), ((x * x).sum(2), (x * x).sum(2)))):
            assert bool(((got[..., k] - want).abs() <= 68 * G.U * mag).all()), f"strip {'sums' if k == 0 else 'sums of squares'} outside (64 + 4) u sum |.|"
    return res


def prepare_mlp(ops, i, p):
    B, M, fmt = p.get("batch", 1), p["M"], p["fmt"]
    C = p.get("C", 96)
    mpad = 2 if B > 1 else 0
    d = dict(mpad=mpad)
    d["a"] = checked_planes(ops, _stack_rows(i["a"], M, mpad), fmt)
    w1 = checked_planes(ops, _stack_rows(i["w1"], 4 * C, mpad), fmt)
    w2 = checked_planes(ops, _stack_rows(i["w2"], C, mpad), fmt)
    d["w1"], d["w2"] = w1, w2
    d["strides"] = dict(stride_a=d["a"].batch_stride(M + mpad), stride_w1=w1.batch_stride(4 * C + mpad), stride_w2=w2.batch_stride(C + mpad)) if B > 1 else {}
    d["b1"], d["b2"], d["gamma"] = (dev(i[k].reshape(-1)) for k in ("b1", "b2", "gamma"))
    return d


def launch_mlp(ops, d, i, p):
    B, M = p.get("batch", 1), p["M"]
    C = p.get("C", 96)
    opad = 1 if B > 1 else 0
    ldx = C + p.get("ldx_pad", 0)
    xbuf = nanbuf(B, M + opad, ldx)
    xbuf[:, :M, :C] = dev(i["x"])
    ops.GEMM_MAX_GRID = p.get("max_grid", 0)
    try:
        ops.convnext_mlp_fused(d["a"], d["w1"], d["w2"], d["b1"], d["b2"], d["gamma"], xbuf.view(B * (M + opad), ldx)[:M, :C], M, batch=B, stride_x=(M + opad) * ldx, **d["strides"])
    finally:
        ops.GEMM_MAX_GRID = 0
    torch.cuda.synchronize()
    assert bool(torch.isnan(xbuf[:, M:]).all()) and bool(torch.isnan(xbuf[:, :, C:]).all()), "the gap behind a row of x / between two batches was written"
    return dict(raw=[xbuf], y=xbuf[:, :M, :C])


WORST = {}     # family -> (worst |y - r| / bound, case id)


def judge(cid, op, y, r, bnd, what=""):
    """Print the worst |y - r| / bound of the case (exact-grid cases: the number of elements that differ) BEFORE asserting, and keep the family's worst."""
    y = y.detach().double().cpu()
    err = (y - r).abs()
    pos = bnd > 0
    ratio = float((err[pos] / bnd[pos]).nan_to_num(float("inf")).max()) if bool(pos.any()) else 0.0
    differ = int((~(err[~pos] == 0)).sum())
    print(f"{cid}{what}: worst |y - r| / bound = {ratio:.3f}" + (f"; {int((~pos).sum())} elements with bound 0, {differ} of them differ" if bool((~pos).any()) else ""))
    if ratio > WORST.get(op, (-1.0, ""))[0]:
        WORST[op] = (ratio, cid)
    assert_inside(y, r, bnd, cid + what)


@pytest.mark.parametrize("cid,op,p", CASES, ids=[c[0] for c in CASES])
def test_variant(ops, cid, op, p):
    i, r, bnd = G.case_data(cid, op, p)
    prepare, launch = (prepare_mlp, launch_mlp) if op == "mlp_fused" else (prepare_gemm, launch_gemm)
    d = prepare(ops, i, p)
    first = launch(ops, d, i, p)
    again = launch(ops, d, i, p)
    for a, b in zip(first["raw"], again["raw"]):
        assert torch.equal(bits(a), bits(b)), f"{cid}: two identical calls differ in their bits"
    if first.get("y") is not None:
        judge(cid, op, first["y"], r, bnd)
    if "decoded" in first:
        judge(cid, op, first["decoded"], r, bnd + first["rel"] * r.abs(), " (planes)")
    if op == "h8c4":      # the four-wave kernel against the eight-wave kernel, bit for bit
        ref8 = launch(ops, d, i, {**p, "flavour": 0})
        for a, b in zip(first["raw"], ref8["raw"]):
            assert torch.equal(bits(a), bits(b)), f"{cid}: gemm_h8c4_kernel and gemm_h8c_kernel differ in their bits"


@pytest.mark.parametrize("cid,p", RAISES, ids=[c[0] for c in RAISES])
def test_variant_refused(ops, cid, p):
    """What the launchers refuse; the NaN-filled / zeroed outputs stay as they were.  (Only the inputs are drawn: a refused shape has no reference.)"""
    w8b = p["fmt"] == "w8" and p.get("batch", 1) > 1      # (operands of one batch: the launcher refuses before it looks at a second)
    q = {**p, "K": 64 if p.get("raw_k") else p["K"], "batch": 1 if w8b else p.get("batch", 1)}
    i = G.make_gemm(q, G.gen_for(cid))
    if p.get("raw_w8"):      # a W8 weight of K = 192 cannot be packed by ops.w8_planes: its words are handed over as they would lie
        d = prepare_gemm(ops, i, {**p, "fmt": "h8c"})
        d["w"] = ops.Planes(torch.zeros(p["N"] + 1, p["K"] // 2, dtype=torch.int16, device=DEV), p["N"], p["K"], p["K"], ops.FMT_W8, True)
        d["stride_w"] = 0
    elif p.get("raw_k"):     # planes of K = 48 columns per row: no packer makes them
        d = prepare_gemm(ops, i, q)
        d["w"] = ops.Planes(torch.zeros(p["N"], 2 * p["K"], dtype=torch.int16, device=DEV), p["N"], p["K"], p["K"], ops.FMT_B3)
        d["a"], d["stride_a"] = d["a"][:, :p["K"]], 0
    elif p["fmt"] in ("h8", "h8c") and p["a"] == "fp32":
        d = prepare_gemm(ops, i, {**p, "a": "planes"})
        d["a"] = dev(i["a"][0])
    else:
        d = prepare_gemm(ops, i, q)
    launch_gemm(ops, d, i, p, refuse=True)


@pytest.mark.parametrize("cid,p", MLP_RAISES, ids=[c[0] for c in MLP_RAISES])
def test_mlp_refused(ops, cid, p):
    C, B, M = p.get("C", 96), p.get("batch", 1), p["M"]
    g = G.gen_for(cid)
    i = dict(a=torch.randn(B, M, C, generator=g), w1=torch.randn(B, 4 * C, C, generator=g), w2=torch.randn(B, C, 4 * C, generator=g), b1=torch.randn(B, 4 * C, generator=g),
             b2=torch.randn(B, C, generator=g), gamma=torch.randn(B, C, generator=g), x=torch.randn(B, M, C, generator=g))
    d = prepare_mlp(ops, i, p)
    x = nanbuf(B * (M + 1), C)
    with pytest.raises(RuntimeError):
        ops.convnext_mlp_fused(d["a"], d["w1"], d["w2"], d["b1"], d["b2"], d["gamma"], x[:M], M, batch=B, stride_x=(M + 1) * C, **d["strides"])
    torch.cuda.synchronize()
    assert bool(torch.isnan(x).all()) and ops.GEMM_MAX_GRID == 0


@pytest.mark.parametrize("fmt,weight", G.SPLIT_KINDS, ids=[f"{f}{'-weight' if w else ''}" for f, w in G.SPLIT_KINDS])
@pytest.mark.parametrize("rows,cols", [(1, 1), (3, 31), (5, 33), (7, 100), (2, 64)])
def test_split_planes_bytes(ops, fmt, weight, rows, cols):
    """split_planes_kernel, all five kinds, element by element: the source a column slice of a wider NaN-filled matrix (ld > cols), odd row counts, columns that
    are no multiple of the 32- / 64-wide blocks, values at and beyond every clamp."""
    x = G.make_split(rows, cols, G.gen_for(f"split-{fmt}-{weight}-{rows}-{cols}"))
    src = nanbuf(rows, cols + 8)
    src[:, 4:4 + cols] = dev(x)
    pl = ops.split_planes(src[:, 4:4 + cols], fmt=fmt_id(ops, fmt), weight=weight)
    again = ops.split_planes(src[:, 4:4 + cols], fmt=fmt_id(ops, fmt), weight=weight)
    torch.cuda.synchronize()
    want = G.planes_words(G.split(x, fmt), weight=weight)
    assert pl.p.shape == want.shape and torch.equal(pl.p.cpu(), want) and torch.equal(pl.p, again.p)
    assert torch.equal(bits(ops.planes_to_float(pl).cpu()), bits(G.value(G.split(x, fmt))))


def test_zz_family_summary():
    """Prints, after every case has run, each family's worst |y - r| / bound (profiles/README.md quotes this table)."""
    for op in sorted(WORST):
        print(f"family {op}: worst |y - r| / bound = {WORST[op][0]:.3f} ({WORST[op][1]})")
    assert not WORST or set(WORST) <= set(G.OPS)
