"""Every `__global__` of conv.hip, conv_pair.hip, gconv_mfma.hip, gfe_qkv.hip, norm.hip (layernorm_rows / rowstats_finalize / colstats / ffrm / lnhw), neck.hip,
tail.hip, head.hip and the forward and backward kernels of msda.hip that a shape can select, reached through its launcher at the smallest shape that selects it and held
ELEMENT BY ELEMENT to the float64 bound of tests/variant_ref.py.  Every call runs twice into NaN-filled outputs and must give identical bits (outputs that meet in float atomics excepted: see msdab-*); wherever a
launch writes fp32 and operand planes together, the planes must be ops.split_planes of that launch's own fp32 output, bit for bit over the whole
zero-initialised buffer (pad columns stay zero).  layernorm_rows and the fused MSDA entries also write the row-pair (h8c) format (csrc/common.h h8c_row /
h8c_lo_off): there the pad columns, whatever lies behind a pair, and the unused half of a last odd row pair must stay as initialised (h8c_untouched_zero).

The table: case id -> operation, launcher, the kernel the shape selects and why.  The ids carry the shape; B = 2 throughout (the batch stride is part of
what can go wrong).  profiles/README.md says how the kernel trace of one run of this file is recorded.

  dw3-strip-*     mmsa_dwconv_nhwc   dwconv3_strip_kernel      k = 3, W % 4 == 0, 16-byte aligned pointers
  dw3-nhwc-*      mmsa_dwconv_nhwc   dwconv3_nhwc_kernel       k = 3, W = 7 (W % 4 != 0), aligned
  dw3-gen-*       mmsa_dwconv_nhwc   dwconv_nhwc_kernel        k = 3, x starts one float past a 16-byte boundary: the alignment test fails
  dw3-stride      mmsa_dwconv_nhwc   dwconv3_strip_kernel      xstride_b / ystride_b larger than dense (the gap must stay untouched)
  dw3-pl-*        mmsa_dwconv_nhwc   strip / nhwc / generic    fp32 + planes (b3, h8, f3) at C = 36 (pad columns) and C = 64; -only: planes alone
  dw5-*           mmsa_dwconv_nhwc   dwconv_nhwc_kernel        k = 5 has no kernel of its own
  dw7-gelu        mmsa_dwconv_nhwc   dwconv_nhwc_kernel        k = 7 with an activation: the 7 x 7 kernels take act == none only
  dw7-tiled-*     mmsa_dwconv_nhwc   dwconv7_tiled_kernel      k = 7, act none, aligned, H or W not a multiple of 16 (8x8, ragged 9x15, 1x1; C = 96: a 32-channel last chunk)
  dw7-blk-*       mmsa_dwconv_nhwc   dwconv7_blk_kernel        k = 7, act none, fp32 only, C % 32 == 0, H % 16 == 0, W % 16 == 0
  dw7-*-ipg       mmsa_dwconv_nhwc   blk / tiled               imgs_per_group = 1: each image its own weights and bias
  dw7-pl-*        mmsa_dwconv_nhwc   dwconv7_tiled_kernel      planes need C % 64 == 0, H % 8 == 0, W % 8 == 0 (lane-pair stores)
  dw7-pl-gen      mmsa_dwconv_nhwc   dwconv_nhwc_kernel        k = 7 planes at C = 32: not a full 64-channel chunk, the generic kernel writes them
  gc1-t*          mmsa_gconv_nhwc    gconv_tiled_kernel<N,1>   k = 1, no bias / act, cout_g = N in the template list
  gc3-t*          mmsa_gconv_nhwc    gconv_tiled_kernel<N,3>   k = 3, cout_g = N <= 16: mmsa_gconv3_mfma_launch declines one n-tile.  (<18,3> <24,3> <36,3> <72,3> are
                                                               reachable through the MMSA_GCONV_VALU knob only: the matrix-pipe kernel takes cout_g 17..48 and 65..80.)
  gc3-mfma*       mmsa_gconv_nhwc    gconv3_mfma_kernel<2|3|5> k = 3, cout_g = 18 / 40 / 72 (2, 3, 5 n-tiles)
  gc3-gen50/81    mmsa_gconv_nhwc    gconv_nhwc_kernel         k = 3, cout_g = 50 (4 n-tiles: declined) / 81 (> 5 n-tiles: declined), not in the template list
  gc1-gen5, gc3-gen5  mmsa_gconv_nhwc gconv_nhwc_kernel        cout_g = 5: outside the template list (k = 3: one n-tile, declined too)
  gc3-gen-bias-*  mmsa_gconv_nhwc    gconv_nhwc_kernel         bias / activation: the generic kernel alone takes them
  gc5-gen         mmsa_gconv_nhwc    gconv_nhwc_kernel         k = 5
  gc3-pair-w*     mmsa_gconv_nhwc    dwpair_nhwc_kernel        k = 3, cin_g = cout_g = 2, even G, aligned: handed to mmsa_dwpair_nhwc_launch
  gc3-pair-oddG   mmsa_gconv_nhwc    gconv_nhwc_kernel         the same with G = 7: the pair kernel works on two groups per lane
  gfe-*           mmsa_gfe_qkv_conv  gfe_qkv_kernel<3|6|12|24> cout_g = 3 cin_g, G cin_g % 24 == 0; -declined: returns False and leaves the NaN-filled output alone
  gate-*          mmsa_dwpair_gate   dwpair_gate4_kernel (W % 4 == 0) / dwpair_gate_kernel; fp32 + b3 planes
  ca-*            mmsa_ca_apply      ca_apply_kernel           fp32 + b3 planes
  gg-*            mmsa_gelu_gate     gelu_gate_kernel
  pool-*          mmsa_pool_hw       pool_hw_kernel<true>; pool-c6: C % 4 != 0 -> pool_hw_kernel<false>
  cs-*            mmsa_colstats      colstats_kernel           HW = 4097: nine 512-row blocks; wrow on / off; out_is_zero on / off.  The blocks meet in a double
                                                               atomicAdd whose order is free, yet two calls must agree in every bit: every term is an fp32
                                                               partial of eight rows (24 bits; it ends at 2^-36 or above for the seeded inputs here, whose
                                                               totals stay below 2^17), so each double addition is exact and the order cannot show.  Data
                                                               with a far wider range of magnitudes could differ in the last bit without a fault in the kernel.
  ffrm-*          mmsa_ffrm_finalize ffrm_stats / ffrm_matvec / ffrm_gate kernels
  lnhw-*          mmsa_lnhw_apply    lnhw_apply_kernel
  gram-*          mmsa_gram_tn       gram_part_kernel + gram_sum_kernel; P around the 256-row slice, c = 768: 8 x 8 blocks; nblk = 8: diagonal head blocks only
  chan-*, gffm-*  mmsa_chanattn_build / mmsa_gffm_build        c = 80: cpad = 96, pad columns must stay zero
  tail-*          mmsa_tail_fuse     tail_fuse64_kernel; tail-c6: C % 4 != 0 -> tail_fuse_kernel; -pl: b3 planes (C % 32 == 0); -noxtok: xtok = None;
                                     tail-pl-narrow: cmap one float past a 16-byte boundary -> tail_fuse_kernel with planes
  n2p-*           mmsa_nchw_to_planes  nchw_to_planes_kernel<true>: HW % 4 == 0 and image stride % 4 == 0 (n2p-c36-hw4096 dense, n2p-c64-hw4096 stride + 4);
                                       every other case <false> (HW = 1, 35, or n2p-c8-hw4096 with stride + 3)
  t2n-*           mmsa_tokens_to_nchw  tokens_to_nchw_kernel
  head-*          mmsa_head_fuse     head_fuse_kernel          four unequal, non-square levels, fp32 + planes
  ln-c*-r*        mmsa_layernorm_rows  layernorm_rows_kernel<NV, RPW>: C = 4, 8, 36, 96, 128 -> <1,2>; 132, 256 -> <1,1>; 260, 384, 512 -> <2,1>; 516, 1024 -> <4,1>;
                                       1028, 2048 -> <8,1>; 2052, 4096 -> <16,1>: each side of each dispatch boundary; rows = 1, 7, 9: less than one workgroup's rows
                                       (4, or 8 at <1,2>) and a ragged last workgroup; eps alternates 1e-6 / 1e-5; every seventh row has a variance near eps
  ln-stream-*     mmsa_layernorm_rows  the streamed walk: rows = 4099 (two rows per slot) / 8197 (four): a slot handles several rows with the next row's loads in flight
  ln-out-*        mmsa_layernorm_rows  y + y2; y + planes and planes alone in b3, h8, f3, h8c at C = 36, 100 (C % 8 != 0: store_planes4 / h8c_store4), 96 (pad
                                       columns up to 128) and 64 (the lane-pair stores); rows = 7: an odd last row pair of the h8c planes
  ln-stride-*     mmsa_layernorm_rows  x a column slice of a wider NaN-filled matrix, y and y2 with ld > C (the gap stays NaN)
  ln-patch-*      mmsa_layernorm_rows  the 2 x 2 patchify map, (H, W) = (2, 2) and (4, 6), two images; planes need C % 32 == 0
  ln-grp*         mmsa_layernorm_rows  row groups with their own weights: group_rows = 5 at C = 96 (<1,2>: the two halves of a wave in different groups); 300 with
                                       wrap and y_gcol = C, and plain; 2050 with rows = 4100 (a slot crosses the group boundary in mid-walk: the `grp != cur_grp`
                                       weight reload); ln-grp-patch-*: grouping with patchify, one image per group
  ln-cw-*         mmsa_layernorm_rows  the clamp watch: h8 planes with |y| > 57344 leave the largest |y| of the fp32 output in the word, bit for bit; ordinary
                                       magnitudes and bf16 hi/lo planes leave 0
  ln-*-refused    mmsa_layernorm_rows  odd patchify H; y2 with patchify; patchified planes with C % 32 != 0; h8c with patchify / groups / a pair stride below
                                       3 * pad64(C); C = 6; C = 4100; rows not a multiple of group_rows
  rs-*            mmsa_rowstats_finalize  rowstats_finalize_kernel: rows = 1, 255, 257 (one 256-thread block and one row more), strips = 1, 2, 16; row 3 constant
                                       (the variance clamps to 0); rs-d100-refused: D != 64 * strips
  msda-d*-q*      mmsa_ms_deform_attn_forward  msda_kernel<false>: D = 4, 8, 12, 32, 40, 64.  Workgroups = ceil(B Lq M (D / 4) / block), block = (256 / (D / 4)) (D / 4);
                                       mmsa_xcd_order permutes the first 8 * (grid / 8) of them:
                                           D = 32, M = 4 (block 256): Lq = 4 / 27 / 32 / 33 / 67 -> 1 / 7 / 8 / 9 / 17 workgroups
                                           D = 40, M = 4 (block 250): Lq = 3 / 26 -> 1 / 9
                                           D = 4 / 8 / 64, M = 4, Lq = 33 -> 2 / 3 / 17;  D = 12, M = 3 (block 255), Lq = 33 -> 3
  msda-scalar-*   mmsa_ms_deform_attn_forward  msda_scalar_kernel<float>: D = 2, D = 6 (D % 4 != 0) and D = 32 with `value` one float past a 16-byte boundary;
                                       <__half> and <double>: D = 2 and 32
  msda-dyadic-*   both entries         levels (4, 8), (2, 4) and dyadic locations: every pixel coordinate exact in fp32; h_im / w_im hit -1 (excluded), -0.5, 0,
                                       size - 1 (upper taps zero) and size (excluded)
  msdaf-*         mmsa_msda_fused      msda_kernel<true> on fp32 values: fp32 alone, fp32 + planes (b3, h8, f3, h8c), planes alone; D = 4, 12 (store_planes4_any),
                                       8, 32, 40 (the pair store); M D = 96 with h8c (pad to 128); msdaf-stride: ldraw and ldo larger than dense, NaN gaps;
                                       msdaf-cw-*: the clamp watch with h8c planes
  msdap-*         mmsa_msda_fused_planes  msda_planes_kernel<false|true> (lo0 / lo1) on H8 value planes that hold the case's values exactly: (M, D) = (4, 8),
                                       (2, 32), (3, 64), (1, 32); outputs as msdaf-*
  msda*-refused   the MSDA entries     D = 6 fused; M D = 48 with value planes; ldraw too small; b3 planes as value; batch 3 with im2col_step 2; an fp32 value
                                       matrix with a row stride, or with the wrong row count (ops.msda_fused: the entry takes no stride)
  msdab-*         mmsa_ms_deform_attn_backward  msda_bwd_kernel<T, SHFL>, one lane per (b, q, m, c), 256 lanes per workgroup; called through lib.call with the three
                                       outputs as views inside larger NaN-filled tensors (the guard regions must stay NaN: the memset sizes, for 2-, 4- and 8-byte
                                       elements); where reference and bound are 0 (a value element no sample touches, a sample outside the map) the device must
                                       hold 0, not NaN.  SHFL = D a power of two <= 64: grad_sampling_loc / grad_attn_weight leave an xor-shuffle tree inside the
                                       D-lane group and must repeat bit for bit.  grad_value always, and with any other D all three outputs, meet in float atomics
                                       whose order is free (unlike cs-*, the addends here are not exact in the sum): there BOTH calls are held to the bound and no
                                       bits are compared.
      -f32-shfl-   <float, true>       D = 1 (no shuffle step), 2, 8 (M = 3, Lq = 33: 1584 lanes = 24 waves + 48 lanes, the last wave holds whole inactive lane
                                       groups that still shuffle), 32, 64 (M = 3, Lq = 33: a lane group is a whole wave, 12672 lanes = 49.5 workgroups) and
                                       D = 16 with M = 4, Lq = 32: 4096 lanes, a multiple of 256
      -f32-atom-   <float, false>      D = 3, 12, 40, and 128 (a power of two above 64 must not take the shuffle path)
      -f64-*       <double, true|false>  D = 2, 32 | 6, 40
      -f16-*       <__half, true|false>  D = 2, 32 | 3 (odd: grad_value elements fall on both halves of the packed pair), 40; every addend to an atomic is
                                       rounded to fp16 and meets in global_atomic_pk_add_f16
      -dyadic-*    <float, true|false> levels (4, 8), (2, 4), D = 8 | 6, the dyadic locations of msda-dyadic-*: the position term of the bound is zero and the
                                       one-sided taps at exact integers must match the reference's floor
                                       Worst |y - r| / bound over both calls, as measured on an MI355X (printed by the test; none of it feeds back into the bound):
                                           f32 shuffle (gloc, gaw)   0.312 (gloc, msdab-f32-shfl-m3d2-q33)      f32 atomics (all three; gvalue everywhere)  0.360 (gloc, -atom-m3d3-)
                                           f64 (all paths)           0.178 (gloc, msdab-f64-shfl-m3d2-q33)      f16 atomics (all three; gvalue everywhere)  0.533 (gvalue, -atom-m4d40-)
                                           f16 shuffle (gloc, gaw)   0.989 (gloc, msdab-f16-shfl-m3d2-q33): one rounding to fp16 of a result whose fp32 error is
                                                                     far smaller, so the 2^-11 |r| term is all but attained whenever r falls next to a rounding tie
                                           dyadic                    0.222 (gvalue); the smallest per-output figure of any case is 0.013 (gaw, D = 128)
                                       The same statement in torch's fp32 on the CPU reaches 0.01 .. 0.36 of the bound, and every wrong restatement of
                                       test_kernel_variants_cpu.py leaves it in more than a hundred elements of every case (D = 128, the loosest, included).
  msdab-*-refused ops.msda_backward    batch 3 with im2col_step 2 (the launcher); grad_output of the wrong shape, of another dtype, non-contiguous; bfloat16
"""
import pytest
import torch

from tests import variant_ref as V

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NAN = float("nan")
B = 2

CASES = []     # (id, op, params)
RAISES = []    # (id, op, params): the launcher must refuse


def _c(cid, op, **p):
    p.setdefault("B", B)
    CASES.append((cid, op, p))


_AB = [(a, b) for b in (False, True) for a in V.ACTS]     # the twelve (activation, bias) pairs
n = 0
for W in (4, 8, 12):
    for H in (1, 5):
        for C in (4, 36, 64):
            a, b = _AB[n % 12]
            n += 1
            _c(f"dw3-strip-{H}x{W}-c{C}-{a}-b{int(b)}", "dwconv", C=C, H=H, W=W, k=3, act=a, bias=b)
for n, (a, b) in enumerate(_AB):
    C, H = ((36, 5), (4, 1), (64, 5), (4, 5), (36, 1), (64, 1))[n % 6]
    _c(f"dw3-nhwc-{H}x7-c{C}-{a}-b{int(b)}", "dwconv", C=C, H=H, W=7, k=3, act=a, bias=b)
for n, a in enumerate(V.ACTS):
    _c(f"dw3-gen-5x8-c36-{a}-b{n % 2}", "dwconv", C=36, H=5, W=8, k=3, act=a, bias=bool(n % 2), misalign=True)
_c("dw3-stride", "dwconv", C=36, H=5, W=8, k=3, act="relu6", bias=True, xpad=8, ypad=12)
for fmt in ("b3", "h8", "f3"):
    for C in (36, 64):
        _c(f"dw3-pl-strip-{fmt}-c{C}", "dwconv", C=C, H=5, W=8, k=3, act="gelu", bias=True, planes=fmt)
        _c(f"dw3-pl-nhwc-{fmt}-c{C}", "dwconv", C=C, H=5, W=7, k=3, act="relu6", bias=False, planes=fmt)
        _c(f"dw3-pl-gen-{fmt}-c{C}", "dwconv", C=C, H=5, W=8, k=3, act="none", bias=True, planes=fmt, misalign=True)
    _c(f"dw3-pl-only-{fmt}", "dwconv", C=36, H=5, W=8, k=3, act="gelu", bias=True, planes=fmt, no_y=True)
_c("dw5-none", "dwconv", C=36, H=5, W=7, k=5, act="none", bias=True)
_c("dw5-gelu", "dwconv", C=36, H=5, W=7, k=5, act="gelu", bias=False)
_c("dw7-gelu", "dwconv", C=32, H=9, W=15, k=7, act="gelu", bias=True)
for H, W, C in ((8, 8, 32), (9, 15, 32), (1, 1, 32), (9, 15, 96)):
    _c(f"dw7-tiled-{H}x{W}-c{C}", "dwconv", C=C, H=H, W=W, k=7, act="none", bias=True)
for H, W in ((16, 16), (32, 16)):
    for C in (32, 96):
        _c(f"dw7-blk-{H}x{W}-c{C}", "dwconv", C=C, H=H, W=W, k=7, act="none", bias=C == 32)
_c("dw7-blk-ipg", "dwconv", C=32, H=16, W=16, k=7, act="none", bias=True, ipg=1)
_c("dw7-tiled-ipg", "dwconv", C=64, H=8, W=8, k=7, act="none", bias=True, ipg=1)
for fmt in ("b3", "h8", "f3"):
    _c(f"dw7-pl-{fmt}", "dwconv", C=64, H=8, W=16, k=7, act="none", bias=True, planes=fmt)
_c("dw7-pl-gen", "dwconv", C=32, H=8, W=8, k=7, act="none", bias=True, planes="b3")
RAISES.append(("dw3-ipg-refused", "dwconv", dict(B=B, C=36, H=5, W=8, k=3, act="none", bias=True, ipg=1)))

for co in (3, 6, 9, 12, 18, 24, 36, 72):
    _c(f"gc1-t{co}", "gconv", G=4, cin_g=co // 3, cout_g=co, H=5, W=7, k=1, act="none")
for co in (3, 6, 9, 12):
    _c(f"gc3-t{co}", "gconv", G=4, cin_g=co, cout_g=co, H=5, W=7, k=3, act="none")
_c("gc3-t9-17x18", "gconv", G=3, cin_g=9, cout_g=9, H=17, W=18, k=3, act="none")
for co in (18, 40, 72):
    _c(f"gc3-mfma{co}", "gconv", G=2, cin_g=co, cout_g=co, H=5, W=7, k=3, act="none")
_c("gc3-mfma18-17x18", "gconv", G=3, cin_g=10, cout_g=18, H=17, W=18, k=3, act="none")
_c("gc3-gen50", "gconv", G=2, cin_g=5, cout_g=50, H=5, W=7, k=3, act="none")
_c("gc3-gen81", "gconv", G=2, cin_g=3, cout_g=81, H=5, W=7, k=3, act="none")
_c("gc1-gen5", "gconv", G=4, cin_g=3, cout_g=5, H=5, W=7, k=1, act="none")
_c("gc3-gen5", "gconv", G=4, cin_g=3, cout_g=5, H=5, W=7, k=3, act="none")
for a in ("gelu", "sigmoid", "hswish", "relu"):
    _c(f"gc3-gen-bias-{a}", "gconv", G=4, cin_g=9, cout_g=9, H=5, W=7, k=3, act=a, bias=True)
_c("gc5-gen", "gconv", G=4, cin_g=3, cout_g=6, H=5, W=7, k=5, act="none")
for W in (3, 4, 9):
    _c(f"gc3-pair-w{W}", "gconv", G=8, cin_g=2, cout_g=2, H=5, W=W, k=3, act="none")
_c("gc3-pair-oddG", "gconv", G=7, cin_g=2, cout_g=2, H=5, W=4, k=3, act="none")

for ci, G in ((3, 8), (6, 4), (12, 2), (24, 1), (3, 16)):
    _c(f"gfe-ci{ci}-g{G}-5x7", "gfe_qkv", G=G, cin_g=ci, cout_g=3 * ci, H=5, W=7, covered=True)
_c("gfe-ci6-g4-17x18", "gfe_qkv", G=4, cin_g=6, cout_g=18, H=17, W=18, covered=True)
_c("gfe-ci9-declined", "gfe_qkv", G=8, cin_g=9, cout_g=27, H=5, W=7, covered=False)
_c("gfe-c36-declined", "gfe_qkv", G=12, cin_g=3, cout_g=9, H=5, W=7, covered=False)

_HW = ((1, 1), (1, 9), (7, 1), (10, 14))
for C in (4, 36, 64, 100):
    for H, W in _HW + ((5, 8),):
        _c(f"gate-{H}x{W}-c{C}", "dwpair_gate", C=C, H=H, W=W)
    for H, W in _HW:
        _c(f"ca-{H}x{W}-c{C}", "ca_apply", C=C, H=H, W=W)
        _c(f"gg-{H}x{W}-c{C}", "gelu_gate", C=C, H=H, W=W)
        _c(f"pool-{H}x{W}-c{C}", "pool_hw", C=C, H=H, W=W)
_c("pool-c6", "pool_hw", C=6, H=10, W=14)

for C in (32, 96):
    for HW in (1, 63, 480, 4097):
        for wr in (False, True):
            for z in (False, True):
                _c(f"cs-c{C}-hw{HW}-w{int(wr)}-z{int(z)}", "colstats", C=C, HW=HW, wrow=wr, out_is_zero=z)
        _c(f"lnhw-c{C}-hw{HW}", "lnhw", C=C, HW=HW)
    for HW in (1, 63, 480, 4097):        # HW = 1: the variance is exactly 0, rstd = 1 / sqrt(1e-5), avg collapses to mean_b
        _c(f"ffrm-c{C}-hw{HW}", "ffrm", C=C, HW=HW)

for P in (1, 255, 256, 257, 1500):
    for c in (8, 12, 80, 768):
        for nblk in (1, 8):
            if c % nblk:
                if P == 1:
                    RAISES.append((f"gram-p{P}-c{c}-n{nblk}-refused", "gram", dict(B=B, P=P, c=c, nblk=nblk)))
                continue
            _c(f"gram-p{P}-c{c}-n{nblk}", "gram", P=P, c=c, nblk=nblk)
for c in (32, 80, 96):
    _c(f"chan-c{c}", "chanattn", c=c, heads=8)
    _c(f"gffm-c{c}", "gffm", c=c)

for sc, (hx, wx) in ((4, (3, 5)), (2, (4, 6)), (1, (5, 7)), (0.5, (6, 10))):
    _c(f"tail-x{sc}", "tail", C=96, Hx=hx, Wx=wx, Hc=int(hx * sc), Wc=int(wx * sc), xtok=True)
_c("tail-noxtok", "tail", C=96, Hx=4, Wx=6, Hc=8, Wc=12, xtok=False)
_c("tail-c6", "tail", C=6, Hx=4, Wx=6, Hc=8, Wc=12, xtok=True)
for C in (32, 96):
    _c(f"tail-pl-c{C}", "tail", C=C, Hx=4, Wx=6, Hc=8, Wc=12, xtok=True, planes=True)
_c("tail-pl-narrow-c32", "tail", C=32, Hx=4, Wx=6, Hc=8, Wc=12, xtok=True, planes=True, misalign=True)
for n, C in enumerate((8, 36, 64)):
    for m, HW in enumerate((1, 35, 4096)):        # image / row stride: dense, + 4, + 3 floats; HW = 4096 meets all three (C = 36, 64, 8)
        _c(f"n2p-c{C}-hw{HW}", "nchw_to_planes", C=C, HW=HW, pad=(0, 4, 3)[(n + m) % 3])
        _c(f"t2n-c{C}-hw{HW}", "tokens_to_nchw", C=C, HW=HW, pad=(0, 4, 3)[(n + m) % 3])
for C in (8, 40):
    _c(f"head-c{C}", "head_fuse", C=C, sizes=((8, 12), (4, 6), (2, 3), (16, 24)))
del n

# ---- layernorm_rows: each C with the instantiation it selects (variant_ref.ln_variant), rows below one workgroup's and with a ragged last workgroup
_LN_C = (4, 8, 36, 96, 128, 132, 256, 260, 384, 512, 516, 1024, 1028, 2048, 2052, 4096)
for n, (C, rows) in enumerate((C, rows) for C in _LN_C for rows in (1, 7, 9)):
    _c(f"ln-c{C}-r{rows}", "layernorm_rows", C=C, rows=rows, eps=(1e-6, 1e-5)[n % 2])
for n, (C, rows) in enumerate([(C, rows) for rows in (4099, 8197) for C in (8, 96, 132, 260, 516)] + [(4096, 4099)]):      # the streamed walk: 2 / 4 rows per slot
    _c(f"ln-stream-c{C}-r{rows}", "layernorm_rows", C=C, rows=rows, eps=(1e-6, 1e-5)[n % 2])
_FMTS = ("b3", "h8", "f3", "h8c")
for C in (36, 100, 96, 64):            # 36, 100: C % 8 != 0 (store_planes4 / h8c_store4); 96: pad columns up to 128; rows = 7: an odd last row pair
    _c(f"ln-out-y2-c{C}", "layernorm_rows", C=C, rows=7, eps=1e-6, y2=True)
    for fmt in _FMTS:
        _c(f"ln-out-y-{fmt}-c{C}", "layernorm_rows", C=C, rows=7, eps=1e-6, planes=fmt)
        _c(f"ln-out-only-{fmt}-c{C}", "layernorm_rows", C=C, rows=7, eps=1e-5, planes=fmt, no_y=True)
_c("ln-out-y-h8c-c64-r8", "layernorm_rows", C=64, rows=8, eps=1e-6, planes="h8c")
for C in (36, 260):
    _c(f"ln-stride-c{C}", "layernorm_rows", C=C, rows=9, eps=1e-6, y2=True, xpad=8, ypad=12)
for H, W in ((2, 2), (4, 6)):
    _c(f"ln-patch-{H}x{W}-c36", "layernorm_rows", C=36, rows=B * H * W, eps=1e-6, patchify=(H, W))
    _c(f"ln-patch-{H}x{W}-c32-b3", "layernorm_rows", C=32, rows=B * H * W, eps=1e-6, patchify=(H, W), planes="b3")
    _c(f"ln-patch-{H}x{W}-c64-h8", "layernorm_rows", C=64, rows=B * H * W, eps=1e-5, patchify=(H, W), planes="h8")
_c("ln-grp5-c96", "layernorm_rows", C=96, rows=10, eps=1e-6, group_rows=5)                       # the two halves of one wave in different groups
_c("ln-grp5-wrap-c96", "layernorm_rows", C=96, rows=10, eps=1e-6, group_rows=5, wrap=True, gcol=96)
for C in (96, 132):
    _c(f"ln-grp300-wrap-c{C}", "layernorm_rows", C=C, rows=600, eps=1e-6, group_rows=300, wrap=True, gcol=C)
    _c(f"ln-grp300-c{C}", "layernorm_rows", C=C, rows=600, eps=1e-5, group_rows=300)
_c("ln-grp300-wrap-c96-b3", "layernorm_rows", C=96, rows=600, eps=1e-6, group_rows=300, wrap=True, gcol=96, planes="b3")
for C in (96, 260):                                                                              # a slot crosses the group boundary in mid-walk: the weight reload
    _c(f"ln-grp2050-c{C}", "layernorm_rows", C=C, rows=4100, eps=1e-6, group_rows=2050)
_c("ln-grp-patch-4x6-c36", "layernorm_rows", C=36, rows=B * 24, eps=1e-6, group_rows=24, patchify=(4, 6))
_c("ln-grp-patch-4x6-c32-b3", "layernorm_rows", C=32, rows=B * 24, eps=1e-6, group_rows=24, patchify=(4, 6), planes="b3")
# the clamp watch: |y| beyond 57344 with h8 planes leaves the largest |y| in the word; ordinary magnitudes, or bf16 hi/lo planes, leave 0
_c("ln-cw-h8-big", "layernorm_rows", C=96, rows=9, eps=1e-6, planes="h8", wscale=1e5, cw=True)
_c("ln-cw-h8", "layernorm_rows", C=96, rows=9, eps=1e-6, planes="h8", cw=True)
_c("ln-cw-b3-big", "layernorm_rows", C=96, rows=9, eps=1e-6, planes="b3", wscale=1e5, cw=True)
_c("ln-cw-b3", "layernorm_rows", C=96, rows=9, eps=1e-6, planes="b3", cw=True)
for cid, kw in (("ln-oddH-refused", dict(C=36, rows=B * 18, patchify=(3, 6))), ("ln-y2-patch-refused", dict(C=36, rows=B * 4, patchify=(2, 2), y2=True)),
                ("ln-patch-c36-planes-refused", dict(C=36, rows=B * 4, patchify=(2, 2), planes="b3")),
                ("ln-h8c-patch-refused", dict(C=64, rows=B * 4, patchify=(2, 2), planes="h8c")),
                ("ln-h8c-grp-refused", dict(C=64, rows=10, group_rows=5, planes="h8c")),
                ("ln-h8c-ldp-refused", dict(C=64, rows=8, planes="h8c", short_ldp=True)),
                ("ln-c6-refused", dict(C=6, rows=9)), ("ln-c4100-refused", dict(C=4100, rows=9)),
                ("ln-grp-rows-refused", dict(C=96, rows=11, group_rows=5))):
    RAISES.append((cid, "layernorm_rows", dict(B=B, eps=1e-6, **kw)))

for rows in (1, 255, 257):
    for strips in (1, 2, 16):
        _c(f"rs-r{rows}-s{strips}", "rowstats", rows=rows, strips=strips, eps=(1e-6, 1e-5)[strips % 2])
RAISES.append(("rs-d100-refused", "rowstats", dict(B=B, rows=9, strips=1, eps=1e-6, D=100)))

# ---- MSDA: non-square levels throughout.  Workgroups of the fp32 vector kernel = ceil(B Lq M (D / 4) / block), block = (256 / (D / 4)) (D / 4):
#        D = 32, M = 4 (block 256): Lq = 4 / 27 / 32 / 33 / 67 -> 1 / 7 / 8 / 9 / 17 workgroups (mmsa_xcd_order permutes the first 8 * (grid / 8))
#        D = 40, M = 4 (block 250): Lq = 3 / 26 -> 1 / 9          D = 4 / 8 / 64, M = 4, Lq = 33 -> 2 / 3 / 17          D = 12, M = 3, Lq = 33 -> 3
_LV2, _LV3 = ((5, 7), (3, 2)), ((9, 7), (5, 4), (2, 3))
for n, Lq in enumerate((4, 27, 32, 33, 67)):
    _c(f"msda-d32-q{Lq}", "msda", levels=(_LV2, _LV3)[n % 2], P=(3, 4)[n % 2], M=4, D=32, Lq=Lq)
for n, (D, M, Lq) in enumerate(((4, 4, 33), (8, 4, 33), (12, 3, 33), (64, 4, 33), (40, 4, 3), (40, 4, 26))):
    _c(f"msda-d{D}-q{Lq}", "msda", levels=(_LV3, _LV2)[n % 2], P=(4, 3)[n % 2], M=M, D=D, Lq=Lq)
_c("msda-scalar-d2", "msda", levels=_LV2, P=4, M=3, D=2, Lq=33)
_c("msda-scalar-d6", "msda", levels=_LV3, P=3, M=3, D=6, Lq=33)
_c("msda-scalar-d32-misaligned", "msda", levels=_LV2, P=4, M=4, D=32, Lq=33, misalign=True)
for dtn in ("f16", "f64"):
    _c(f"msda-scalar-{dtn}-d2", "msda", levels=_LV3, P=4, M=3, D=2, Lq=33, dtype=dtn)
    _c(f"msda-scalar-{dtn}-d32", "msda", levels=_LV2, P=3, M=4, D=32, Lq=33, dtype=dtn)
_DY = ((4, 8), (2, 4))
_c("msda-dyadic-fwd", "msda", levels=_DY, P=4, M=2, D=8, Lq=33, dyadic=True)
_c("msda-dyadic-fwd-scalar", "msda", levels=_DY, P=4, M=2, D=2, Lq=33, dyadic=True)
_c("msda-dyadic-fused", "msda_fused", levels=_DY, P=4, M=2, D=8, Lq=33, dyadic=True)
_c("msda-dyadic-fused-h8", "msda_fused", levels=_DY, P=4, M=4, D=8, Lq=33, dyadic=True, value="h8", lo_bytes=True)
for n, (M, D) in enumerate(((4, 4), (3, 12), (4, 8), (4, 32), (4, 40), (3, 32))):      # D = 4, 12: store_planes4_any; 8, 32, 40: the pair store; M D = 96: h8c pads to 128
    kw = dict(levels=(_LV2, _LV3)[n % 2], P=(3, 4)[n % 2], M=M, D=D, Lq=(33, 26)[n % 2])
    _c(f"msdaf-m{M}d{D}", "msda_fused", **kw)
    for fmt in _FMTS:
        _c(f"msdaf-m{M}d{D}-{fmt}", "msda_fused", planes=fmt, **kw)
    _c(f"msdaf-m{M}d{D}-only-{_FMTS[n % 4]}", "msda_fused", planes=_FMTS[n % 4], no_y=True, **kw)
_c("msdaf-m3d32-only-h8c", "msda_fused", levels=_LV2, P=3, M=3, D=32, Lq=33, planes="h8c", no_y=True)
_c("msdaf-stride", "msda_fused", levels=_LV3, P=4, M=4, D=8, Lq=33, rawpad=5, opad=12)
for n, (M, D) in enumerate(((4, 8), (2, 32), (3, 64), (1, 32))):                          # the gather on H8 value planes, both lo_bytes settings
    for lo in (False, True):
        kw = dict(levels=(_LV3, _LV2)[n % 2], P=(4, 3)[n % 2], M=M, D=D, Lq=33, value="h8", lo_bytes=lo)
        _c(f"msdap-m{M}d{D}-lo{int(lo)}", "msda_fused", **kw)
        for fmt in _FMTS:
            _c(f"msdap-m{M}d{D}-lo{int(lo)}-{fmt}", "msda_fused", planes=fmt, **kw)
        _c(f"msdap-m{M}d{D}-lo{int(lo)}-only-{_FMTS[(n + lo) % 4]}", "msda_fused", planes=_FMTS[(n + lo) % 4], no_y=True, **kw)
_c("msdap-stride", "msda_fused", levels=_LV3, P=4, M=4, D=8, Lq=33, value="h8", lo_bytes=True, rawpad=5, opad=12)
_c("msdaf-cw-h8c-big", "msda_fused", levels=_LV2, P=3, M=3, D=32, Lq=33, planes="h8c", vscale=1e5, cw=True)
_c("msdaf-cw-h8c", "msda_fused", levels=_LV2, P=3, M=3, D=32, Lq=33, planes="h8c", cw=True)
_c("msdaf-cw-b3-big", "msda_fused", levels=_LV2, P=3, M=3, D=32, Lq=33, planes="b3", vscale=1e5, cw=True)
_c("msdaf-cw-b3", "msda_fused", levels=_LV2, P=3, M=3, D=32, Lq=33, planes="b3", cw=True)
_KW = dict(B=B, levels=_LV2, P=3, Lq=9)
RAISES += [("msdaf-d6-refused", "msda_fused", dict(M=4, D=6, **_KW)), ("msdap-md48-refused", "msda_fused", dict(M=2, D=24, value="h8", lo_bytes=False, **_KW)),
           ("msdaf-ldraw-refused", "msda_fused", dict(M=4, D=8, short_raw=True, **_KW)), ("msdaf-b3-value-refused", "msda_fused", dict(M=4, D=8, value="b3", **_KW)),
           ("msda-batch3-step2-refused", "msda", dict(M=4, D=8, batch=3, im2col_step=2, **_KW)),
           ("msdaf-value-strided-refused", "msda_fused", dict(M=4, D=8, value_slice=True, **_KW)),
           ("msdaf-value-rows-refused", "msda_fused", dict(M=4, D=8, value_short=True, **_KW))]
# ---- MSDA backward: one lane per (b, q, m, c), 256 lanes per workgroup; SHFL = D a power of two <= 64 (variant_ref.msda_bwd_shfl)
for n, (D, M, Lq) in enumerate(((1, 3, 33), (2, 3, 33), (8, 3, 33), (32, 3, 33), (64, 3, 33), (16, 4, 32))):      # <float, true>; lanes = 198, 396, 1584, 6336, 12672, 4096
    _c(f"msdab-f32-shfl-m{M}d{D}-q{Lq}", "msda_bwd", levels=(_LV2, _LV3)[n % 2], P=(3, 4)[n % 2], M=M, D=D, Lq=Lq)
for n, (D, M, Lq) in enumerate(((3, 3, 33), (12, 3, 33), (40, 4, 26), (128, 2, 9))):                             # <float, false>
    _c(f"msdab-f32-atom-m{M}d{D}-q{Lq}", "msda_bwd", levels=(_LV3, _LV2)[n % 2], P=(4, 3)[n % 2], M=M, D=D, Lq=Lq)
for dtn, d_atom in (("f64", 6), ("f16", 3)):                                                                      # <double | __half, true | false>
    for n, (D, M, Lq) in enumerate(((2, 3, 33), (32, 3, 33), (d_atom, 3, 33), (40, 4, 26))):
        _c(f"msdab-{dtn}-{('shfl', 'atom')[n // 2]}-m{M}d{D}-q{Lq}", "msda_bwd", levels=(_LV2, _LV3)[n % 2], P=(3, 4)[n % 2], M=M, D=D, Lq=Lq, dtype=dtn)
_c("msdab-dyadic-shfl-m2d8-q33", "msda_bwd", levels=_DY, P=4, M=2, D=8, Lq=33, dyadic=True)
_c("msdab-dyadic-atom-m2d6-q33", "msda_bwd", levels=_DY, P=4, M=2, D=6, Lq=33, dyadic=True)
_KW = dict(B=B, levels=_LV2, P=3, Lq=9, M=4, D=8)
RAISES += [("msdab-batch3-step2-refused", "msda_bwd", dict(refuse="step", batch=3, im2col_step=2, **_KW)),
           ("msdab-gout-shape-refused", "msda_bwd", dict(refuse="gout-shape", **_KW)), ("msdab-gout-dtype-refused", "msda_bwd", dict(refuse="gout-dtype", **_KW)),
           ("msdab-gout-strided-refused", "msda_bwd", dict(refuse="gout-strided", **_KW)), ("msdab-bf16-refused", "msda_bwd", dict(refuse="bf16", **_KW))]
del n, kw, _KW

assert len({c[0] for c in CASES}) == len(CASES)


@pytest.fixture(scope="module")
def ops():
    import mmsa
    return mmsa.ops


def dev(t):
    return t.contiguous().to(DEV)


def nanbuf(*shape, dtype=torch.float32):
    return torch.full(shape, NAN, dtype=dtype, device=DEV)


def bits(t):
    t = t.contiguous()
    return t.view({2: torch.int16, 4: torch.int32, 8: torch.int64}[t.element_size()])


def fmt_of(ops, name):
    return {"b3": ops.FMT_B3, "h8": ops.FMT_H8, "f3": ops.FMT_F3, "h8c": ops.FMT_H8C}[name]


def planes_equal_split(ops, pl, y, fmt):
    """The planes a launch wrote next to its fp32 output are split_planes of that output, bit for bit over the whole buffer (pad columns: zero)."""
    want = ops.split_planes(y.contiguous(), out=ops.alloc_planes(y.shape[0], y.shape[1], DEV, zero=True, fmt=fmt))
    torch.cuda.synchronize()
    assert pl.p.shape == want.p.shape
    assert torch.equal(pl.p, want.p), "planes differ from split_planes of the same launch's fp32 output"
    assert pads_zero(ops, pl)


def pads_zero(ops, pl):
    """Every 16-bit word / byte that belongs to a column >= k of the planes is zero."""
    k, kp = pl.k, pl.kpad
    if pl.fmt == ops.FMT_H8C:
        return h8c_untouched_zero(pl)
    if k == kp:
        return True
    by = pl.p.contiguous().view(torch.uint8).view(pl.p.shape[0], kp // 32, 128)
    cols = torch.arange(32 * (k // 32), kp)
    blk, c = cols // 32, cols % 32
    if pl.fmt == ops.FMT_H8:
        lo = 64 + (c // 8) * 16 + c % 8
        offs = [2 * c, 2 * c + 1, lo, lo + 8]
    else:
        offs = [2 * c, 2 * c + 1, 64 + 2 * c, 64 + 2 * c + 1]
    keep = cols >= k
    return all(bool((by[:, blk[keep], o[keep]] == 0).all()) for o in offs)


def h8c_untouched_zero(pl):
    """Row-pair planes (csrc/common.h h8c_row / h8c_lo_off): pair j = [row 2j: kpad fp16 hi][row 2j+1: kpad fp16 hi][kpad / 64 lines of 128 lo bytes: row 2j's
    64 | row 2j+1's 64], the lo byte of column c of a chunk at ((c & 31) >> 3) * 16 + ((c >> 5) & 1) * 8 + (c & 7).  Everything that belongs to a column
    >= k, whatever lies beyond 3 * kpad in a pair, and the unused half of a last odd row pair must be as initialised: zero."""
    k, kp, n = pl.k, pl.kpad, pl.n
    pairs = pl.p.shape[0]
    ok = bool((pl.p[:, 3 * kp:] == 0).all())
    by = pl.p[:, :3 * kp].contiguous().view(torch.uint8).view(pairs, 6 * kp)
    hi = by[:, :4 * kp].contiguous().view(torch.int16).view(pairs, 2, kp)
    lo = by[:, 4 * kp:].view(pairs, kp // 64, 2, 64)
    if k < kp:
        cols = torch.arange(k, kp)
        c = cols % 64
        ok = ok and bool((hi[:, :, k:] == 0).all()) and bool((lo[:, cols // 64, :, ((c & 31) >> 3) * 16 + ((c >> 5) & 1) * 8 + (c & 7)] == 0).all())
    if n % 2:
        ok = ok and bool((hi[-1, 1] == 0).all()) and bool((lo[-1, :, 1] == 0).all())
    return ok


# ------------------------------------------------------------------------------------------------ runners: one launch into fresh NaN-filled outputs
# each returns dict(y = fp32 result in the reference's layout or None, raw = every buffer the launch wrote (compared bit for bit between two runs),
# planes = (Planes, format) written next to y, or decoded = fp32 decode of a planes-only output)
def run_dwconv(ops, i, p):
    Bn, C, H, W, k = p["B"], p["C"], p["H"], p["W"], p["k"]
    hwc = H * W * C
    xs, ys = hwc + p.get("xpad", 0), hwc + p.get("ypad", 0)
    off = 1 if p.get("misalign") else 0
    xbuf = nanbuf(off + Bn * xs + 3)
    xbuf[off:off + Bn * xs].view(Bn, xs)[:, :hwc] = dev(V.nhwc(i["x"]).view(Bn, hwc))
    w = dev(i["w"].reshape(-1, C, k * k).transpose(1, 2))          # [groups][tap][C]
    b = dev(i["b"]) if "b" in i else None
    ybuf = None if p.get("no_y") else nanbuf(Bn * ys)
    pl = ops.alloc_planes(Bn * H * W, C, DEV, zero=True, fmt=fmt_of(ops, p["planes"])) if p.get("planes") else None
    ops.dwconv(xbuf[off:off + hwc].view(H * W, C), w, b, None if ybuf is None else ybuf[:hwc].view(H * W, C), Bn, H, W, k, act=p["act"],
               xstride_b=xs, ystride_b=ys, out_planes=pl, imgs_per_group=p.get("ipg", 0))
    out = dict(raw=[t for t in (ybuf, pl.p if pl else None) if t is not None])
    if ybuf is not None:
        out["y"] = ybuf.view(Bn, ys)[:, :hwc].reshape(Bn * H * W, C)
        assert bool(torch.isnan(ybuf.view(Bn, ys)[:, hwc:]).all()), "the gap between two images was written"
        if pl:
            out["planes"] = (pl, pl.fmt)
    else:
        out["decoded"] = (ops.planes_to_float(pl), V.FMT_REL[p["planes"]])
        assert pads_zero(ops, pl)
    return out


def run_gconv(ops, i, p):
    Bn, G, ci, co, H, W, k = p["B"], p["G"], p["cin_g"], p["cout_g"], p["H"], p["W"], p["k"]
    w = dev(i["w"].reshape(G, co, ci, k * k).permute(0, 3, 2, 1))   # [g][tap][ci][co]
    y = nanbuf(Bn * H * W, G * co)
    ops.gconv(dev(V.nhwc(i["x"])), w, dev(i["b"]) if "b" in i else None, y, Bn, H, W, G, ci, co, k, act=p["act"])
    return dict(y=y, raw=[y])


def run_gfe_qkv(ops, i, p):
    from mmsa.backbone import fold_gfe_qkv
    Bn, G, ci, co, H, W = p["B"], p["G"], p["cin_g"], p["cout_g"], p["H"], p["W"]
    if co == 3 * ci:
        w12 = dev(fold_gfe_qkv(i["q1"], i["q2"], groups=G))
    else:
        w12 = torch.zeros(G, 9, ci, co, device=DEV)
    y = nanbuf(Bn * H * W, G * co)
    covered = ops.gfe_qkv(dev(V.nhwc(i["x"])), w12, y, Bn, H, W, G, ci, co)
    torch.cuda.synchronize()
    assert covered == p["covered"]
    if not covered:
        assert bool(torch.isnan(y).all()), "a declined call wrote to its output"
        return dict(y=None, raw=[y])
    return dict(y=y, raw=[y])


def run_dwpair_gate(ops, i, p):
    Bn, C, H, W = p["B"], p["C"], p["H"], p["W"]
    w = dev(i["w"].reshape(C, 2, 2, 9).permute(3, 0, 2, 1))          # [tap][group][ci][co]
    y = nanbuf(Bn * H * W, C)
    pl = ops.alloc_planes(Bn * H * W, C, DEV, zero=True)
    ops.dwpair_gate(dev(V.nhwc(i["x"])), w, y, Bn, H, W, C, out_planes=pl)
    return dict(y=y, raw=[y, pl.p], planes=(pl, ops.FMT_B3))


def run_ca_apply(ops, i, p):
    Bn, C, H, W = p["B"], p["C"], p["H"], p["W"]
    y = nanbuf(Bn * H * W, C)
    pl = ops.alloc_planes(Bn * H * W, C, DEV, zero=True)
    ops.ca_apply(dev(i["z"]), dev(i["att"]), y, Bn, H, W, out_planes=pl)
    return dict(y=y, raw=[y, pl.p], planes=(pl, ops.FMT_B3))


def run_gelu_gate(ops, i, p):
    y = nanbuf(i["x"].shape[0], p["C"])
    ops.gelu_gate(dev(i["x"]), y, p["C"])
    return dict(y=y, raw=[y])


def run_pool_hw(ops, i, p):
    y = nanbuf(p["B"] * (p["H"] + p["W"]), p["C"])
    ops.pool_hw(dev(i["z"]), y, p["B"], p["H"], p["W"])
    return dict(y=y, raw=[y])


def run_colstats(ops, i, p):
    Bn, C, HW = p["B"], p["C"], p["HW"]
    st = torch.zeros(Bn * 3, C, dtype=torch.float64, device=DEV) if p["out_is_zero"] else nanbuf(Bn * 3, C, dtype=torch.float64)
    ops.colstats(dev(i["x"]), HW * C, Bn, HW, st, wrow=dev(i["wrow"]) if "wrow" in i else None, out_is_zero=p["out_is_zero"])
    return dict(y=st, raw=[st])


def run_ffrm(ops, i, p):
    Bn, C, HW = p["B"], p["C"], p["HW"]
    o = nanbuf(3 * Bn, C)
    ops.ffrm_finalize(dev(i["stats"]), Bn, HW, C, i["mean_w"], i["mean_b"], dev(i["wc"]), dev(i["gn_w"]), dev(i["gn_b"]),
                      o[:Bn], o[Bn:2 * Bn], o[2 * Bn:], nanbuf(2 * Bn, C))
    return dict(y=o, raw=[o])


def run_lnhw(ops, i, p):
    y = nanbuf(p["B"] * p["HW"], p["C"])
    ops.lnhw_apply(dev(i["x"]), dev(i["mean"]), dev(i["rstd"]), dev(i["mult"]), dev(i["w"]), dev(i["b"]), y, p["B"], p["HW"])
    return dict(y=y, raw=[y])


def run_gram(ops, i, p):
    Bn, P, c, nblk = p["B"], p["P"], p["c"], p["nblk"]
    xy = dev(i["xy"])
    g = nanbuf(Bn * c, c, dtype=torch.float64)
    need = ops.gram_tn_scratch_bytes(Bn, P, c)
    assert need % 4 == 0
    ops.gram_tn(xy[:, :c], xy[:, c:], P * 2 * c, g, Bn, P, nblk=nblk, scratch=nanbuf(need // 4))    # exactly the bytes asked for
    return dict(y=g, raw=[g], mask=V.gram_mask(c, nblk).repeat(Bn, 1))


def run_chanattn(ops, i, p):
    Bn, c, heads = p["B"], p["c"], p["heads"]
    cpad = ops.pad32(c)
    pl = ops.Planes(torch.zeros(Bn * c, 2 * cpad, dtype=torch.int16, device=DEV), Bn * c, c, cpad)
    sq, sk = dev(i["sq"]), dev(i["sk"])
    ops.chanattn_build(dev(i["G"]), sq.data_ptr(), c, sk.data_ptr(), c, dev(i["temp"]), dev(i["wp"]), pl, Bn, c, heads)
    torch.cuda.synchronize()
    assert pads_zero(ops, pl)
    return dict(y=None, raw=[pl.p], decoded=(ops.planes_to_float(pl), None))


def run_gffm(ops, i, p):
    Bn, c = p["B"], p["c"]
    cpad = ops.pad32(c)
    px, py = (ops.Planes(torch.zeros(Bn * c, 2 * cpad, dtype=torch.int16, device=DEV), Bn * c, c, cpad) for _ in range(2))
    ops.gffm_build(dev(i["E"]), px, py, Bn, c)
    torch.cuda.synchronize()
    assert pads_zero(ops, px) and pads_zero(ops, py)
    return dict(y=None, raw=[px.p, py.p], decoded=(torch.cat([ops.planes_to_float(px), ops.planes_to_float(py)]), None))


def run_tail(ops, i, p):
    Bn, C, Hc, Wc = p["B"], p["C"], p["Hc"], p["Wc"]
    y = nanbuf(Bn, C, Hc, Wc)
    pl = ops.alloc_planes(Bn * Hc * Wc, C, DEV, zero=True) if p.get("planes") else None
    cm = dev(V.nhwc(i["cm"]))
    if p.get("misalign"):                         # the map starts one float past a 16-byte boundary
        buf = nanbuf(1 + cm.numel() + 3)
        buf[1:1 + cm.numel()] = cm.flatten()
        cm = buf[1:1 + cm.numel()].view(cm.shape)
    ops.tail_fuse(cm, Hc * Wc * C, dev(V.nhwc(i["xt"])) if "xt" in i else None, dev(i["scale"]), dev(i["shift"]), y,
                  Bn, Hc, Wc, p["Hx"], p["Wx"], out_planes=pl)
    out = dict(y=y, raw=[y] + ([pl.p] if pl else []))
    if pl:
        out["planes"] = (pl, ops.FMT_B3)
        out["planes_src"] = V.nhwc(y)
    return out


def run_nchw_to_planes(ops, i, p):
    from mmsa import lib
    Bn, C, HW = p["B"], p["C"], p["HW"]
    sb = C * HW + p["pad"]
    src = nanbuf(Bn, sb)
    src[:, :C * HW] = dev(i["x"].reshape(Bn, C * HW))
    pl = ops.alloc_planes(Bn * HW, C, DEV, zero=True)
    lib.call("mmsa_nchw_to_planes", src.data_ptr(), sb, pl.p.data_ptr(), 2 * pl.kpad, Bn, C, HW, ops._stream())
    torch.cuda.synchronize()
    planes_equal_split(ops, pl, dev(i["x"].permute(0, 2, 1).reshape(Bn * HW, C)), ops.FMT_B3)     # a pure layout change: the planes of the token matrix
    return dict(y=None, raw=[pl.p], decoded=(ops.planes_to_float(pl), None))


def run_tokens_to_nchw(ops, i, p):
    from mmsa import lib
    Bn, C, HW = p["B"], p["C"], p["HW"]
    ld = C + p["pad"]
    src = nanbuf(Bn * HW, ld)
    src[:, :C] = dev(i["x"])
    y = nanbuf(Bn, C, HW)
    lib.call("mmsa_tokens_to_nchw", src.data_ptr(), ld, y.data_ptr(), Bn, HW, C, ops._stream())
    return dict(y=y, raw=[y])


def run_head_fuse(ops, i, p):
    from mmsa import lib
    Bn, C, sizes = p["B"], p["C"], p["sizes"]
    ld = C + 4
    zs = []
    for l, (h, w) in enumerate(sizes):
        z = nanbuf(Bn * h * w, ld)
        z[:, :C] = dev(V.nhwc(i[f"z{l}"]))
        zs.append(z)
    (H, W) = sizes[0]
    y = nanbuf(Bn * H * W, C)
    pl = ops.alloc_planes(Bn * H * W, C, DEV, zero=True)
    sc, sh = dev(i["scale"]), dev(i["shift"])
    lib.call("mmsa_head_fuse", zs[0].data_ptr(), zs[1].data_ptr(), sizes[1][0], sizes[1][1], zs[2].data_ptr(), sizes[2][0], sizes[2][1],
             zs[3].data_ptr(), sizes[3][0], sizes[3][1], ld, sc.data_ptr(), sh.data_ptr(), pl.p.data_ptr(), 2 * pl.kpad, y.data_ptr(), C,
             Bn, H, W, C, ops.ACT["relu"], ops._stream())
    return dict(y=y, raw=[y, pl.p], planes=(pl, ops.FMT_B3))


def watch_word(ops, p):
    """(context, word): the clamp watch of a `cw` case -- a zeroed device word handed to the launch."""
    import contextlib
    if not p.get("cw"):
        return contextlib.nullcontext(), None
    word = torch.zeros(1, device=DEV)
    return ops.clamp_watch(word), word


def check_watch(p, word, y):
    """The word holds the largest |y| of the launch's fp32 output, bit for bit, when a format of fp16 range had to clamp (the `big` cases); 0 otherwise."""
    if word is None:
        return
    torch.cuda.synchronize()
    big = y.abs().max().reshape(1)
    clamps = p["planes"] in ("h8", "h8c") and float(big) > 57344.0
    assert clamps == (p["planes"] in ("h8", "h8c") and (p.get("wscale", 1) > 1 or p.get("vscale", 1) > 1)), "the case does not do what its id says"
    want = big if clamps else torch.zeros_like(big)
    assert torch.equal(bits(word), bits(want)), f"clamp watch word {float(word)!r}, expected {float(want)!r}"


def out_buffers(ops, p, rows, cols):
    """NaN-filled fp32 output (row stride cols + opad) and zero-initialised planes, as the case asks."""
    ybuf = None if p.get("no_y") else nanbuf(rows, cols + p.get("opad", p.get("ypad", 0)))
    pl = ops.alloc_planes(rows, cols, DEV, zero=True, fmt=fmt_of(ops, p["planes"])) if p.get("planes") else None
    return ybuf, pl


def finish(ops, p, ybuf, pl, cols, extra_raw=(), y_extra=None):
    out = dict(raw=[t for t in (ybuf, pl.p if pl else None) + tuple(extra_raw) if t is not None])
    if ybuf is not None:
        assert bool(torch.isnan(ybuf[:, cols:]).all()), "the gap behind an output row was written"
        y = ybuf[:, :cols]
        out["y"] = y if y_extra is None else torch.cat([y, y_extra], 1)
        if pl:
            out["planes"], out["planes_src"] = (pl, pl.fmt), y
    else:
        torch.cuda.synchronize()
        out["decoded"] = (ops.planes_to_float(pl), V.FMT_REL[p["planes"]])
        assert pads_zero(ops, pl)
    return out


def run_layernorm_rows(ops, i, p):
    rows, C, gr = p["rows"], p["C"], p.get("group_rows", 0)
    xoff, xpad = (4, p["xpad"]) if p.get("xpad") else (0, 0)
    xbuf = nanbuf(rows, C + xpad)                                    # x: a column slice of a wider NaN-filled matrix
    xbuf[:, xoff:xoff + C] = dev(i["x"])
    orows, ocols = V.ln_out_shape(p)
    ybuf, pl = out_buffers(ops, p, orows, ocols)
    if p.get("short_ldp"):                                           # a pair stride below 3 * pad64(C)
        pl = ops.Planes(torch.zeros((rows + 1) // 2, 3 * pl.kpad - 64, dtype=torch.int16, device=DEV), rows, C, pl.kpad, ops.FMT_H8C)
    y2buf = nanbuf(rows, C + p.get("ypad", 0)) if p.get("y2") else None
    ctx, word = watch_word(ops, p)
    with ctx:
        ops.layernorm(xbuf[:, xoff:xoff + C], dev(i["w"]), dev(i["b"]), p["eps"], out=None if ybuf is None else ybuf[:, :ocols],
                      out2=None if y2buf is None else y2buf[:, :C], patchify=p.get("patchify"), out_planes=pl, group_rows=gr,
                      w_gstride=C if gr else 0, y_gcol=p.get("gcol", 0), y_wrap=bool(p.get("wrap")))
    if y2buf is not None:
        assert bool(torch.isnan(y2buf[:, C:]).all()), "the gap behind a y2 row was written"
    out = finish(ops, p, ybuf, pl, ocols, extra_raw=(y2buf,), y_extra=None if y2buf is None else y2buf[:, :C])
    check_watch(p, word, ybuf[:, :ocols] if ybuf is not None else None)
    return out


def run_rowstats(ops, i, p):
    rows = p["rows"]
    o = nanbuf(rows, 2)
    ops.rowstats_finalize(dev(i["rs"].float()), rows, p.get("D", 64 * p["strips"]), p["eps"], o)
    return dict(y=o, raw=[o])


def msda_tables(p):
    levels, starts, S = V.msda_geometry(p)
    return torch.tensor(levels, dtype=torch.long, device=DEV), torch.tensor(starts, dtype=torch.long, device=DEV), S


def run_msda(ops, i, p):
    ss, lsi, S = msda_tables(p)
    dt = {"f16": torch.float16, "f64": torch.float64}.get(p.get("dtype"), torch.float32)
    nb = p.get("batch", p["B"])
    value, loc, aw = (dev(torch.cat([t] * 2)[:nb].to(dt)) for t in (i["value"], i["loc"], i["aw"]))
    if p.get("misalign"):                                            # value starts one float past a 16-byte boundary: the scalar kernel takes it
        buf = nanbuf(1 + value.numel() + 3)
        buf[1:1 + value.numel()] = value.flatten()
        value = buf[1:1 + value.numel()].view(value.shape)
        assert value.data_ptr() % 16 == 4
    y = ops.msda_forward(value, ss, lsi, loc, aw, im2col_step=p.get("im2col_step", 64))
    y = y.view(nb * p["Lq"], p["M"] * p["D"])
    return dict(y=y, raw=[y])


def run_msda_fused(ops, i, p):
    ss, lsi, S = msda_tables(p)
    Bn, M, D, Lq, P, L = p["B"], p["M"], p["D"], p["Lq"], p["P"], len(p["levels"])
    n3 = M * L * P * 3
    if p.get("value") == "h8":                                       # the planes hold the case's values exactly (variant_ref.h8_exact)
        v = dev(i["value"])
        value = ops.split_planes(v, fmt=ops.FMT_H8)
        torch.cuda.synchronize()
        assert torch.equal(bits(ops.planes_to_float(value)), bits(v)), "split_planes / planes_to_float do not return the H8-exact values"
    elif p.get("value") == "b3":
        value = ops.split_planes(dev(i["value"]), fmt=ops.FMT_B3)
    elif p.get("value_slice"):                                       # a column slice of a wider matrix: the entry has no row stride for it
        value = nanbuf(Bn * S, M * D + 4)[:, :M * D]
    elif p.get("value_short"):
        value = dev(i["value"])[:Bn * S - 1]
    else:
        value = dev(i["value"])
    rawbuf = nanbuf(Bn * Lq, n3 + p.get("rawpad", 0))
    rawbuf[:, :n3] = dev(i["raw"])
    raw = rawbuf[:, :n3 - 4].contiguous() if p.get("short_raw") else rawbuf[:, :n3]
    ybuf, pl = out_buffers(ops, p, Bn * Lq, M * D)
    ctx, word = watch_word(ops, p)
    with ctx:
        ops.msda_fused(value, ss, lsi, raw, dev(i["ref"]), None if ybuf is None else ybuf[:, :M * D], Bn, S, M, D, L, Lq, P, out_planes=pl,
                       lo_bytes=bool(p.get("lo_bytes")))
    out = finish(ops, p, ybuf, pl, M * D)
    check_watch(p, word, ybuf[:, :M * D] if ybuf is not None else None)
    return out


GUARD = 8      # elements in front of and behind every msda_bwd output: a multiple of 16 bytes for each of the three element sizes


def run_msda_bwd(ops, i, p):
    """mmsa_ms_deform_attn_backward through lib.call: the three outputs are views inside larger NaN-filled tensors, whose guard regions must stay NaN (the
    memset sizes, for every element size).  `parts`: the slices of y the ratios are printed for; `both`: the second call is held to the bound as well."""
    from mmsa import lib
    ss, lsi, S = msda_tables(p)
    Bn, M, D, Lq, P, L = p["B"], p["M"], p["D"], p["Lq"], p["P"], len(p["levels"])
    dt = {"f16": torch.float16, "f64": torch.float64}.get(p.get("dtype"), torch.float32)
    nb = p.get("batch", Bn)
    value, loc, aw, gout = (dev(torch.cat([t] * 2)[:nb].to(dt)) for t in (i["value"], i["loc"], i["aw"], i["gout"].reshape(Bn, Lq, M * D)))
    if "refuse" in p:                                                # through ops.msda_backward: the layer that refuses all but the im2col_step
        kind = p["refuse"]
        if kind == "gout-shape":
            gout = gout[:, :, :-1].contiguous()
        elif kind == "gout-dtype":
            gout = gout.double()
        elif kind == "gout-strided":
            gout = torch.cat([gout, gout], 2)[:, :, :M * D]
            assert not gout.is_contiguous()
        elif kind == "bf16":
            value, loc, aw, gout = (t.bfloat16() for t in (value, loc, aw, gout))
        return ops.msda_backward(value, ss, lsi, loc, aw, gout, im2col_step=p.get("im2col_step", 64))
    parts = V.msda_bwd_slices(p)
    bufs = [nanbuf(GUARD + s.stop - s.start + GUARD, dtype=dt) for s in parts.values()]
    outs = [b[GUARD:b.numel() - GUARD] for b in bufs]
    lib.call("mmsa_ms_deform_attn_backward", value.data_ptr(), ss.data_ptr(), lsi.data_ptr(), loc.data_ptr(), aw.data_ptr(), gout.data_ptr(),
             outs[0].data_ptr(), outs[1].data_ptr(), outs[2].data_ptr(), nb, S, M, D, L, Lq, P, 64, ops.MSDA_DTYPES[dt], ops._stream())
    torch.cuda.synchronize()
    for b, name in zip(bufs, parts):
        assert bool(torch.isnan(b[:GUARD]).all()) and bool(torch.isnan(b[-GUARD:]).all()), f"{name}: the guard region around the output was written"
    # grad_value, and everything on the atomics path, meets in float atomics whose order is free: only the shuffle path's two outputs must repeat bit for bit
    return dict(y=torch.cat(outs), raw=outs[1:] if V.msda_bwd_shfl(p) else [], parts=parts, both=True)


RUN = {"layernorm_rows": run_layernorm_rows, "rowstats": run_rowstats, "msda": run_msda, "msda_fused": run_msda_fused, "msda_bwd": run_msda_bwd, "dwconv": run_dwconv, "gconv": run_gconv, "gfe_qkv": run_gfe_qkv, "dwpair_gate": run_dwpair_gate, "ca_apply": run_ca_apply,
       "gelu_gate": run_gelu_gate, "pool_hw": run_pool_hw, "colstats": run_colstats, "ffrm": run_ffrm, "lnhw": run_lnhw, "gram": run_gram,
       "chanattn": run_chanattn, "gffm": run_gffm, "tail": run_tail, "nchw_to_planes": run_nchw_to_planes, "tokens_to_nchw": run_tokens_to_nchw,
       "head_fuse": run_head_fuse}


@pytest.mark.parametrize("cid,op,p", CASES, ids=[c[0] for c in CASES])
def test_variant(ops, cid, op, p):
    i, r, bnd = V.case_data(cid, op, p)
    first = RUN[op](ops, i, p)
    again = RUN[op](ops, i, p)
    torch.cuda.synchronize()
    for a, b in zip(first["raw"], again["raw"]):
        assert torch.equal(bits(a), bits(b)), f"{cid}: two identical calls differ in their bits"
    y = first.get("y")
    if y is not None:
        if "mask" in first:                      # only part of the output is defined (gram_tn's diagonal head blocks)
            m = first["mask"]
            y, r, bnd = torch.where(m, y.cpu(), 0.0), torch.where(m, r, 0.0), torch.where(m, bnd, 0.0)
        ratio = V.assert_inside(y, r, bnd, cid)
        print(f"{cid}: worst |y - r| / bound = {ratio:.3f}")
        if first.get("both"):                    # outputs that meet in atomics need not repeat bit for bit: the second call is held to the bound itself
            V.assert_inside(again["y"], r, bnd, cid + " (second call)")
        for name, s in first.get("parts", {}).items():
            worst = max(float(((t["y"][s].cpu().double() - r[s]).abs() / bnd[s].clamp_min(1e-300)).max()) for t in (first, again))
            print(f"{cid}: {name} worst |y - r| / bound = {worst:.3f}")
        if "planes" in first:
            pl, fmt = first["planes"]
            planes_equal_split(ops, pl, first.get("planes_src", y).to(DEV), fmt)
    if "decoded" in first:                        # planes only: the bound plus the format's own rounding
        d, rel = first["decoded"]
        ratio = V.assert_inside(d, r, bnd + (rel * r.abs() if rel else 0.0), cid + " (planes)")
        print(f"{cid}: worst |planes - r| / bound = {ratio:.3f}")


@pytest.mark.parametrize("cid,op,p", RAISES, ids=[c[0] for c in RAISES])
def test_variant_refused(ops, cid, op, p):
    """Shapes a launcher must refuse: image groups outside the 7 x 7 kernels; head blocks that do not divide the channels; the ln-*, rs-* and msda*
    refusals of the table.  (Only the inputs are drawn: a refused shape need not have a reference.)"""
    i = V.OPS[op][0](p, V.gen_for(cid))
    with pytest.raises(RuntimeError):
        RUN[op](ops, i, p)
