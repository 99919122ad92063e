/* mmsa.h -- C ABI of libmmsa_hip.so: the MI355X (gfx950) kernels of the MM-SAM-Adapter image-encoder forward.
 *
 * Drop-in boundary.  The reference's only native interface on this path is the pybind11 module
 * `MultiScaleDeformableAttention` (segmentation/ops/src/vision.cpp:13-16) whose forward entry
 * `ms_deform_attn_forward(value, spatial_shapes, level_start_index, sampling_loc, attn_weight, im2col_step)`
 * (segmentation/ops/src/ms_deform_attn.h:20-39 -> cuda/ms_deform_attn_cuda.cu:20-80) is replaced by
 * `mmsa_ms_deform_attn_forward` below.  Every other arithmetic op of the path is a stock PyTorch/ATen call in
 * the reference (F.linear, F.conv2d, F.layer_norm, softmax, F.interpolate ...); the remaining entries are the
 * hand-written kernels that take their place (file:line of the replaced call site is given per entry).
 *
 * Conventions
 *  - plain C, no torch types; every pointer is a DEVICE pointer unless stated; `long` is 64-bit.
 *  - the caller owns all memory (inputs, outputs, workspaces); the library never allocates or frees.
 *  - every call enqueues work on `stream` (a hipStream_t) and returns immediately; no host sync inside, so the
 *    whole forward can be captured into a HIP graph.
 *  - the library is stateless: no environment variable is read and there is no writable global besides the thread-local error string
 *    (A/B knobs exist only in debug-knob builds of single sources, tools/build_variant.sh -DMMSA_DEBUG_KNOBS); what used to be set
 *    through `mmsa_debug_*_flavour` / `mmsa_gemm_next_extras` is an explicit argument of the call it concerns.
 *  - return 0 on success, negative on error; `mmsa_last_error()` returns a thread-local message.  Shapes,
 *    alignment and strides are validated on the host BEFORE anything is launched.
 *  - activations are fp32, token-major / NHWC: a [rows, channels] matrix with a row stride `ld*` in elements.
 *  - GEMM weights -- and the intermediate activations that feed GEMMs / attention -- are operand "planes": row r of a
 *    [rows, K] matrix (K padded to a multiple of 32) is 2K uint16 = one 128-byte line per 32-wide k-block (everything an MFMA
 *    k-step needs from that row).  Plane pointers are 128-byte aligned, row strides multiples of 64.  Two formats:
 *      MMSA_FMT_B3  bf16 hi/lo ("split3": x = hi + lo, three bf16 MFMA products, fp32 accumulate): the 32 hi values, then the 32 lo values;
 *      MMSA_FMT_H8  fp16 hi + e5m2 cross-term bytes (x = hi + lo; hi.hi on the fp16 MFMA, both cross terms of two k-blocks on
 *                   one block-scaled fp8 MFMA at twice the rate: same precision class, 2/3 of the matrix-pipe time): 32 fp16 hi
 *                   values, then four 16-byte chunks, chunk g = 8 bytes e5m2(lo * 2^11) + 8 bytes e5m2(hi) of k = 8g..8g+7 for an
 *                   ACTIVATION (A operand) row, the two halves swapped for a WEIGHT (W operand) row.  |x| is clamped to 57344.
 *      MMSA_FMT_F3  (round 4) the MMSA_FMT_B3 layout with fp16 halves: x = fp16(x) + fp16(x - fp16(x)), 22 significant bits instead of 16, the same
 *                   three MFMAs per product (on the fp16 MFMA); values are clamped to +-65504.  Read by mmsa_gemm_split3 (A as planes, or fp32 A
 *                   with fp32 outputs) and mmsa_convnext_mlp_fused; written by the GEMM, by mmsa_layernorm_rows, mmsa_split_planes (kind 4) and (round 6) mmsa_msda_fused / mmsa_dwconv_nhwc.
 *                   The TwinConvNeXt chain uses it.
 *      MMSA_FMT_H8C the h8 arithmetic on 3 bytes per element (round 4), laid out for the LDS-DMA operand stream of the GEMM: q(hi) is not
 *                   stored (the e5m2 image of an fp16 value is its top byte; the GEMM takes it in registers) and rows are stored in PAIRS --
 *                   pair j of a [rows, K] matrix (K padded to a multiple of 64, rows to even) occupies `ld` uint16 (>= 3 K):
 *                   [row 2j: K fp16 hi][row 2j+1: K fp16 hi][K / 64 lines of 128 bytes: chunk c = {row 2j: 64 lo bytes | row 2j+1: 64 lo bytes}],
 *                   a row's 64 lo bytes of a chunk = 4 groups g of 16 bytes = e5m2(lo * 2^11 * 1.09375) of k = 64c + 8g .. +7, then of k = 64c + 32 + 8g .. +7
 *                   (the factor 1.09375 makes up for q(hi) being the TRUNCATED top byte of hi in this format: csrc/common.h MMSA_H8C_LO_COMP).
 *                   Every `ld*` of h8c planes is the row-PAIR stride; activations and weights share the layout.  1.5 cache lines per row and
 *                   64 k-values where MMSA_FMT_H8 has 2: the GEMM's L2 -> LDS stream is what bounds its k loop (csrc/gemm_h8c.hip).
 *      MMSA_FMT_W8  fp8 WEIGHTS (the opt-in fp8 weights of the ViT-block GEMMs): W[n, k] = 2^e_n * e4m3(code[n, k]) with OCP e4m3fn codes and one exponent
 *                   e_n in [-15, 7] per row (every such value is exact in fp16).  A [N, K] weight (K % 128 == 0) is N rows of K code bytes -- one 128-byte
 *                   line per 128 k, a line's 64-k half c = 4 groups g of 16 bytes = the codes of k = 64c + 8g .. +7, then of k = 64c + 32 + 8g .. +7 (the
 *                   order of the h8c lo bytes) -- followed by the N exponents as signed bytes, zero padded to a multiple of 128.  A W operand only: the
 *                   A operand of such a GEMM is MMSA_FMT_H8C planes (mmsa_gemm_split3 with fmt = MMSA_FMT_W8; csrc/gemm_h8c_w8.hip).
 *    `mmsa_split_planes` converts fp32; producer kernels emit the format of their `*_fmt` argument (h8c: mmsa_gemm_split3, mmsa_layernorm_rows,
 *    the three attention entries, mmsa_msda_fused, mmsa_split_planes).
 *  - Clamp watch (round 5).  The fp16-based formats clamp what they cannot hold (h8 / h8c: |x| > 57344, f3: |x| > 65504; bf16 hi/lo planes have fp32's
 *    range).  The entries that convert UNBOUNDED fp32 values to planes -- mmsa_gemm_split3, mmsa_layernorm_rows, mmsa_split_planes, mmsa_msda_fused,
 *    mmsa_dwconv_nhwc -- take `clamp_max`, an optional DEVICE float (NULL = no watch): a launch that had to clamp folds the largest |value| it met beyond
 *    the format's range (the GEMM's register epilogue: at least the format's limit -- it reports THAT it clamped, not by how much) into it with an atomic max (never lowered; the caller zeroes it).  0 after a forward = every operand plane holds its value.  The
 *    attention entries need none (their outputs are convex combinations of v, which the qkv GEMM's watch has seen).  The reference computes in fp32
 *    and has no such range; mmsa/backbone.py reads the word with the attention guard words and refuses a forward that clamped.
 */
#ifndef MMSA_H
#define MMSA_H
#include <stddef.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

/* A binding sees an opaque pointer.  The library's own sources include this header too (csrc/common.h defines MMSA_BUILDING_LIBRARY behind
 * <hip/hip_runtime.h>), with the stream spelled as the HIP type they use, so that every definition is compiled against its declaration here:
 * a definition whose argument list differs from the prototype is a "conflicting types" error of the library build, not silent stack garbage
 * in a caller.  Both spellings are one pointer in the ABI. */
#ifdef MMSA_BUILDING_LIBRARY
typedef hipStream_t mmsa_stream_t;
#else
typedef void* mmsa_stream_t; /* hipStream_t */
#endif

/* mmsa_version() returns the MMSA_ABI_VERSION (mmsa_version.h) the library was built with; a binding must refuse a library whose number differs from
 * the header it was written against (mmsa/lib.py does) -- argument lists are not self-describing through a C ABI. */
#include "mmsa_version.h"
int mmsa_version(void);
const char* mmsa_last_error(void);

/* testing aid: fill the LDS of every CU with `pattern` (finds kernels that read LDS they did not write) */
int mmsa_debug_poison_lds(unsigned pattern, mmsa_stream_t stream);
/* HIP events on the launch stream (for bench.py; torch.cuda.Event only sees torch's current stream). */
int mmsa_event_create(void** ev);
int mmsa_event_record(void* ev, mmsa_stream_t stream);
int mmsa_event_elapsed_ms(void* start, void* stop, float* ms); /* synchronises on `stop` */
int mmsa_event_destroy(void* ev);

/* activation codes of the fused epilogues */
/* MMSA_ACT_GELU is the erf form (nn.GELU's default: IE:154-167, TC:107-111), evaluated to 3.3e-7 absolute in fp32 (csrc/common.h gelu1 / gelu2) */
enum { MMSA_ACT_NONE = 0, MMSA_ACT_GELU = 1, MMSA_ACT_RELU = 2, MMSA_ACT_RELU6 = 3, MMSA_ACT_HSWISH = 4, MMSA_ACT_SIGMOID = 5 };

/* scalar type codes of the dtype-dispatched entry points (the reference's AT_DISPATCH_FLOATING_TYPES_AND_HALF) */
enum { MMSA_DT_F32 = 0, MMSA_DT_F16 = 1, MMSA_DT_F64 = 2 };

/* operand-plane formats (see Conventions) */
enum { MMSA_FMT_B3 = 0, MMSA_FMT_H8 = 1, MMSA_FMT_H8C = 2, MMSA_FMT_F3 = 3, MMSA_FMT_W8 = 4 /* weights only: see Conventions */ };

/* --- reference native ops -----------------------------------------------------------------------------------
 * ms_deform_attn_forward (vision.cpp:14 -> ms_deform_attn.h:20-39 -> cuda/ms_deform_attn_cuda.cu:20-80).
 * value [N,S,M,D], spatial_shapes int64 [L,2] (H,W), level_start_index int64 [L], sampling_loc [N,Lq,M,L,P,2] (x,y in
 * [0,1]), attn_weight [N,Lq,M,L,P]; out [N,Lq,M*D] (overwritten).  `dtype` = the scalar type of value / sampling_loc /
 * attn_weight / out (ms_deform_attn_cuda.cu:64 dispatches float, double and half; f16 is computed in fp32 here).
 * Error behaviour mirrors ms_deform_attn_cuda.cu:52: batch % min(batch, im2col_step) must be 0. */
int mmsa_ms_deform_attn_forward(const void* value, const int64_t* spatial_shapes, const int64_t* level_start_index,
                                const void* sampling_loc, const void* attn_weight, void* out, int batch,
                                int spatial_size, int num_heads, int channels, int num_levels, int num_query,
                                int num_point, int im2col_step, int dtype, mmsa_stream_t stream);

/* ms_deform_attn_backward (vision.cpp:15 -> ms_deform_attn.h:42-61 -> cuda/ms_deform_attn_cuda.cu:83-151, kernels
 * ms_deform_im2col_cuda.cuh:301-920).  grad_output [N,Lq,M*D]; grad_value / grad_sampling_loc / grad_attn_weight have the
 * shapes of value / sampling_loc / attn_weight and are caller-allocated; the call zero-fills and then fully writes them on
 * `stream` (the reference returns freshly allocated zeros-initialised tensors, :121-123).  grad_value is a scatter of
 * floating-point atomic adds like the reference's, so its last bits depend on the arrival order.
 * f16: 16-bit float atomics work on aligned pairs, so grad_value must be 4-byte aligned, and so must grad_sampling_loc and
 * grad_attn_weight when `channels` is not a power of two <= 64 (they are then summed with atomics too); the call refuses
 * anything else.  The call changes no byte outside the three buffers.  One 32-bit word can reach past one: when a buffer
 * that is summed with atomics has an ODD element count (batch = 1 with odd S*M*D, or odd Lq*M*L*P), its last element shares
 * an aligned word with the half word behind the buffer.  That word is read and rewritten by compare-and-swap with the
 * neighbouring half word's own bits, so its value never changes (a -0.0 stays -0.0, a NaN keeps its payload); it must be
 * readable and writable memory, which it is inside any allocation, whose sizes are multiples of 4 bytes. */
int mmsa_ms_deform_attn_backward(const void* value, const int64_t* spatial_shapes, const int64_t* level_start_index,
                                 const void* sampling_loc, const void* attn_weight, const void* grad_output,
                                 void* grad_value, void* grad_sampling_loc, void* grad_attn_weight, int batch,
                                 int spatial_size, int num_heads, int channels, int num_levels, int num_query,
                                 int num_point, int im2col_step, int dtype, mmsa_stream_t stream);

/* Fused hot-path form of MSDeformAttn.forward's middle part (ops/modules/ms_deform_attn.py:105-127): takes the raw
 * output `raw` [N*Lq, ldraw] of the concatenated sampling_offsets|attention_weights projection
 * (columns [0, M*L*P*2) offsets, then M*L*P logits), the per-query reference points [Lq,2], does softmax over L*P,
 * loc = ref + off/(W_l,H_l), and the sampling gather.  out [N*Lq, ldo]. */
int mmsa_msda_fused(const float* value, const int64_t* spatial_shapes, const int64_t* level_start_index,
                    const float* raw, long ldraw, const float* ref_points, float* out, long ldo,
                    uint16_t* out_planes, long ldop /* optional operand planes output */, int out_fmt /* MMSA_FMT_* */, int batch,
                    int spatial_size, int num_heads, int channels, int num_levels, int num_query, int num_point,
                    float* clamp_max /* optional clamp watch word of out_planes, see Conventions */, mmsa_stream_t stream);

/* mmsa_msda_fused on fp16 values (round 6; the model's opt-in `msda_value` attribute).  The gather is bound by the bytes it pulls through the CU's vector-memory
 * pipe; `value_planes` = the value projection's output (ops/modules/ms_deform_attn.py:103-104) as MMSA_FMT_H8 ACTIVATION planes [batch * spatial_size, row stride
 * ldvp >= 2 * num_heads * channels], written by that GEMM's own epilogue.  lo_bytes = 0: a corner reads the 8 fp16 hi values of a lane's 8 channels (half the
 * bytes of fp32 values; the value is rounded to 11 significant bits); lo_bytes != 0: + their e5m2 lo bytes (3/4 of the bytes, ~14 bits).  Everything else as
 * mmsa_msda_fused; channels % 8 == 0, num_heads * channels % 32 == 0. */
int mmsa_msda_fused_planes(const uint16_t* value_planes, long ldvp, int lo_bytes, const int64_t* spatial_shapes, const int64_t* level_start_index,
                           const float* raw, long ldraw, const float* ref_points, float* out, long ldo,
                           uint16_t* out_planes, long ldop, int out_fmt, int batch,
                           int spatial_size, int num_heads, int channels, int num_levels, int num_query, int num_point,
                           float* clamp_max, mmsa_stream_t stream);

/* --- GEMM (replaces F.linear / 1x1 conv / patchify conv / ConvTranspose2d 2x2 s2) ---------------------------
 * C = beta*resid + colscale[n] * alpha * act(A[M,K] W[N,K]^T + bias[n]); batch > 1 = strided batched (strides in
 * elements; strideW / strideBias may be 0 to share; colscale, when given, uses strideBias too).  K % 32 == 0.  resid_mod > 0: residual row = row % resid_mod
 * (broadcast over the batch, e.g. pos_embed).  out_mode 1 = 2x2 pixel-shuffle store for ConvTranspose2d(k=2,s=2)
 * (BK:55,324): row (b,h,w), column (i,j,co) -> row (b,2h+i,2w+j), column co; resid uses the destination index.
 * Call sites replaced: IE:488,499,162-167; TC:107-111,297-304,328-335; AM:947-950,447-451,87-89,121-126,286-290;
 * ops/modules/ms_deform_attn.py:103,107-110,129; BK:324.
 * A is EITHER fp32 (`A`, split to hi/lo while staged) OR interleaved activation planes (`Ap`, written by the
 * producing kernel; lda/strideA then count uint16 elements, lda >= 2K).  W: interleaved planes, row stride 2K.
 * The result goes to fp32 `C`, to planes `Cp` (row stride ldcp >= 2*N rounded up to 64), or both.
 * fmt = format of the A and W planes (MMSA_FMT_H8 / MMSA_FMT_H8C: A must come as planes, K % 64 == 0, any M -- rows beyond M are clamped on the way in and masked on the way out; lda / ldcp of h8c planes =
 * row-pair strides >= 3 K / 3 pad64(N); MMSA_FMT_W8: A as MMSA_FMT_H8C planes, W = a W8 weight, K % 128 == 0, batch 1); cp_fmt = format written to `Cp`:
 * bits 0..7 MMSA_FMT_*, bits 8.. = split / 32 -- columns >= split (a multiple of 32; 0 = none) are written as MMSA_FMT_H8 planes
 * whatever the base format (the qkv projection: q and k as f3 planes, v with an fp16 hi part for the attention kernels' v_fmt = 1).
 * max_grid > 0 caps the number of persistent workgroups (a caller running independent chains on concurrent streams gives each
 * its share of the CUs); 0 = all CUs.  Results do not depend on it. */
/* LayerNorm folded into a producer / consumer pair of GEMMs (base/image_encoder.py:396-421: x -> norm1 -> qkv, x -> norm2 -> lin1): three
 * optional arguments of the call (it must then be one the LDS-DMA kernel takes: activation planes, M >= 128):
 *   rowstats_out [M, N/64, 2] fp32: the call also writes, per output row and 64-column strip, the sum and the sum of squares of the fp32
 *     values it stores (plain fp32 output, no activation, N % 64 == 0) -- the producer of the residual stream;
 *   rownorm_mean_rstd [M, 2] + rownorm_colsum [N] (batch stride = strideBias): the call runs on the RAW stream's planes against W o w and its
 *     epilogue computes rstd_r * (acc - mean_r * colsum_n) + bias_n before the activation (planes-only output, N % 128 == 0) -- the consumer.
 * mmsa_rowstats_finalize turns the strip sums into (mean, rstd) per row (D = 64 * strips columns, biased variance, eps inside the root).
 * flavour: 0 = workgroup shape chosen by the problem (256-row ping-pong tiles; 128-row tiles, two workgroups per CU, for bf16 hi/lo
 * operands with K <= 256); 4 / 8 force the 128- / 256-row form (tests, A/B runs).  Results are bit-identical either way. */
int mmsa_rowstats_finalize(const float* rowstats, int rows, int strips, int D, float eps, float* mean_rstd, mmsa_stream_t stream);

/* Zero-fill `bytes` bytes at p on `stream` (hipMemsetAsync): the statistics blocks the neck's kernels accumulate into.  Host-side mirror: the
 * `.zero_()` calls of the reference's own accumulator initialisations are torch kernels; inside a captured step every node is the library's. */
int mmsa_zero_bytes(void* p, size_t bytes, mmsa_stream_t stream);
int mmsa_gemm_split3(const float* A, const uint16_t* Ap, long lda, long strideA,
                     const uint16_t* Wp, long strideW,
                     const float* bias, long strideBias, const float* colscale, const float* resid, long ldr,
                     long strideR, int resid_mod, float beta, float* C, long ldc, long strideC,
                     uint16_t* Cp, long ldcp, long strideCp, int M, int N, int K,
                     int batch, int act, float alpha, int out_mode, int ps_H, int ps_W, int ps_C, int fmt, int cp_fmt,
                     int max_grid, float* rowstats_out, const float* rownorm_mean_rstd, const float* rownorm_colsum, int flavour,
                     float* clamp_max /* optional clamp watch word of the planes output, see Conventions */, mmsa_stream_t stream);

/* ConvNeXt pointwise pair of the narrow stages as ONE kernel (TC:107-132): x[b] <- x[b] + gamma[b] * (GELU(A[b] W1[b]^T + b1[b]) W2[b]^T
 * + b2[b]); A = LayerNorm output as bf16 hi/lo planes [M, C] (row stride lda, batch stride strideA, uint16 units), W1 [4C, C] and
 * W2 [C, 4C] bf16 hi/lo planes per batch, b1 [batch, 4C], b2 / gamma [batch, C], x fp32 [M, C] (row stride ldx) updated in place.
 * C = 96 (the narrowest ConvNeXt stage); the 4C-wide hidden tensor stays in LDS.  max_grid as in mmsa_gemm_split3.  fmt = MMSA_FMT_B3 or
 * MMSA_FMT_F3: the format of A, W1, W2 (and of the hidden image the kernel keeps in LDS). */
int mmsa_convnext_mlp_fused(const uint16_t* Ap, long lda, long strideA, const uint16_t* W1p, long strideW1, const uint16_t* W2p,
                            long strideW2, const float* b1, const float* b2, const float* gamma, float* x, long ldx, long strideX,
                            int M, int C, int batch, int max_grid, int fmt,
                            float* clamp_max /* optional clamp watch word of the hidden tensor's planes (fmt = MMSA_FMT_F3), see Conventions */, mmsa_stream_t stream);

/* fp32 [rows, cols] (row stride ld) -> planes [rows, 2*cols_pad], zero padded (cols_pad % 32 == 0).
 * kind 0: bf16 hi/lo; 1: h8 activation rows; 2: h8 weight rows; 3: h8c planes [ceil(rows / 2), 3*cols_pad] (cols_pad % 64 == 0; activations and weights);
 * 4: f3 (fp16 hi/lo pairs in the bf16 hi/lo layout). */
int mmsa_split_planes(const float* src, long ld, int rows, int cols, int cols_pad, uint16_t* planes, int kind,
                      float* clamp_max /* optional clamp watch word, see Conventions */, mmsa_stream_t stream);

/* --- attention (IE:465-501 incl. window_partition/unpartition IE:504-551 and rel-pos IE:587-623) -------------
 * Attention logit guard: the planes entries take `max_abs_logit`, an optional DEVICE float (NULL = none).  The launch folds the largest
 * |logit| it scores -- scale * q.k + the rel-pos terms, natural units, over existing keys (pad tokens of a window included, they are
 * attended to) and live queries -- into it with an atomic max (never lowered; the caller zeroes it).  The reference computes attention
 * in fp32 (IE:488-499) and needs no such word; this library chooses the operand precision of a block's attention (v_fmt) from it:
 * the host reads it after the step and moves a block whose logits outgrow single fp16 operands to fp16 hi/lo PAIRS (f3 planes; mmsa/backbone.py).
 * qkv [B*H*W, ldq] = q|k|v, channel = head*head_dim + c; qkv_bias [3*D]; rp from mmsa_relpos_bias;
 * window_size 0 = global.  out [B*H*W, ldo]. head_dim in {32, 64}. */
int mmsa_attention(const float* qkv, long ldq, const float* qkv_bias, const float* rp, float* out, long ldo, int B,
                   int H, int W, int heads, int head_dim, int window_size, float scale, mmsa_stream_t stream);
/* same with qkv [.., 2*3D], qkv_bias [2*3D] and the output [.., 2*D] as interleaved planes (strides in uint16) */
int mmsa_attention_planes(const uint16_t* qkv_planes, long ldq, const uint16_t* bias_planes, const float* rp,
                          uint16_t* out_planes, long ldo, int B, int H, int W, int heads, int head_dim,
                          int window_size, float scale, int out_fmt /* MMSA_FMT_* of out_planes */,
                          int v_fmt /* 0: qkv_planes / bias_planes (and the rel-pos planes of the fused entries) are MMSA_FMT_F3 planes -- fp16 hi/lo pairs, three fp16 MFMAs per product; round 4: bf16 hi/lo planes before, same layout, NOT accepted any more; 1 (this entry): their v columns are h8 planes (fp16 hi,
                                       as the qkv GEMM writes them with cp_fmt = MMSA_FMT_F3 | (2D/32) << 8): P V runs on the fp16 MFMA with
                                       P rounded to fp16; 2 (the two fused rel-pos entries below): qkv_planes, bias_planes AND relpos_planes
                                       are h8 planes throughout (and the window kernel's selector holds fp16 ones): every contraction of
                                       the kernel is one fp16 MFMA on the hi parts */,
                          float* max_abs_logit /* optional, see "Attention logit guard" */, mmsa_stream_t stream);

/* rel-pos bias terms: rp [B, heads, H*W, KH+KW]; Rh [QS,KH,head_dim], Rw [QS,KW,head_dim] = gathered tables
 * get_rel_pos(...)  (IE:554-584), (KH,KW,QS) = (ws,ws,ws) for windowed blocks or (H,W,max) for global ones. */
int mmsa_relpos_bias(const float* qkv, long ldq, const float* Rh, const float* Rw, float* rp, int B, int H, int W,
                     int heads, int head_dim, int window_size, mmsa_stream_t stream);
int mmsa_relpos_bias_planes(const uint16_t* qkv_planes, long ldq, const float* Rh, const float* Rw,
                            float* rp, int B, int H, int W, int heads, int head_dim, int window_size, mmsa_stream_t stream);

/* --- normalisation / reductions ------------------------------------------------------------------------------
 * Row LayerNorm (biased variance): y = (x-mean)/sqrt(var+eps)*w + b; optional y2 = x + y.  map_mode 1 scatters
 * token (b,h,w) of an [B,map_H,map_W] grid to row (b,h/2,w/2), column block (h&1)*2+(w&1) (the im2col layout of
 * the ConvNeXt 2x2 s2 downsample conv, TC:328-335).  Replaces nn.LayerNorm / LN2d / WithBias_LayerNorm:
 * IE:367,377; AM:479-487,519-520,51-74; mmpretrain_custom/models/utils/norm.py:51-90.
 * Row groups (group_rows > 0; the two TwinConvNeXt streams stacked along the rows, TC:445-476): group g = row / group_rows
 * uses w + g*w_gstride, b + g*w_gstride and writes at column offset g*y_gcol; y_wrap != 0: output row = row % group_rows
 * (channel-concatenation of the two streams' stage outputs, TC:466-472).  group_rows = 0: one group. */
int mmsa_layernorm_rows(const float* x, long ldx, const float* w, const float* b, float eps, float* y, long ldy,
                        float* y2, long ldy2, uint16_t* y_planes, long ldp /* optional interleaved planes of y */,
                        int rows, int C, int map_mode, int map_H, int map_W, int group_rows, long w_gstride, long y_gcol,
                        int y_wrap, int plane_fmt /* MMSA_FMT_* of y_planes */, float* clamp_max /* optional clamp watch word, see Conventions */,
                        mmsa_stream_t stream);

/* out (double) [B,3,C]: sum_p x, sum_p x^2, sum_p wrow[p]*x over the HW rows of each image (wrow may be NULL). */
int mmsa_colstats(const float* x, long ldx, long strideB, const float* wrow, int B, int HW, int C, double* out,
                  int out_is_zero /* 1: the caller zeroed `out` on this stream; 0: the call zeroes it first */, mmsa_stream_t stream);

/* GFFM LayerNorm(H*W) statistics + FFRM gate (AM:241,265 and AM:158-162), see csrc/norm.hip. */
int mmsa_ffrm_finalize(const double* stats, int B, int HW, int C, float mean_w, float mean_b, const float* Wc,
                       const float* gn_w, const float* gn_b, float* mean_o, float* rstd_o, float* mult_o,
                       float* scratch /* [2,B,C] */, mmsa_stream_t stream);
int mmsa_lnhw_apply(const float* x, long ldx, const float* mean, const float* rstd, const float* mult, const float* w,
                    const float* bias, float* y, long ldy, int B, int HW, int C, mmsa_stream_t stream);

/* --- convolutions on NHWC maps (stride 1, same padding) and patch gather ------------------------------------
 * dwconv: weights tap-major [k*k, C]; replaces TC:69-70,102; AM:288; AM:459,464-469.
 * gconv: weights [G][k*k][cin_g][cout_g]; replaces AM:87-88,123-124.
 * im2col_nchw: out[(b,ph,pw)][(c,kh,kw)] from NCHW input channels [c0, c0+Cin) (IE:658-663, TC:297-304). */
int mmsa_dwconv_nhwc(const float* x, long ldx, long xstrideB, const float* w, const float* bias, float* y, long ldy,
                     long ystrideB, uint16_t* y_planes, long ldp, long pstrideB /* optional operand planes */, int planes_fmt /* MMSA_FMT_* */,
                     int B, int H, int W, int C, int k, int act,
                     int imgs_per_group /* > 0: image group g = b / imgs_per_group uses w + g*k*k*C, bias + g*C */,
                     float* rowstats /* optional, 7x7 only (C % 64 == 0, H, W % 8 == 0): per pixel and 64-channel chunk (sum, sum of squares) of the
                                        output, [B*H*W][C/64][2]: the strip sums of the LayerNorm fold (mmsa_rowstats_finalize) */,
                     float* clamp_max /* optional clamp watch word, see Conventions */, mmsa_stream_t stream);
int mmsa_gconv_nhwc(const float* x, long ldx, const float* w, const float* bias, float* y, long ldy, int B, int H,
                    int W, int G, int cin_g, int cout_g, int k, int act, mmsa_stream_t stream);
/* GFE qkv (AM:87-92): qkv2(qkv1(x)), a bias-free grouped 1x1 conv (cin_g -> cout_g) followed by a bias-free grouped 3x3 conv (cout_g -> cout_g) over
 * the same G groups, as ONE grouped 3x3 conv with the folded weights w[g][tap][ci][co] = sum_m q1[g][ci][m] * q2[g][tap][m][co] (csrc/gfe_qkv.hip; fp32
 * operands and accumulation).  Covered: cout_g = 3 cin_g, cin_g = 3 / 6 / 12 / 24, G * cin_g a multiple of 24.  *covered = 1: y is written;
 * *covered = 0: nothing was launched and the caller runs the two mmsa_gconv_nhwc launches. */
int mmsa_gfe_qkv_conv(const float* x, long ldx, const float* w, float* y, long ldy, int B, int H, int W, int G, int cin_g, int cout_g,
                      int* covered, mmsa_stream_t stream);
/* gated pair stage of the neck Mlp (AM:127-132): y = gelu(dw3x3(x)[:, :C]) * dw3x3(x)[:, C:], x token-major [B*H*W, 2C], the
 * depthwise conv has 2 channels per group (C groups), weights TAP-major [9][C][ci=2][co=2]; fp32 and/or interleaved-planes output */
int mmsa_dwpair_gate(const float* x, long ldx, const float* w, float* y, long ldy, uint16_t* y_planes, long ldp, int B, int H,
                     int W, int C, mmsa_stream_t stream);
int mmsa_im2col_nchw(const float* x, int B, int Ctot, int c0, int Cin, int H, int W, int p, float* out, int Kpad,
                     mmsa_stream_t stream);

/* --- modality-fusion neck pieces (AM:75-109, 234-267, 110-132, 176-221) ------------------------------------- */
/* G[b] = X[b]^T Y[b] over the P rows of each image: fp32 MFMA per 256-row slice, the slices summed in double in slice order (deterministic;
 * G needs no zeroing).  nblk > 1: only the entries of the nblk diagonal head blocks (c / nblk channels each) are written.  `scratch`:
 * caller-owned, >= mmsa_gram_tn_scratch_bytes(B, P, c) bytes, 16-byte aligned (the per-slice partial sums). */
long mmsa_gram_tn_scratch_bytes(int B, int P, int c);
int mmsa_gram_tn(const float* X, long ldx, const float* Y, long ldy, long strideB, double* G /* [B,c,c] */, int B, int P, int c,
                 int nblk, void* scratch, long scratch_bytes, mmsa_stream_t stream);
int mmsa_chanattn_build(const double* G, const double* sq, long sq_strideB, const double* sk, long sk_strideB,
                        const float* temp, const float* Wp, uint16_t* planes /* [B,c,2*cpad] */, int B, int c, int cpad,
                        int heads, mmsa_stream_t stream);
int mmsa_gffm_build(const double* E, uint16_t* x_planes, uint16_t* y_planes /* [B,c,2*cpad] each */, int B, int c,
                    int cpad, mmsa_stream_t stream);
int mmsa_gelu_gate(const float* x, long ldx, float* y, long ldy, long rows, int C, mmsa_stream_t stream);
int mmsa_pool_hw(const float* z, long ldz, float* out, long ldo, int B, int H, int W, int C, mmsa_stream_t stream);
int mmsa_ca_apply(const float* z, long ldz, const float* att, long lda, float* out, long ldo,
                  uint16_t* out_planes, long ldp /* optional interleaved planes */, int B, int H, int W, int C, mmsa_stream_t stream);

/* --- tail (BK:316-337): out NCHW [B,C,Hc,Wc] = (cmap + bilinear(xtok)) * bn_scale + bn_shift; cmap image b starts at b*cstrideB;
 * xtok == NULL: no ViT feature is added (add_vit_feature = False, BK:326) --- */
int mmsa_tail_fuse(const float* cmap, long ldc, long cstrideB, const float* xtok, long ldx, const float* bn_scale,
                   const float* bn_shift, float* out, uint16_t* out_planes /* optional: the same map token-major
                   [B*Hc*Wc, 2*C] as interleaved planes, for the decode head's first 1x1 conv */, long ldp,
                   int B, int Hc, int Wc, int Hx, int Wx, int C, mmsa_stream_t stream);

/* --- global attention with the rel-pos terms computed in the kernel (Attention.forward IE:465-501 + add_decomposed_rel_pos IE:587-623 on a
 *     window_size = 0 block): planes in / out as mmsa_attention_planes; relpos_planes = interleaved planes of a [256, 64] matrix, rows
 *     0..2H-2 = rel_pos_h and rows 128..128+2W-2 = rel_pos_w (tables already resized to 2H-1 / 2W-1 rows, IE:568-575).  W = 64,
 *     H <= 64 and a multiple of 4, head_dim 64.  No mmsa_relpos_bias pass. --- */
int mmsa_global_attention_planes(const uint16_t* qkv_planes, long ldq, const uint16_t* bias_planes, const uint16_t* relpos_planes,
                                 uint16_t* out_planes, long ldo, int B, int H, int W, int heads, int head_dim, float scale,
                                 int out_fmt /* MMSA_FMT_* of out_planes */, int v_fmt /* 0 or 2: see mmsa_attention_planes */,
                                 float* max_abs_logit /* optional */, mmsa_stream_t stream);

/* --- windowed attention with the rel-pos bias fused (Block.forward IE:382-423 on a window_size > 0 block: window_partition ->
 *     Attention.forward IE:465-501 + add_decomposed_rel_pos IE:587-623 -> window_unpartition).  qkv / bias / out as in
 *     mmsa_attention_planes; relpos_planes = interleaved planes of a [64, 64] matrix whose rows 0..2ws-2 are the block's
 *     rel_pos_h table (already resized to 2ws-1 rows, IE:568-575) and rows 32..32+2ws-2 its rel_pos_w.  selector =
 *     [208, 32] bf16 (row-major, 128-byte aligned): selector[j][j / ws] = selector[j][14 + j % ws] = 1.0 for j < ws*ws,
 *     0 elsewhere (a constant of the window size).  head_dim 64, window_size <= 14.  No mmsa_relpos_bias pass. --- */
int mmsa_window_attention_planes(const uint16_t* qkv_planes, long ldq, const uint16_t* bias_planes,
                                 const uint16_t* relpos_planes, const uint16_t* selector, uint16_t* out_planes, long ldo, int B, int H, int W,
                                 int heads, int head_dim, int window_size, float scale, int out_fmt /* MMSA_FMT_* of out_planes */,
                                 int v_fmt /* 0 or 2: see mmsa_attention_planes */, float* max_abs_logit /* optional */, mmsa_stream_t stream);

/* --- Segformer decode head (segmentation/mmseg_custom/models/decode_heads/segformer_head.py:47-66; the 1x1 convs are
 *     mmsa_gemm_split3 calls).  nchw_to_planes: backbone map [B,C,HW] fp32 (image b at b*strideB) -> interleaved planes
 *     [B*HW, C].  head_fuse: planes/out32 [B*H*W, C] = act((z0 + sum_i bilinear_{align_corners=False}(z_i -> HxW)) * bn_scale
 *     + bn_shift); z_i token-major [B*H_i*W_i, ld] fp32, NULL levels skipped.  tokens_to_nchw: [B*HW, ld] -> [B,C,HW]. --- */
int mmsa_nchw_to_planes(const float* src, long strideB, uint16_t* planes, long ldp, int B, int C, long HW,
                        mmsa_stream_t stream);
int mmsa_head_fuse(const float* z0, const float* z1, int H1, int W1, const float* z2, int H2, int W2, const float* z3,
                   int H3, int W3, long ld, const float* bn_scale, const float* bn_shift, uint16_t* planes, long ldp,
                   float* out32, long ldo, int B, int H, int W, int C, int act, mmsa_stream_t stream);
int mmsa_tokens_to_nchw(const float* src, long ld, float* dst, int B, long HW, int C, mmsa_stream_t stream);

/* --- segmentor glue (segmentation/mmseg_custom/models/segmentors/encoder_decoder.py): bilinear_accum writes (accumulate = 0) or adds
 *     (accumulate != 0) resize(src -> hc x wc, bilinear, align_corners=False) into window (y0, x0) of the NCHW canvas dst and, when count
 *     is given, adds 1 to count[b, y, x] over the window (ED:90-94, 213-219); div_count: preds / count_mat (ED:225); argmax over C
 *     (ED:477) -> uint8 map, first maximum wins. --- */
int mmsa_bilinear_accum_nchw(const float* src, long src_strideB, int B, int C, int hs, int ws, float* dst, int Hd, int Wd, int y0, int x0,
                             int hc, int wc, float* count, int accumulate, mmsa_stream_t stream);
int mmsa_div_count_nchw(float* x, const float* count, int B, int C, long HW, mmsa_stream_t stream);
int mmsa_argmax_nchw(const float* x, unsigned char* out, int B, int C, long HW, mmsa_stream_t stream);
/* crop extraction of slide inference (ED:205-212) for a batch of windows in one launch: dst[k] = src[b_k, :, y0_k:+hc, x0_k:+wc];
 * `windows` is a HOST array [n,3] = (image, y0, x0), n <= 64 (copied into the launch arguments). */
int mmsa_crop_batch_nchw(const float* src, int B, int C, int H, int W, const int* windows, int n, float* dst, int hc, int wc,
                         mmsa_stream_t stream);
/* class map of a whole sliding-window frame in one pass (ED:213-225 + ED:449,477): out[b,y,x] = argmax_c (sum over the covering windows,
 * in window order, of bilinear(logits_k -> hc x wc)[c]) / count -- the same additions in the same order as bilinear_accum + div_count +
 * argmax without the [B,C,H,W] canvas; one full-size window per image = resize + argmax of whole-image inference.  logits [n,C,hs,ws];
 * `uncovered` (device int, zeroed by the caller) counts pixels that no window covers (ED:220). */
int mmsa_slide_argmax(const float* logits, int n, int C, int hs, int ws, const int* windows, unsigned char* out, int B, int H, int W,
                      int hc, int wc, int* uncovered, mmsa_stream_t stream);
/* the same class map at a RESCALED size (`rescale=True`: ED:227-233, 314-325, 349-360, 393-414): the averaged logits of the H x W frame are resized once
 * more (bilinear, align_corners=False) to Hd x Wd -- larger or smaller, any ratio per axis, no antialiasing -- and cropped to [:Hcut, :Wcut] (Hcut <= Hd,
 * Wcut <= Wd; ED:414) before the argmax; out [B, Hcut, Wcut].  Bit for bit the map of bilinear_accum (accumulate) + div_count + bilinear_accum (write, into
 * [B,C,Hd,Wd]) + argmax + crop, with neither canvas in memory.  Each of an output pixel's four canvas taps divides by its own window count; a pixel with a
 * tap that no window covers (or more than 8 do) gets 255 and is counted once in `uncovered`. */
int mmsa_slide_argmax_resized(const float* logits, int n, int C, int hs, int ws, const int* windows, unsigned char* out, int B, int H, int W,
                              int hc, int wc, int Hd, int Wd, int Hcut, int Wcut, int* uncovered, mmsa_stream_t stream);

/* --- test-time augmentation (EncoderDecoder.aug_test, ED:509-546): several views of a frame -- flipped, at several scales -- whose PROBABILITIES are
 *     averaged before the argmax.
 * the canvas-path step: p = softmax over C of logits [B, C, H, W] (F.softmax(seg_logit, dim=1), ED:449,460: m = max, e = expf(x - m), s = sum in class
 * order, p = e / s), flipped back (flip 1 = 'horizontal': x' = W - 1 - x, ED:454-455,465-466; 2 = 'vertical': y' = H - 1 - y, ED:456-457,467-468; 0: not
 * flipped) and written (accumulate = 0) or added (seg_logit += cur_seg_logit, ED:540) to acc [B, C, H, W]; finish_div > 0: the stored value is also
 * divided by it (seg_logit /= len(imgs), ED:541).  acc must not alias logits. */
int mmsa_softmax_flip_accum_nchw(const float* logits, float* acc, int B, int C, int H, int W, int flip, int accumulate, int finish_div, mmsa_stream_t stream);
/* the whole of aug_test after the head in ONE launch (ED:517, 538-542): out uint8 [B, Ho, Wo] = first argmax_c of the mean over the A views (1..12), in
 * view order, of the softmax of view a's logits at the pixel's mirror image (that view's flip) -- the logits mmsa_slide_argmax_resized computes there from
 * the view's head-resolution logits.  logits: HOST array of A device pointers, view a's being [n_a, C, hs_a, ws_a]; views: HOST int [A, 11] rows
 * (w0, n, hs, ws, H, W, hc, wc, Hd, Wd, flip): view a's windows are rows w0 .. w0 + n - 1 (n <= 64) of `windows`, a DEVICE int [total, 3] array of
 * (image, y0, x0) owned by the caller, with `windows_host` its HOST copy (validated here); H x W the view's canvas, hc x wc its window size, Hd x Wd its
 * rescale target (H x W: none), of which [:Ho, :Wo] is kept.  Bit for bit mmsa_argmax_nchw of the mmsa_softmax_flip_accum_nchw canvas path.  C <= 128 (two
 * columns of C floats per pixel in LDS).  A pixel where any view has a tap that no window covers (or more than 8 do) gets 255 and is counted once in `uncovered`. */
int mmsa_aug_argmax(const float* const* logits, const int* views, int A, int C, const int* windows, const int* windows_host, int total,
                    unsigned char* out, int B, int Ho, int Wo, int* uncovered, mmsa_stream_t stream);

/* --- confidence maps: next to every class map above, the probability of the class it names -- conf[b, y, x] = max_c P[b, c, y, x], float32 [B, Ho, Wo],
 *     with P what EncoderDecoder.inference returns (F.softmax(seg_logit, dim=1), ED:449,460; for several views their mean, ED:538-541).  One view, with
 *     x_c the pixel's logits after the resize stages: m = max_c x_c; s = e_0, s += e_c in class order, e_c = expf(x_c - m); conf = expf(m - m) / s, which
 *     is P at the first maximum and so the largest P.  Several views: conf = max_c (sum over the views of P_a[c]) / A.  Bit for bit the maximum over C of
 *     the mmsa_softmax_flip_accum_nchw canvas path.  A pixel the one-pass kernels mark 255 (a tap without a window, or more than 8) gets conf = 0.
 *     Each entry is its sibling above with `conf` (not NULL) after `out`: same arguments, same checks, same class map. --- */
/* mmsa_argmax_nchw that also writes the maximum, maxval float [B, HW]: on a canvas of probabilities, the class map and its confidence (ED:449,460,477). */
int mmsa_argmax_max_nchw(const float* x, unsigned char* out, float* maxval, int B, int C, long HW, mmsa_stream_t stream);
/* mmsa_slide_argmax + conf [B, H, W] (ED:449,460 on the averaged logits of ED:213-225). */
int mmsa_slide_argmax_conf(const float* logits, int n, int C, int hs, int ws, const int* windows, unsigned char* out, float* conf, int B, int H, int W,
                           int hc, int wc, int* uncovered, mmsa_stream_t stream);
/* mmsa_slide_argmax_resized + conf [B, Hcut, Wcut] (ED:449,460 on the logits at the rescaled size). */
int mmsa_slide_argmax_resized_conf(const float* logits, int n, int C, int hs, int ws, const int* windows, unsigned char* out, float* conf, int B, int H,
                                   int W, int hc, int wc, int Hd, int Wd, int Hcut, int Wcut, int* uncovered, mmsa_stream_t stream);
/* mmsa_aug_argmax + conf [B, Ho, Wo] (ED:449,460 per view, the mean of ED:538-541, its maximum over the classes). */
int mmsa_aug_argmax_conf(const float* const* logits, const int* views, int A, int C, const int* windows, const int* windows_host, int total,
                         unsigned char* out, float* conf, int B, int Ho, int Wo, int* uncovered, mmsa_stream_t stream);

/* --- the input side of the test pipelines (segmentation/mmseg_custom/datasets/pipelines/transform.py): Pad_multimodal (2934-3010, impad bottom /
 *     right) -> Normalize_multimodal / Normalize_multimodal_Muses (2601-2825: `/ 255` when norm_by_max, mmcv.imnormalize = channel reversal when
 *     to_rgb, subtract mean, multiply by 1 / float64(std)) -> ImageToTensor (HWC -> CHW) -> Collectmod, from the loaders' frames in one pass.
 *     src0 / src1 = the two modalities, each [B, Hs, Ws, 3] HWC contiguous, uint8 or float32 (dtype0 / dtype1 below).  HOST arrays (copied into
 *     the launch arguments): mean[6], sinv[6] per OUTPUT channel, sinv = float32(1 / float64(float32(std))); div255[2], swap[2], pad_val[2] per
 *     modality.  out[c] = (a - mean[c]) * sinv[c] with a = x / 255.0f where div255 (a correctly rounded division), x = the modality's channel
 *     2 - c where swap; float32, one rounding per step, no fused multiply-add.  Pixels outside the source (H >= Hs, W >= Ws: padded bottom /
 *     right) are pad_val BEFORE normalisation, as in the FMB pipelines (pad first, normalise after).
 *     preprocess_nhwc: dst [B, 6, H, W].  preprocess_crops: dst[k] = window (image, y0, x0) of size hc x wc of that canvas (ED:205-212),
 *     `windows` as in mmsa_crop_batch_nchw, checked against the PADDED H x W canvas; the full-size normalised frame is never written. --- */
enum { MMSA_PRE_U8 = 0, MMSA_PRE_F32 = 1 };
int mmsa_preprocess_nhwc(const void* src0, int dtype0, const void* src1, int dtype1, int B, int Hs, int Ws, const float* mean,
                         const float* sinv, const int* div255, const int* swap, const float* pad_val, float* dst, int H, int W,
                         mmsa_stream_t stream);
int mmsa_preprocess_crops(const void* src0, int dtype0, const void* src1, int dtype1, int B, int Hs, int Ws, const float* mean,
                          const float* sinv, const int* div255, const int* swap, const float* pad_val, int H, int W, const int* windows,
                          int n, float* dst, int hc, int wc, mmsa_stream_t stream);
/* The same two outputs from sources of another size: `Resize_multimodal` FIRST (transform.py:1136-1167: mmcv.imrescale / mmcv.imresize per
 * modality = cv2.resize(..., INTER_LINEAR)), then the steps above.  The Hs x Ws sources are resized to Hr x Wr inside the H x W canvas (H >= Hr,
 * W >= Wr; the rest is padding).  DEVICE tables, one entry per resized row / column: yofs[Hr] / xofs[Wr] = first source row / column of the two
 * taps (the second is + 1, clamped to the source), ycoef / xcoef = the coefficient pair: int16[.][2] scaled by 2048 when fixed_point (OpenCV's
 * 8-bit path: D = S0 * a0 + S1 * a1 in int32, dst = (((b0 * (D0 >> 4)) >> 16) + ((b1 * (D1 >> 4)) >> 16) + 2) >> 2; both sources must be uint8),
 * float32[.][2] otherwise (D = S0 * a0 + S1 * a1, dst = D0 * b0 + D1 * b1, one float32 rounding per product and sum; a uint8 source is
 * converted exactly first, as numpy's concatenation of a uint8 and a float32 modality does, loading.py:225).  The tables are the caller's
 * (mmsa/preprocess.py builds them as OpenCV's resize.cpp states them); taps are clamped into the source whatever they hold.  The resized frame
 * is never written. */
int mmsa_preprocess_resize_nhwc(const void* src0, int dtype0, const void* src1, int dtype1, int B, int Hs, int Ws, const float* mean,
                                const float* sinv, const int* div255, const int* swap, const float* pad_val, float* dst, int H, int W,
                                int Hr, int Wr, const int* xofs, const void* xcoef, const int* yofs, const void* ycoef, int fixed_point,
                                mmsa_stream_t stream);
int mmsa_preprocess_resize_crops(const void* src0, int dtype0, const void* src1, int dtype1, int B, int Hs, int Ws, const float* mean,
                                 const float* sinv, const int* div255, const int* swap, const float* pad_val, int H, int W, const int* windows,
                                 int n, float* dst, int hc, int wc, int Hr, int Wr, const int* xofs, const void* xcoef, const int* yofs,
                                 const void* ycoef, int fixed_point, mmsa_stream_t stream);

/* --- evaluation (segmentation/mmseg_custom/datasets/DELIVER.py:219-259 `pre_eval` -> apis/evaluation/metrics_micro.py:26-86 `intersect_and_union`): the
 *     confusion counts of a uint8 class map against a uint8 label map.  counts = int64 [n_slots, C + 1, C + 1], counts[s][l][p] = pixels of the images
 *     routed to slot s with transformed label class l and predicted class p; index C = a value outside [0, C) that is not ignored (what
 *     torch.histc(min=0, max=C-1) drops from one of its histograms only); pixels whose label is ignored are counted nowhere.  The reference's four
 *     histograms: area_intersect = diag[:C]; area_pred_label[p] = sum over all C + 1 rows of column p < C; area_label[l] = sum over all C + 1 columns
 *     of row l < C; area_union = area_pred_label + area_label - area_intersect.  The call ADDS into counts (the caller zeroes it): integer sums, the
 *     same bytes whatever the order of arrival.
 *     lut: 256 DEVICE bytes, raw label byte -> class 0 .. C - 1, C (kept, out of range; any other code counts as C too) or 255 (ignored): the whole of
 *       label_map / reduce_zero_label / ignore_index (metrics_micro.py:66-74; mmsa/evaluate.py builds it).
 *     ymap [H], xmap [W]: optional DEVICE int32 source-index tables, both or neither: the label is read at label[b, ymap[y], xmap[x]] -- the
 *       nearest-neighbour resize of Resize_multimodal._resize_seg (datasets/pipelines/transform.py:1169-1188) -- clamped into the label map whatever
 *       they hold.  Without them Hl == H and Wl == W is required.
 *     slots: HOST int [B] (copied into the launch arguments, B <= 64), each in [0, n_slots): the count slot of image b.  0 .. B - 1 = per-image counts
 *       as pre_eval returns them; several images on one slot = a per-case total.
 *     2 <= C <= 126 (the (C + 1)^2 uint32 histogram a workgroup keeps in LDS must fit 64 KiB).
 *   eval_confusion_u8: pred [B, H, W], label [B, Hl, Wl].
 *   slide_argmax_eval: mmsa_slide_argmax and the counts of its class map in ONE launch; out == NULL writes no map.  Uncovered pixels (class 255)
 *     count under predicted index C, as a 255 in a map given to eval_confusion_u8 does. --- */
int mmsa_eval_confusion_u8(const unsigned char* pred, const unsigned char* label, int B, int H, int W, int Hl, int Wl, const unsigned char* lut,
                           int C, const int* ymap, const int* xmap, const int* slots, int n_slots, int64_t* counts, mmsa_stream_t stream);
int mmsa_slide_argmax_eval(const float* logits, int n, int C, int hs, int ws, const int* windows, unsigned char* out, int B, int H, int W,
                           int hc, int wc, int* uncovered, const unsigned char* label, int Hl, int Wl, const unsigned char* lut, const int* ymap,
                           const int* xmap, const int* slots, int n_slots, int64_t* counts, mmsa_stream_t stream);

/* --- calibration of the confidence map (the probability of the predicted class, float32, written next to every class map): reliability bins of a uint8
 *     class map and its confidence map against a uint8 label map.  cal = int64 [n_slots, 3, bins], rows total / correct / conf_sum per confidence bin.
 *     The label side -- lut, ymap / xmap (both or neither, clamped into the label map), slots (HOST int [B]) -- is mmsa_eval_confusion_u8's.  Per pixel:
 *       it takes part iff its transformed label l = lut[label byte] is a class, l < C (ignored, 255, and kept-but-out-of-range labels take no part);
 *       it is correct iff pred == l (a prediction of 255, uncovered, never is);
 *       c = conf with NaN and negative values -> 0.0f and values above 1 -> 1.0f;
 *       bin k = min(bins - 1, (int)(c * (float)bins)): one float32 product, truncated (conf == 1 falls into the last bin);
 *       conf_sum gets floor(c * 2^24) (the scaling is exact): mean confidence = conf_sum / (2^24 * total), below the float64 mean by less than 2^-24.
 *     The call ADDS into cal (the caller zeroes it): integer sums, the same bytes whatever the order of arrival; int64 holds 2^39 pixels per bin and slot.
 *     pred and label may sit at any byte address, conf at any 4-byte aligned one.  2 <= C <= 254, 1 <= bins <= 64, 1 <= B <= 64. --- */
int mmsa_eval_calibration(const unsigned char* pred, const float* conf, const unsigned char* label, int B, int H, int W, int Hl, int Wl,
                          const unsigned char* lut, int C, const int* ymap, const int* xmap, const int* slots, int n_slots, int bins, int64_t* cal,
                          mmsa_stream_t stream);

/* --- selective evaluation: one confusion matrix per confidence bin, and the thresholded map those counts describe.  The project's own definitions (the
 *     reference has no such step), each reused verbatim from the two entries above so that the three reductions agree exactly:
 *       label side (mmsa_eval_confusion_u8): l = lut[label byte]; a pixel with l == 255 is ignored and counted nowhere; otherwise row = min(l, C) and
 *         col = min(pred, C); with ymap / xmap (both or neither) the label is read at [ymap[y], xmap[x]], clamped into the label map;
 *       confidence side (mmsa_eval_calibration): c = conf with NaN, negative values and -0.0 -> 0.0f, values above 1 and +inf -> 1.0f;
 *         bin k = min(bins - 1, (int)(c * (float)bins)): ONE float32 product, truncated, no contraction;
 *       counts[slot][k][row][col] += 1 for every pixel that is not ignored: int64 [n_slots, bins, C + 1, C + 1].  Row C (kept labels outside [0, C)) is
 *         counted, as in mmsa_eval_confusion_u8; mmsa_eval_calibration drops those pixels.
 *     What follows: (1) the sum over k is mmsa_eval_confusion_u8's [C + 1, C + 1] matrix of the same map; (2) the rows < C of bin k sum to
 *     mmsa_eval_calibration's total[k], and the trace of its [:C, :C] block is correct[k]; (3) the plain confusion counts of the map mmsa_abstain_u8 writes at
 *     min_bin = k0 are counts[k0:].sum(0) with the row sums of counts[:k0] added into column C.
 *     The call ADDS into counts (the caller zeroes it): integer sums, the same bytes whatever the order of arrival.  pred and label may sit at any byte
 *     address, conf at any 4-byte aligned one.  2 <= C <= 126 (a workgroup keeps (C + 1)^2 uint32 cells per resident bin in 64 KiB of LDS; where not all
 *     bins fit, groups of bins each make a pass over the pixels within the one launch), 1 <= bins <= 64, 1 <= B <= 64; slots: HOST int [B].
 *   abstain_u8: out[i] = pred[i] where bin(conf[i]) >= min_bin, 255 elsewhere, i < n, with the SAME clamp and bin; 0 <= min_bin <= bins (min_bin == bins
 *     abstains everywhere, 0 copies); out may be pred itself (any other overlap is an error of the caller); 1 <= n < 2^40. --- */
int mmsa_eval_selective(const unsigned char* pred, const float* conf, const unsigned char* label, int B, int H, int W, int Hl, int Wl,
                        const unsigned char* lut, int C, const int* ymap, const int* xmap, const int* slots, int n_slots, int bins, int64_t* counts,
                        mmsa_stream_t stream);
int mmsa_abstain_u8(const unsigned char* pred, const float* conf, long n, int bins, int min_bin, unsigned char* out, mmsa_stream_t stream);

/* --- temperature scaling (the reference has no such step): the confidence of softmax(x / T) in place of softmax(x), and the fit of T.
 *     The tempered softmax is the confidence maps' softmax with ONE more float32 product: e_c = expf((x_c - m) * it), it = float32(1 / float64(T)) made by
 *     the caller (finite and > 0, else MMSA_ERR_ARG); m, the sum in class order and the division are unchanged, and conf = expf((m - m) * it) / s.  No
 *     contraction.  With it == 1.0f the product is exact: each `_t` entry then writes the bytes of its sibling.  T > 0 never changes a class map.
 *   APPLY: each `_t` entry is its sibling above with `inv_temperature` before `stream`: same arguments, same checks, same class map, the same choice of
 *     kernel form (slide_argmax_conf_t: the per-lane LDS column up to 64 classes, the second pass from 65 on; slide_argmax_resized_conf_t: slots / scanning).
 *   FIT, temperature_sweep_nchw: ONE pass over a logits canvas [B, C, H, W] (what mmsa_bilinear_accum_nchw / mmsa_div_count_nchw leave, at any size or cut)
 *     for J temperatures at once.  sweep = int64 [n_slots, J, 4, bins], rows total / correct / conf_sum / nll_sum per temperature and confidence bin.  The
 *     label side -- lut, ymap / xmap (both or neither, clamped into the label map), slots (HOST int [B]) -- is mmsa_eval_confusion_u8's.  Per pixel:
 *       it takes part iff l = lut[label byte] is a class, l < C (mmsa_eval_calibration's rule);
 *       m = max_c x_c from x_0; p = the first argmax (mmsa_argmax_nchw's); correct iff p == l;
 *       for every j: s_j = e_0, s_j += e_c in class order, e_c = expf((x_c - m) * it_j); conf_j = expf((m - m) * it_j) / s_j, clamped and binned as in
 *         mmsa_eval_calibration (bin k = min(bins - 1, (int)(c * (float)bins)), conf_sum gets floor(c * 2^24));
 *         nll_j = logf(s_j) - (x_l - m) * it_j (no contraction), nll_sum gets floor(clamp(nll_j, 0, 1024) * 2^20), NaN counting as 1024.
 *     So rows 0 .. 2 of temperature j are mmsa_eval_calibration's bins of (mmsa_argmax_nchw of the canvas, the maximum over C of
 *     mmsa_softmax_flip_accum_nchw_t at it_j), bit for bit, and the sum of row 3 over the bins / (2^20 * the sum of row 0) is the mean NLL at T_j.
 *     The call ADDS into sweep (the caller zeroes it): integer sums, the same bytes whatever the order of arrival; int64 holds 2^33 capped pixels per cell.
 *     inv_temperatures: HOST float [J], copied into the launch arguments.  logits at any 4-byte aligned address, label at any byte address.
 *     2 <= C <= 254, 1 <= J <= 16, 1 <= bins <= 64, 1 <= B <= 64. --- */
int mmsa_slide_argmax_conf_t(const float* logits, int n, int C, int hs, int ws, const int* windows, unsigned char* out, float* conf, int B, int H, int W,
                             int hc, int wc, int* uncovered, float inv_temperature, mmsa_stream_t stream);
int mmsa_slide_argmax_resized_conf_t(const float* logits, int n, int C, int hs, int ws, const int* windows, unsigned char* out, float* conf, int B, int H,
                                     int W, int hc, int wc, int Hd, int Wd, int Hcut, int Wcut, int* uncovered, float inv_temperature, mmsa_stream_t stream);
int mmsa_softmax_flip_accum_nchw_t(const float* logits, float* acc, int B, int C, int H, int W, int flip, int accumulate, int finish_div,
                                   float inv_temperature, mmsa_stream_t stream);
int mmsa_temperature_sweep_nchw(const float* logits, const unsigned char* label, int B, int C, int H, int W, int Hl, int Wl, const unsigned char* lut,
                                const int* ymap, const int* xmap, const int* slots, int n_slots, const float* inv_temperatures, int J, int bins,
                                int64_t* sweep, mmsa_stream_t stream);

/* --- uncertainty maps (the reference has no such step): one of the two other standard per-pixel scores in the confidence's place, score float32 [B, Ho, Wo] in
 *     [0, 1], higher = more certain, 0 where the map is 255 -- what mmsa_eval_calibration, mmsa_eval_selective and mmsa_abstain_u8 take as `conf`.  Both are
 *     formed from the float32 probabilities p_c the confidence paths produce (one view: e_c / s of the tempered softmax above; several views: their mean), with
 *     bi the class the map names, no contraction:
 *       kind 1, top-2 margin:  p[bi] - p2, p2 = the largest p_c over c != bi (class order, `>`): one float32 subtraction; C == 1: p[bi];
 *       kind 2, entropy score: max(0, 1 - H * inv_log_c), H = sum_c (p_c > 0 ? -(p_c * logf(p_c)) : 0) in class order from the first term;
 *         inv_log_c = float32(1 / log(float64(C))) made by the caller, 0 for C == 1 (the score is then 1); finite and >= 0, else MMSA_ERR_ARG.
 *     Any other kind: MMSA_ERR_ARG.  inv_temperature as in the `_t` entries (1.0f: the untempered softmax, exactly).
 *   argmax_score_nchw: mmsa_argmax_max_nchw with the score in the maximum's place, on a canvas of probabilities [B, C, H, W]; bi = their first maximum.
 *   slide_argmax_score / slide_argmax_resized_score: mmsa_slide_argmax_conf_t / mmsa_slide_argmax_resized_conf_t with the score in the confidence's place
 *     (same arguments, same checks, same class map; `kind` before inv_temperature, inv_log_c behind it): bit for bit argmax_score_nchw on the
 *     probabilities of the canvas path.  Frame size: a per-lane LDS column up to 64 classes, three recomputing passes from 65 on; rescaled: recomputing. --- */
int mmsa_argmax_score_nchw(const float* prob, unsigned char* out, float* score, int B, int C, int H, int W, int kind, float inv_log_c, mmsa_stream_t stream);
int mmsa_slide_argmax_score(const float* logits, int n, int C, int hs, int ws, const int* windows, unsigned char* out, float* score, int B, int H, int W,
                            int hc, int wc, int* uncovered, int kind, float inv_temperature, float inv_log_c, mmsa_stream_t stream);
int mmsa_slide_argmax_resized_score(const float* logits, int n, int C, int hs, int ws, const int* windows, unsigned char* out, float* score, int B, int H,
                                    int W, int hc, int wc, int Hd, int Wd, int Hcut, int Wcut, int* uncovered, int kind, float inv_temperature,
                                    float inv_log_c, mmsa_stream_t stream);

/* --- top-k maps (the reference has no such step): the first K classes of every pixel and their probabilities, 1 <= K <= 8, rank-major:
 *     classes uint8 [K, B, Ho, Wo], probs float32 [K, B, Ho, Wo] -- every rank plane is a class map / confidence map in the format every other entry takes.
 *     The probabilities are the float32 p_c the confidence paths form (one view: e_c / s of the tempered softmax above; several views: their mean); only
 *     comparisons and moves are added, no rounding:
 *       rank 0      = bi, the class the map names, with p[bi]: classes[0] IS the class map, probs[0] IS the confidence map, bit for bit;
 *       rank r >= 1 = among the classes not yet ranked the one with the largest p_c, the lowest class index among equal values (class order, `>`):
 *                     probs[0] - probs[1], one float32 subtraction, IS the top-2 margin for C >= 2;
 *       rank r >= C = class 255 with probability 0; a pixel whose map byte is 255 (uncovered) has 255 / 0 at every rank.
 *     K outside 1..8, C > 255 or a null pointer: MMSA_ERR_ARG with a message.
 *   slide_argmax_topk: mmsa_slide_argmax_conf_t with the K planes in the place of out / conf (same arguments, same checks, same class map in plane 0; K before
 *     inv_temperature, which is always given: 1.0f is the untempered softmax, exactly).  A per-lane LDS column up to 64 classes, three recomputing passes from
 *     65 on; the rank list of a pixel stays in registers (2 / 4 / 8 slots, the smallest that holds K).
 *   argmax_topk_nchw: on a canvas of probabilities [B, C, H, W].  first == NULL: bi = their first maximum (the augmented path's map, as argmax_score_nchw).
 *     first = a uint8 map [B, H, W]: bi = its byte -- the one-view canvas path, whose map is the argmax of the LOGITS (two logits can round to one
 *     probability); a byte that is no class of the canvas (255) gives 255 / 0 at every rank.  first may be `classes` itself (plane 0, in place): a lane reads
 *     its byte before it writes.  Bit for bit slide_argmax_topk on the probabilities of the canvas path.
 *   eval_topk_u8: counts int64 [n_slots, C, K + 1], ADDED to (the caller zeroes it).  The label side -- lut, ymap / xmap (both or neither, clamped into the
 *     label map), slots (HOST int [B]) -- is mmsa_eval_confusion_u8's.  A pixel takes part iff l = lut[label byte] is a class, l < C; it adds 1 at
 *     [slot, l, r], r = the first rank whose class byte equals l, K if none does.  Column r is the diagonal of mmsa_eval_confusion_u8 on plane r, row l sums to
 *     row l of plane 0's matrix; the cumulative column sums are the top-1 .. top-K pixel accuracies.  Integer sums: the same bytes whatever the order of
 *     arrival.  2 <= C <= 255, 1 <= B <= 64. --- */
int mmsa_slide_argmax_topk(const float* logits, int n, int C, int hs, int ws, const int* windows, unsigned char* classes, float* probs, int B, int H, int W,
                           int hc, int wc, int* uncovered, int K, float inv_temperature, mmsa_stream_t stream);
int mmsa_argmax_topk_nchw(const float* prob, const unsigned char* first, unsigned char* classes, float* probs, int B, int C, int H, int W, int K,
                          mmsa_stream_t stream);
int mmsa_eval_topk_u8(const unsigned char* classes, int K, const unsigned char* label, int B, int H, int W, int Hl, int Wl, const unsigned char* lut, int C,
                      const int* ymap, const int* xmap, const int* slots, int n_slots, int64_t* counts, mmsa_stream_t stream);

/* --- boundary evaluation (csrc/boundary.hip): the confusion counts of a stored uint8 class map pred [B, H, W] against a label map, split into four zones by
 *     whether the pixel lies near a boundary of the label map and near a boundary of the prediction -- the integers the trimap accuracy / mIoU and the Boundary
 *     IoU are formed from.  The label side -- lut, ymap / xmap (both or neither, clamped into the label map), slots (HOST int [B]) -- is
 *     mmsa_eval_confusion_u8's.  For a pixel p of the prediction grid: the label code L(p) = lut[label[ymap[y], xmap[x]]] normalised to a class < C, C (kept
 *     but out of range: any LUT value in [C, 254]) or 255 (ignored); the prediction code P(p) = min(pred[p], C).  near_label(p) iff some pixel q OF THE IMAGE at
 *     Chebyshev distance max(|dy|, |dx|) <= radius from p has L(q) != L(p) (an ignored label is a code like any other as a neighbour); near_pred(p) the same
 *     for P.  border = 0: neighbours outside the image do not exist; border = 1: a pixel with y < radius, x < radius, y >= H - radius or x >= W - radius is near
 *     a boundary on both sides (the zero-padded erosion).
 *     counts int64 [n_slots, 4, C + 1, C + 1], ADDED to (the caller zeroes it): every pixel whose own L is not 255 adds 1 at
 *     [slot, 2 * near_label + near_pred, min(L, C), P].  The sum over the four zones is mmsa_eval_confusion_u8's matrix, bit for bit.  One launch; integer sums:
 *     the same bytes whatever the order of arrival.  1 <= radius <= 32 (a radius larger than the image is legal: every window is then the whole image),
 *     2 <= C <= 82 (one zone's histogram must fit a workgroup's LDS next to the tiles of radius 32), 1 <= B <= 64. --- */
int mmsa_eval_boundary_u8(const unsigned char* pred, const unsigned char* label, int B, int H, int W, int Hl, int Wl, const unsigned char* lut, int C,
                          const int* ymap, const int* xmap, const int* slots, int n_slots, int radius, int border, int64_t* counts, mmsa_stream_t stream);

/* --- Euclidean boundary evaluation (csrc/distance.hip): exact squared distance maps of code maps, and what is counted from two of them.
 *   boundary_distance_u8: for the code map M(y, x) = lut[src[b, ymap[y], xmap[x]]] on the grid [H, W] (lut == NULL: the byte itself; ymap / xmap both or
 *     neither, clamped into the source; without them Hs == H and Ws == W) the kernel compares BYTES and knows nothing of classes: the caller's LUT makes the
 *     codes (v -> min(v, C) for a class map; the label LUT with every value in [C, 254] mapped to C for a label map).
 *       D2(p) = min over pixels q OF THE IMAGE with M(q) != M(p) of (qy - py)^2 + (qx - px)^2; border = 1: additionally D2(p) <= db^2,
 *       db = min(y, x, H - 1 - y, W - 1 - x) + 1 (the first pixel outside the image: the Euclidean counterpart of mmsa_eval_boundary_u8's border rule).
 *     d2 uint16 [B, H, W] = D2 where D2 <= cap^2, else 65535 (FAR); 1 <= cap <= 255.  Images of a batch never see each other.  scratch: uint16 [B, H, W] of the
 *     caller's, written and read by the two launches of the call (a row pass and a column pass), never allocated here.  Every loop is bounded by the row
 *     length, by cap or by the image height.
 *   eval_boundary_d2: mmsa_eval_boundary_u8's counts with "near" = within a Euclidean radius: every pixel whose own label code L is not 255 adds 1 at
 *     [slot, 2 * (d2_label <= t) + (d2_pred <= t), min(L, C), P] of counts int64 [n_slots, 4, C + 1, C + 1], ADDED to.  pred, the label side (lut, ymap / xmap,
 *     slots: HOST int [B]) and the codes L, P are mmsa_eval_boundary_u8's; d2_pred / d2_label are uint16 [B, H, W] as boundary_distance_u8 writes them for P and
 *     for L; t = floor(radius^2), 1 <= t <= 65025 (t <= cap^2 of the maps is the caller's to keep: FAR is above every t).  The zone sum is
 *     mmsa_eval_confusion_u8's matrix.  2 <= C <= 126 (one zone's histogram in a workgroup's LDS; the zones are split over gridDim.z where four do not fit).
 *   eval_boundary_displacement: hist int64 [n_slots, 2, C + 1, cap + 2], ADDED to; bin 0 stays 0.  For every pixel whose own L is not 255: where
 *     d2_label <= 2 (a label-boundary pixel: a pixel with another label code among its 8 neighbours) 1 is added at [slot, 0, min(L, C), k(d2_pred)]; where
 *     d2_pred <= 2, 1 at [slot, 1, P, k(d2_label)].  k(d2) = the smallest integer k >= 1 with k^2 >= d2, exact; cap + 1 for FAR.  cap is the maps' cap
 *     (with cap = 1 the value 2 is FAR, and only pixels with another code among their 4 neighbours are boundary pixels).  (C + 1) * (cap + 2) <= 16320 (one
 *     side's uint32 histogram in a workgroup's LDS): 62 classes at cap 255, 246 at cap 64.
 *   A limit broken or a null pointer: MMSA_ERR_ARG with a message, before any launch.  Integer sums: the same bytes whatever the order of arrival. --- */
int mmsa_boundary_distance_u8(const unsigned char* src, int B, int Hs, int Ws, const unsigned char* lut, const int* ymap, const int* xmap, int H, int W,
                              int cap, int border, unsigned short* scratch, unsigned short* d2, mmsa_stream_t stream);
int mmsa_eval_boundary_d2(const unsigned char* pred, const unsigned char* label, int B, int H, int W, int Hl, int Wl, const unsigned char* lut, int C,
                          const int* ymap, const int* xmap, const int* slots, int n_slots, const unsigned short* d2_pred, const unsigned short* d2_label,
                          int t, int64_t* counts, mmsa_stream_t stream);
int mmsa_eval_boundary_displacement(const unsigned char* pred, const unsigned char* label, int B, int H, int W, int Hl, int Wl, const unsigned char* lut,
                                    int C, const int* ymap, const int* xmap, const int* slots, int n_slots, const unsigned short* d2_pred,
                                    const unsigned short* d2_label, int cap, int64_t* hist, mmsa_stream_t stream);

/* --- segment-level evaluation (csrc/components.hip): the connected components of code maps, and what is counted from two of them.
 *   components_u8: the code map M(y, x) = lut[src[b, ymap[y], xmap[x]]] on the grid [H, W] is mmsa_boundary_distance_u8's (lut == NULL: the byte itself; ymap /
 *     xmap both or neither, clamped into the source; without them Hs == H and Ws == W); the kernels compare BYTES: 255 and C are codes like any other.  Two
 *     pixels of one image are connected iff they are 4- or 8-neighbours (connectivity = 4 or 8) and hold the same code; a component is a maximal connected set.
 *     root int32 [B, H, W]: root[b, y, x] = the smallest linear index y * W + x of the pixel's component within its own image -- canonical, the same bytes
 *     whatever the schedule.  B * H * W < 2^31, B <= 65535.  root is also the working plane of the (up to) three launches of the call -- a tile pass, a merge
 *     pass over the tile borders, a flatten pass; no scratch.  No workgroup waits for another; every loop follows strictly falling indices or is bounded by
 *     the tile's pixel count, and is capped by that size besides.
 *   component_area: area int32 [B, H, W] (not root): the pixel count of the component at its root pixel, 0 elsewhere; the plane is zeroed, then added to (one
 *     add per wave and distinct root).  root is a plane as components_u8 writes it; a value outside [0, H * W) is clamped, never followed outside the plane.
 *   suppress_small_u8: out[p] = fill where area[root[p]] < min_area, pred[p] elsewhere; out may be pred.  min_area >= 1 (1: the identity), 0 <= fill <= 255.
 *   eval_segments: pred, the label side (lut, ymap / xmap, slots: HOST int [B]) and the codes L (a class < C, C, or 255 = ignored), P = min(pred, C) are
 *     mmsa_eval_confusion_u8's; root_pred / root_label are int32 [B, H, W] as components_u8 writes them for P and for L.  scratch int32 [4, B, H, W] is zeroed
 *     here; every pixel whose own L is not 255 adds 1 at scratch[0][root_label[p]] and scratch[2][root_pred[p]], and where L < C and P == L also at
 *     scratch[1][root_label[p]] and scratch[3][root_pred[p]]: area and hits of the label segments (side 0) and of the prediction segments (side 1), whose
 *     area therefore excludes ignored pixels.  Then every root pixel with area > 0 and code c < C adds 1 at [slot, side, c, s, k] of counts int64
 *     [n_slots, 2, C, 24, bins + 1], ADDED to: s = min(23, floor(log2 area)), k = floor(bins * hit / area) in 64-bit integers (k == bins iff the segment is
 *     covered completely); 1 <= bins <= 64, 2 <= C <= 254, 1 <= B <= 64.
 *   A limit broken or a null pointer: MMSA_ERR_ARG with a message, before any launch.  Integer sums: the same bytes whatever the order of arrival. --- */
int mmsa_components_u8(const unsigned char* src, int B, int Hs, int Ws, const unsigned char* lut, const int* ymap, const int* xmap, int H, int W,
                       int connectivity, int* root, mmsa_stream_t stream);
int mmsa_component_area(const int* root, int B, int H, int W, int* area, mmsa_stream_t stream);
int mmsa_suppress_small_u8(const unsigned char* pred, const int* root, const int* area, int B, int H, int W, int min_area, int fill, unsigned char* out,
                           mmsa_stream_t stream);
int mmsa_eval_segments(const unsigned char* pred, const unsigned char* label, int B, int H, int W, int Hl, int Wl, const unsigned char* lut, int C,
                       const int* ymap, const int* xmap, const int* slots, int n_slots, const int* root_pred, const int* root_label, int bins, int* scratch,
                       int64_t* counts, mmsa_stream_t stream);

/* --- panoptic quality (Kirillov et al., "Panoptic Segmentation", CVPR 2019): which prediction segment IS which label segment (csrc/pairs.hip).  Maps, codes,
 *   connectivity and roots are components_u8's and eval_segments'.  A pixel takes part iff its own label code L is not 255; a HIT pixel has L < C and
 *   P == L; inter(p, g) = the hit pixels with root_pred == p and root_label == g; area_g / area_p = planes 0 / 2 of eval_segments' scratch.
 *   segment_pairs: ONE launch fills an open-addressing table with the intersections: keys int64 [capacity] (set to all-ones = empty by the entry), counts
 *     int32 [capacity] (zeroed by the entry), capacity a power of two, 2 .. 2^30.  Every hit pixel of image b forms key = ((b * H * W + root_label) << 31) |
 *     root_pred; counts[slot of key] = inter.  slot = (key * 0x9e3779b97f4a7c15 mod 2^64) >> (64 - log2 capacity), then linear probing over at most
 *     min(128, capacity) slots; a key that finds none adds its pixels to *overflow (DEVICE int, zeroed by the CALLER, as `uncovered` of the class-map entries)
 *     and is dropped.  Which key sits in which slot depends on the schedule; the multiset of (key, count) and -- while nothing is dropped -- the set of
 *     occupied slots do not.  2 <= C <= 254, B * H * W < 2^31, B <= 65535.
 *   eval_panoptic: the label side (lut, ymap / xmap, slots: HOST int [B]) is eval_segments'; planes = its scratch, as that entry left it; keys / counts as
 *     segment_pairs left them.  match int32 [2, B, H, W] is set to -1 here.  Launch 1, a lane per slot: an occupied slot with 3 * inter > area_p + area_g
 *     (IoU > 1/2, strict; at most one per segment) writes match[0][b][root_label] = root_pred and match[1][b][root_pred] = root_label and, where the label
 *     code c at root_label is < C, adds 1 at [slot, c, s, 0] (TP) and floor(inter * 2^24 / (area_p + area_g - inter)) at [slot, c, s, 3] of pq_counts int64
 *     [n_slots, C, 24, 4], ADDED to; s = min(23, floor(log2 area_g)).  Launch 2, a lane per pixel: a label root with area_g > 0, c < C and no match adds 1
 *     at [slot, c, s, 2] (FN); a prediction root with area_p > 0, P < C and no match adds 1 at [slot, P, min(23, floor(log2 area_p)), 1] (FP).
 *     2 <= C <= 254, 1 <= B <= 64, n_slots * C * 96 < 2^31. --- */
int mmsa_segment_pairs(const unsigned char* pred, const unsigned char* label, int Hl, int Wl, const unsigned char* lut, int C, const int* ymap,
                       const int* xmap, const int* root_pred, const int* root_label, int B, int H, int W, int64_t* keys, int* counts, long capacity,
                       int* overflow, mmsa_stream_t stream);
int mmsa_eval_panoptic(const unsigned char* pred, const unsigned char* label, int B, int H, int W, int Hl, int Wl, const unsigned char* lut, int C,
                       const int* ymap, const int* xmap, const int* slots, int n_slots, const int* root_pred, const int* root_label, const int* planes,
                       const int64_t* keys, const int* counts, long capacity, int* match, int64_t* pq_counts, mmsa_stream_t stream);

/* --- the segment table (csrc/segtable.hip): the segments of a code map handed out -- dense ids, and one record per segment.  The code map (src, lut, ymap /
 *   xmap, Hs x Ws on the grid H x W) and root int32 [B, H, W] are components_u8's, root as that entry wrote it for this code map.
 *   segment_table: a component of image b is LISTED iff its area >= min_area and its code < void_from (the class count C: the classes only; 256: every code,
 *     C and 255 included).  min_area == 1 needs no area; min_area > 1 reads `area` as mmsa_component_area wrote it for root.  The listed segments of an image
 *     are numbered 0 .. n_b - 1 in ascending order of their root index (the raster order of their first pixel): canonical, the same bytes whatever the schedule.
 *     count int32 [B] = n_b, also where it exceeds capacity.  ids int32 [B, H, W] = the number of the pixel's segment, -1 where it is not listed; it does not
 *     depend on capacity.  records int64 [B, capacity, 10], zeroed here: row k < min(n_b, capacity) = ROOT, CLASS (the code), AREA, X0, Y0, X1, Y1 (the box,
 *     inclusive), SUM_X, SUM_Y, SUM_Q; the rows of the segments from capacity on are dropped (count[b] > capacity shows it), every other row stays zero.
 *     SUM_Q = the sum of floor(c * 2^24) over the segment's pixels, c = values float32 [B, H, W] clamped as in mmsa_eval_calibration (NaN, negatives, -0.0 ->
 *     0; above 1, +inf -> 1); 0 with values == NULL.  scratch int32 [B * ceil(H * W / 2048)]: the block counts of the prefix sum.  root, ids and scratch are
 *     three buffers.  Four launches -- flag counts per 2048 pixels, their prefix sums (one workgroup per image), ids and row heads at the root pixels, then a
 *     lane per pixel that writes its id and adds itself to its row by 64-bit atomics: a wave reduces its lanes per distinct id in registers (8 rounds, then
 *     lane by lane), the four waves of a workgroup merge their first id through LDS, and a wave issues one add, one min and one max instruction for all of
 *     its rounds.  No workgroup waits for another; every loop is bounded by an index or a block count.  B * H * W < 2^31, B <= 65535, B * capacity < 2^31.
 *   select_segments_u8: out[p] = fill where 0 <= ids[p] < capacity and keep[b][ids[p]] == 0, pred[p] elsewhere (ids -1 or >= capacity: unchanged); keep uint8
 *     [B, capacity]; out may be pred.  0 <= fill <= 255.
 *   A limit broken or a null pointer: MMSA_ERR_ARG with a message, before any launch.  Integer sums: the same bytes whatever the order of arrival. --- */
int mmsa_segment_table(const unsigned char* src, int B, int Hs, int Ws, const unsigned char* lut, const int* ymap, const int* xmap, int H, int W,
                       const int* root, const int* area, const float* values, int min_area, int void_from, int capacity, int* count, int* ids,
                       int64_t* records, int* scratch, mmsa_stream_t stream);
int mmsa_segment_table_block(void); /* the pixels per word of segment_table's scratch in THIS build (2048): scratch holds B * ceil(H * W / block) words */
int mmsa_select_segments_u8(const unsigned char* pred, const int* ids, const unsigned char* keep, int B, int H, int W, int capacity, int fill,
                            unsigned char* out, mmsa_stream_t stream);

/* --- segments tracked across frames (csrc/track.hip): persistent ids by IoU match.  Image b of one call follows image b of the call before (B parallel
 *   streams).  ids int32 [B, H, W], count int32 [B] and records int64 [B, rows, 10] are segment_table's of the CURRENT frame, rows = its capacity R.  A segment
 *   of either frame takes part iff its id is in [0, R); ids -1 and ids >= R take part nowhere.  inter(k, j) = the pixels with ids_cur == k and ids_prev == j;
 *   k CONTINUES j iff 3 * inter > AREA_k + AREA_j (IoU > 1/2, strict, in 64 bits) and, with same_class = 1, CLASS_k == CLASS_j: at most one j per k and one k
 *   per j pass (two j of one k would need inter1 + inter2 > AREA_k; the class test only removes candidates), so matches never conflict.
 *   track_pairs: TWO launches.  The first, a lane per slot, empties the table: keys int64 [capacity] to all-ones = empty, counts int32 [capacity] to 0;
 *     capacity a power of two, 2 .. 2^30.  (A launch where segment_pairs has two memsets: a captured sequence with the memsets was seen to replay wrongly,
 *     cause not known -- csrc/track.hip, track_empty_kernel.)  The second, a lane per pixel, fills the table as segment_pairs does (the same device code,
 *     csrc/pair_table.h).  Every pixel of
 *     image b whose two ids take part forms key = ((b * rows + id_cur) << 31) | id_prev; counts[slot of key] = inter.  The slot, the probing over at most
 *     min(128, capacity) slots and *overflow (DEVICE int, zeroed by the CALLER, added to by the pixels of the keys that found no slot) are segment_pairs'.
 *     Which key sits in which slot depends on the schedule; the multiset of (key, count) and -- while nothing is dropped -- the set of occupied slots do not.
 *     B * H * W < 2^31, B <= 65535, 1 <= rows, B * rows < 2^31.
 *   track_update: keys / counts as track_pairs left them for (ids_cur, prev_ids).  The previous frame lives in the caller's buffers at FIXED addresses:
 *     prev_ids int32 [B, H, W], prev_rows int32 [B, rows, 4] = CLASS, AREA, TRACK, AGE and prev_count int32 [B]; prev_count[b] = 0 (and prev_ids -1) is an
 *     image without a previous frame: everything is born, nothing ends.  state int32 [B, rows, 4] = TRACK, AGE, PREV, INTER: row k < min(count[b], rows) of
 *     a segment that continues j = TRACK of j, AGE of j + 1, j, inter(k, j); of any other = next_track[b] + (the non-continuing rows k' < k), 1, -1, 0 -- new
 *     ids in ascending k, the raster order of the first pixel: canonical, the same bytes whatever the schedule.  Every row from min(count[b], rows) on is
 *     (-1, 0, -1, 0).  succ int32 [B, rows]: at a previous row the current row that continues it, -1 elsewhere; prev_area int32 [B, rows]: at a continued
 *     row AREA of its predecessor, 0 elsewhere.  stats int32 [B, 3] = continued, born, ended (the previous rows below min(prev_count[b], rows) that nothing
 *     continues) of this frame; the same three are ADDED to totals int64 [B, 3]; next_track int32 [B] grows by `born`.  tracks int32 [B, H, W] or NULL:
 *     TRACK of the pixel's row, -1 where its id takes part nowhere.  Then prev_ids = ids_cur, prev_rows = (CLASS, AREA, TRACK, AGE) of every row and
 *     prev_count = count.  Four launches -- a lane per row (the rows to "unmatched"), a lane per table slot (the test; conflict-free by uniqueness), ONE
 *     workgroup per image (a scan of the flags "not continued" in trips of track_trip() = 1024 rows with a carry, bounded by rows), a lane per pixel / row
 *     (the carry-over).  No workgroup waits for another.  state and prev_rows 16-byte aligned; ids_cur, prev_ids and tracks are three buffers; limits as above.
 *   A limit broken or a null pointer: MMSA_ERR_ARG with a message, before any launch. --- */
int mmsa_track_pairs(const int* ids_cur, const int* ids_prev, int B, int H, int W, int rows, int64_t* keys, int* counts, long capacity, int* overflow,
                     mmsa_stream_t stream);
int mmsa_track_update(const int64_t* keys, const int* counts, long capacity, const int* ids_cur, const int* count, const int64_t* records, int B, int H, int W,
                      int rows, int same_class, int* prev_ids, int* prev_rows, int* prev_count, int* succ, int* prev_area, int* state, int* stats,
                      int64_t* totals, int* next_track, int* tracks, mmsa_stream_t stream);
int mmsa_track_trip(void); /* the rows one trip of track_update's scan takes in THIS build (1024) */

/* --- run-length tables (csrc/runs.hip): the runs of a map, and the map of a table.  src [B, H, W] contiguous: uint8 (a class or code map) or int32 (the ids
 *   of segment_table, -1 included; any value).  flat_b = the pixels of image b in row-major order (order 0) or column-major order (order 1: index x * H + y,
 *   the order of COCO's mask RLE).  A HEAD is index 0 and every i > 0 with flat_b[i] != flat_b[i - 1]: runs continue across line ends; one value is ONE run.
 *   run_lengths_u8 / _i32: count int32 [B] = the heads of image b, also where it exceeds capacity.  starts, values int32 [B, capacity]: row j <
 *     min(count[b], capacity) = the flat index of the j-th head in ascending order, and flat_b there.  The rows from min(count[b], capacity) on are NOT
 *     written: the caller's bytes stay.  Lengths are not stored: length[j] = (starts[j + 1], or H * W for the last) - starts[j].  Ascending starts and the
 *     definition of a head make the table unique: the same bytes whatever the schedule.  scratch int32: one word per scan unit of run_lengths_block(0)
 *     flat indices, B * ceil(H * W / 2048) words, and for order 1 the transposed map behind them: B * H * W more words for _i32, ceil(B * H * W / 4) for
 *     _u8.  Three launches, reduce-then-scan: heads per unit, the exclusive prefix sums of the unit counts (one workgroup per image, run_lengths_block(3)
 *     counts per trip), and the units again, writing their heads at their offsets.  Order 1 first transposes the map into scratch (one more launch, 64 x 64
 *     tiles through padded LDS) and counts the rows of the copy: its flat index is the column-major index.  No workgroup waits for another; every loop is
 *     bounded by an index or a unit count.  src, count, starts, values and scratch are separate buffers.
 *   run_lengths_block(what): 0 = the pixels per scan unit (2048), 1 = the tile edge of the transpose (64), 2 = the lanes of the scan workgroup (256), 3 = the
 *     unit counts per trip of the scan (1024) in THIS build; -1 otherwise.
 *   run_decode_i32: the inverse, a lane per pixel: out int32 [B, H, W] = values[b, j] of the last row j < min(count[b], capacity) with starts[b, j] <= the
 *     pixel's flat index (a binary search, 32 steps at the most), `fill` where the image has no row.  Of an overflowed table (count[b] > capacity) the last
 *     kept run has no row behind it that ends it: its head pixel gets its value, and every pixel past that head gets `fill`.
 *   B * H * W < 2^31, B <= 65535, 1 <= capacity, B * capacity < 2^31, order 0 or 1; a limit broken or a null pointer: MMSA_ERR_ARG with a message, before
 *   any launch. --- */
int mmsa_run_lengths_u8(const unsigned char* src, int B, int H, int W, int order, int capacity, int* count, int* starts, int* values, int* scratch,
                        mmsa_stream_t stream);
int mmsa_run_lengths_i32(const int* src, int B, int H, int W, int order, int capacity, int* count, int* starts, int* values, int* scratch,
                         mmsa_stream_t stream);
int mmsa_run_lengths_block(int what);
int mmsa_run_decode_i32(const int* count, const int* starts, const int* values, int B, int H, int W, int order, int capacity, int fill, int* out,
                        mmsa_stream_t stream);

/* --- nearest-label fill (csrc/fill.hip): the holes of a byte map take the value of the nearest kept pixel of their image.  src uint8 [B, H, W] contiguous;
 *   role: DEVICE uint8 [256], the role of every byte: 0 = source (keeps its value and offers it to holes), 1 = hole (is to be filled), 2 = inert (keeps its
 *   value and offers nothing; it blocks nothing: the fill is Euclidean, not geodesic).  none_byte: any byte whose role is 1 (the caller's to keep: the row pass
 *   marks "no source within 255 columns" with it, which no source's value can be).  1 <= cap <= 255.
 *     For a hole p = (py, px): among the source pixels q of the same image with d2 = (qy - py)^2 + (qx - px)^2 <= cap^2, the one with the smallest key
 *     (d2, qy, qx), compared lexicographically -- nearest first, then topmost, then leftmost: out[p] = src[q].  No such q: out[p] = src[p].  Every pixel that
 *     is not a hole: out[p] = src[p].  d2 (uint16 [B, H, W], or NULL: not written) = 0 at every pixel that is not a hole, the taken d2 (1..65025) at a filled
 *     hole, 65535 at a hole that stays.  Images of a batch never see each other.  Integers only: the same bytes on every run.
 *   out may be src (in place).  scratch: uint16 [B, H, W] of the caller's, written and read by the two launches of the call (a row pass and a column pass, as
 *   mmsa_boundary_distance_u8's), never allocated here; scratch, d2 and the maps are separate buffers.  H * W < 2^31.  Every loop is bounded by the row
 *   length, by cap or by the image height.  A limit broken or a null pointer: MMSA_ERR_ARG with a message, before any launch. --- */
int mmsa_fill_nearest_u8(const unsigned char* src, int B, int H, int W, const unsigned char* role, int none_byte, int cap, unsigned short* scratch,
                         unsigned char* out, unsigned short* d2, mmsa_stream_t stream);

/* --- majority (mode) filter (csrc/majority.hip): every target pixel of a byte map takes the most frequent voter value of its (2 r + 1) x (2 r + 1) window.
 *   src uint8 [B, H, W] contiguous; role: DEVICE uint8 [256], the role of every byte: 0 = voter (votes with its value and may be rewritten), 1 = hole (votes
 *   nothing and is to be rewritten), 2 = inert (votes nothing, is never rewritten and blocks nothing).  1 <= radius r <= 32; all, half: 0 or 1.
 *     Votes.  The window of a pixel p of image b is the set of pixels q of the SAME image with |qy - py| <= r and |qx - px| <= r, clipped at the image border:
 *     there is no padding, a window at a corner simply holds fewer pixels.  n_v(p) = the number of voter pixels of value v in the window, T(p) = sum_v n_v(p),
 *     n_best(p) = max_v n_v(p).
 *     Winner.  w(p) = p's own value if p is a voter and n_own(p) = n_best(p) -- a tie never changes a pixel that is among the tied; otherwise the smallest v
 *     with n_v(p) = n_best(p).
 *     Targets.  Every hole pixel; with all = 1 every voter pixel as well; never an inert pixel.
 *     Result.  out[p] = w(p) iff p is a target AND T(p) > 0 AND (half = 0 OR 2 n_best(p) > T(p), strict); otherwise out[p] = src[p].
 *     support (uint16 [B, H, W], or NULL: not written) = n_best(p) at every target pixel, whether or not the half rule let it change, 0 at every other pixel;
 *     the largest value is 65^2 = 4225.  Images of a batch never see each other.  Integers only: the same bytes on every run.
 *   out must not be src (a stencil cannot run in place), and support is a separate buffer from both.  H * W < 2^31.  ONE launch; every loop is bounded by the
 *   tile, by the radius or by 256 values.  A limit broken or a null pointer: MMSA_ERR_ARG with a message, before any launch. --- */
int mmsa_majority_filter_u8(const unsigned char* src, int B, int H, int W, const unsigned char* role, int radius, int all, int half,
                            unsigned char* out, unsigned short* support, mmsa_stream_t stream);

/* --- guided vote filter (csrc/vote.hip): the joint-bilateral weighted mode filter of a byte map.  Every voter of the (2 r + 1) x (2 r + 1) window of a pixel
 *   votes for its value with a weight that falls with the difference of its guide pixel from the centre's and rises with its own confidence.
 *   src, role, all, half: as mmsa_majority_filter_u8 (roles 0 = voter, 1 = hole, 2 = inert; the window is clipped at the image border, there is no padding;
 *   targets are every hole and, with all = 1, every voter, never an inert pixel).  1 <= radius r <= 16.
 *   guide: uint8 [B, Hg, Wg, G] contiguous, G = 1 or 3, Hg >= H, Wg >= W, of which the top-left H x W is used (a padded raw frame needs no copy), with
 *     range_lut: DEVICE uint16 [255 G + 1], every entry in 0 .. 4096; or both NULL (G, Hg, Wg are not looked at then).  weight: float32 [B, H, W], or NULL.
 *     Votes.  d(p, q) = sum_c |g_p[c] - g_q[c]|, the L1 distance of two guide pixels, 0 .. 255 G.  wq(q) = min(255, (int)(clamp(weight[q]) * 256.0f)) with
 *     the clamp of the calibration bins (NaN, negatives and -0.0 -> 0, above 1 -> 1): NaN, negatives and anything below 1 / 256 vote nothing; wq = 1 without
 *     weight.  S_v(p) = sum of range_lut[d(p, q)] * wq(q) over the voter pixels q of value v in the window (range_lut = 1 without a guide),
 *     T(p) = sum_v S_v(p), S_best(p) = max_v S_v(p).  A tap adds at most 4096 * 255 < 2^20 and a window holds at most 33^2 = 1089 < 2^11 taps, so
 *     T <= 1 137 438 720 < 2^31: the uint32 sums are exact.
 *     Winner.  w(p) = p's own value if p is a voter and S_own(p) = S_best(p); otherwise the smallest v with S_v(p) = S_best(p).
 *     Result.  out[p] = w(p) iff p is a target AND T(p) > 0 AND (half = 0 OR 2 S_best(p) > T(p), strict); otherwise out[p] = src[p].  T = 0 can happen with
 *     voters in the window: zeros in the table, zero weights.
 *     support (uint32 [B, H, W], or NULL: not written) = S_best(p) at every target pixel, 0 at every other pixel.
 *     With neither guide nor weight, or with a table of ones, out and support are mmsa_majority_filter_u8's.  Images of a batch never see each other.
 *     Integers only: the same bytes on every run.
 *   out must not be src, and out and support are separate buffers from every input.  H * W < 2^31.  ONE launch; every loop is bounded by the tile, by the
 *   radius or by 256 values.  A limit broken or a null pointer: MMSA_ERR_ARG with a message, before any launch. --- */
int mmsa_vote_filter_u8(const unsigned char* src, int B, int H, int W, const unsigned char* role, int radius, int all, int half,
                        const unsigned char* guide, int Hg, int Wg, int G, const unsigned short* range_lut, const float* weight,
                        unsigned char* out, unsigned* support, mmsa_stream_t stream);

/* --- the picture of a prediction (segmentation/mmseg_custom/apis/test_bs.py:257-349, the `--show` / `--show-dir` output): `tensor2imgs` (test_bs.py:18-63) on
 *     planes 0..2 of the input tensor -> the crop `img[:h, :w]` (test_bs.py:275-276) -> `show_result` (tools/color_gt_according_palette.py:23-81:
 *     color_seg[seg == label] = color, channels reversed, img * (1 - opacity) + color_seg * opacity, .astype(uint8)), in one pass.
 *     pred: uint8 class map, pixel (b, y, x) at pred[b * pred_image_stride + y * pred_row_stride + x] (a crop of a larger map needs no copy).
 *     palette: DEVICE uint32 [npal], 1 <= npal <= 256, entry = c0 | c1 << 8 | c2 << 16 (bits 24..31 ignored); palette_reverse swaps c0 and c2 (what
 *       show_result does).  A class without an entry -- 255, the "uncovered" value of mmsa_slide_argmax, included -- has colour 0 (the zero-initialised color_seg).
 *     opacity in (0, 1] and one_minus_opacity = the double 1 - opacity, formed by the CALLER.  out[c] = uint8(double(img[c]) * one_minus_opacity +
 *       double(colour[c]) * opacity): two float64 products and one float64 sum, each rounded, no fused multiply-add, then truncation.
 *     out: uint8 [B, h, w, 3] contiguous (HWC, what mmcv.imwrite takes).
 *   render_u8: src = NULL (a black image: out = uint8(colour * opacity)) or the raw uint8 frames [B, Hs, Ws, 3], Hs >= h, Ws >= w, of which the top-left
 *     h x w is used; src_reverse swaps the frame's channels 0 and 2 first.
 *   render_denorm_f32: src = the normalised float32 tensor [B, Cs >= 3, Hs >= h, Ws >= w] the backbone read; HOST mean[3], std[3] per PLANE.  Per pixel, in
 *     float32 with one rounding per step: d[p] = n[p] * std[p] + mean[p]; img[c] = d[2 - c] when to_rgb, else d[c]; * 255.0f when mul255 (norm_by_max);
 *     truncation to uint8.  Values below 0 / from 255 up saturate to 0 / 255 and NaN gives 0 (the reference's C cast is undefined there). --- */
int mmsa_render_u8(const unsigned char* pred, long pred_image_stride, long pred_row_stride, int B, int h, int w, const unsigned* palette, int npal,
                   int palette_reverse, const unsigned char* src, int Hs, int Ws, int src_reverse, double opacity, double one_minus_opacity,
                   unsigned char* out, mmsa_stream_t stream);
int mmsa_render_denorm_f32(const unsigned char* pred, long pred_image_stride, long pred_row_stride, int B, int h, int w, const unsigned* palette, int npal,
                           int palette_reverse, const float* src, int Cs, int Hs, int Ws, const float* mean, const float* std, int to_rgb, int mul255,
                           double opacity, double one_minus_opacity, unsigned char* out, mmsa_stream_t stream);

/* --- diagnostic pictures (csrc/render_diag.hip; the reference paints the ground truth through show_result in tools/color_gt_according_palette.py and has no
 *     other): every pixel gets ONE paint chosen by a rule, then the blend of the block above.  out: uint8 [B, h, w, 3] contiguous.
 *     table: DEVICE uint32 [ntab], packed by the CALLER: bits 0..23 the colour c0 | c1 << 8 | c2 << 16 in the PICTURE's channel order (no palette_reverse
 *       here), bit 24 PAINT (0: the pixel is the source pixel unchanged, black without a source), bit 25 MARK (the blend uses mark_opacity /
 *       one_minus_mark_opacity in the place of opacity / one_minus_opacity).  All four weights are formed by the caller, each pair as in the block above.
 *       ntab must be exactly the size the picture's index rule needs (below), else MMSA_ERR_ARG.
 *     src, src_form: 0 = none (src ignored), 1 = the raw uint8 frames [B, Hs, Ws, 3] (src_reverse swaps channels 0 and 2 first), 2 = the normalised float32
 *       tensor [B, Cs >= 3, Hs, Ws] with HOST mean[3], std[3], to_rgb, mul255, de-normalised exactly as mmsa_render_denorm_f32 does it (mean / std / to_rgb /
 *       mul255 / Cs are ignored otherwise).  Hs >= h, Ws >= w: the top-left h x w is used.
 *     pred: uint8 class map, pixel (b, y, x) at pred[b * pred_image_stride + y * pred_row_stride + x].
 *     The label side -- label uint8 [B, Hl, Wl], lut [256], ymap / xmap (both or neither; the label is read at [ymap[y], xmap[x]], clamped into the label map)
 *       -- is mmsa_eval_confusion_u8's, and L is the label code of mmsa_eval_boundary_u8: a class < C, C (kept, out of range) or 255 (ignored).
 *   render_labels_u8, 1 <= C <= 254:
 *     mode 0, the ground truth: index = L < C ? L : C, ntab = C + 1; pred is not read.
 *     mode 1, the wrong pixels: index = 0 where L == 255 (ignored); 1 + pred where L < C and pred == L (correct); 257 + (wrong_by_label ? L : pred)
 *       elsewhere (wrong: L == C and pred == 255 included, as mmsa_eval_confusion_u8 counts them); ntab = 513.
 *   render_values_f32: values float32 [B, h, w] contiguous; k = min(bins - 1, (int)(c * (float)bins)) of c = the value clamped as in mmsa_eval_calibration
 *       (NaN, negatives, -0.0 -> 0; above 1, +inf -> 1), 1 <= bins <= 256.
 *     pred == NULL, the heat map: index = k, ntab = bins.
 *     pred given, the abstained pixels: index = pred where k >= min_bin, 256 + k elsewhere, 0 <= min_bin <= bins, ntab = 256 + bins: with entries 0..255 a
 *       palette and the others one MARKED colour, the picture of the map mmsa_abstain_u8 writes, without writing that map.
 *   render_band_u8: near_pred / near_label EXACTLY as mmsa_eval_boundary_u8 defines them for (radius, border), with P = min(pred, C); 1 <= radius <= 32,
 *       1 <= C <= 253 (the kernel marks a mixed window with the byte 0xFE).  pred or label may be NULL (not both): the missing map has no band.
 *     marked = ((where & 1) and near_pred) or ((where & 2) and near_label), and never a pixel whose own L is 255; where = 1, 2 or 3.
 *     index = marked ? (mark_by_label ? L : P) : 256 + (inside_by_label ? L : P); ntab = 512.  A paint by L needs label.
 *   Any limit broken, a null out / table, a source smaller than the map: MMSA_ERR_ARG with a message, before any launch. --- */
int mmsa_render_labels_u8(const unsigned char* pred, long pred_image_stride, long pred_row_stride, const unsigned char* label, int B, int h, int w, int Hl, int Wl,
                          const unsigned char* lut, int C, const int* ymap, const int* xmap, int mode, int wrong_by_label, const unsigned* table, int ntab,
                          const void* src, int src_form, int Cs, int Hs, int Ws, int src_reverse, const float* mean, const float* std, int to_rgb, int mul255,
                          double opacity, double one_minus_opacity, double mark_opacity, double one_minus_mark_opacity, unsigned char* out,
                          mmsa_stream_t stream);
int mmsa_render_values_f32(const float* values, const unsigned char* pred, long pred_image_stride, long pred_row_stride, int B, int h, int w, int bins,
                           int min_bin, const unsigned* table, int ntab, const void* src, int src_form, int Cs, int Hs, int Ws, int src_reverse,
                           const float* mean, const float* std, int to_rgb, int mul255, double opacity, double one_minus_opacity, double mark_opacity,
                           double one_minus_mark_opacity, unsigned char* out, mmsa_stream_t stream);
int mmsa_render_band_u8(const unsigned char* pred, long pred_image_stride, long pred_row_stride, const unsigned char* label, int B, int H, int W, int Hl, int Wl,
                        const unsigned char* lut, int C, const int* ymap, const int* xmap, int radius, int border, int where, int mark_by_label,
                        int inside_by_label, const unsigned* table, int ntab, const void* src, int src_form, int Cs, int Hs, int Ws, int src_reverse,
                        const float* mean, const float* std, int to_rgb, int mul255, double opacity, double one_minus_opacity, double mark_opacity,
                        double one_minus_mark_opacity, unsigned char* out, mmsa_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* MMSA_H */
