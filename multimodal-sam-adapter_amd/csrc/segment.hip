// Segmentor-side glue on device: what EncoderDecoder does with the head's logits
// (segmentation/mmseg_custom/models/segmentors/encoder_decoder.py):
//   bilinear_accum_nchw : resize(logits, size=crop.shape[2:], 'bilinear', align_corners=False) (ED:90-94) written -- or, for
//                         slide inference, ADDED (preds += F.pad(crop_seg_logit, ...), count_mat[...] += 1, ED:213-219) -- into a
//                         window (y0, x0, hc, wc) of a [B, C, Hd, Wd] canvas;
//   div_count_nchw      : preds / count_mat (ED:225);
//   argmax_nchw         : seg_logit.argmax(dim=1) (ED:477; the softmax of ED:449 is monotonic) -> uint8 class map;
//   argmax_max_nchw     : the same, and the maximum itself -> float32 [B, H, W]: on probabilities, the confidence map.
// All are one pass over the canvas, HBM-bound.
#include "common.h"
#include "eval_hist.h"

// No fused multiply-add contraction in this file: the canvas path (bilinear_accum + div_count + argmax) and the one-pass class map
// (slide_argmax) must round the SAME interpolation formula identically, or an exact tie between two classes in one of them is not a
// tie in the other (seen once in 2 073 600 pixels of a 1080 x 1920 frame, where the compiler had contracted the two differently).
#pragma clang fp contract(off)
#include "slide_taps.h"   // WindowTable, the tap arithmetic and the two-stage pixel of the rescaled class map (shared with augment.hip)
#include "softmax_px.h"   // the softmax of the confidence variants (shared with augment.hip)
#include "slide_pixel.h"  // the pixel of the frame-size class-map kernels

// The file by topic: what the variants of a class map write; the canvas path's kernels, each with its entry; the crop; the frame-size class maps (one pixel,
// csrc/slide_pixel.h); the rescaled ones (one pixel, slide_resized_pixel); the host side of the one-pass entries.  Where a definition stands does not touch a
// kernel's instruction stream: regrouping the file left every stream as it was (profiles/slide_pixel_template_isa.txt).

// ---- confidence maps: the probability of the predicted class next to every class map, conf[b, y, x] = max_c P[b, c, y, x] with P the probabilities of
// EncoderDecoder.inference (F.softmax(seg_logit, dim=1), ED:449,460), written by the launch that writes the map.  The arithmetic is csrc/softmax_px.h:
// m = max_c x_c; s = e_0, s += e_c in class order, e_c = expf(x_c - m); conf = expf(m - m) / s -- P at the first maximum, which is the largest P.
// ---- tempered confidence: softmax(x / T) in place of softmax(x) -- `it` = float32(1 / float64(T)) from the host, and every exponential is softmax_px_exp_t
// (csrc/softmax_px.h: ONE more float32 product, exact at it == 1.0f, where the `_t` kernels are their siblings bit for bit).  The class map does not depend on T > 0.
// ---- uncertainty maps: the top-2 margin or the entropy score (csrc/softmax_px.h: `kind` SCORE_MARGIN / SCORE_ENTROPY) in the confidence's place, float32
// [B, Ho, Wo] in [0, 1], higher = more certain, 0 where the map is 255 -- so that csrc/conf_bin.h and everything behind it take it unchanged.  Both are formed
// from the float32 probabilities p_c, the same operations in the canvas kernel (which reads p_c) and in the one-pass kernels (which form p_c = e_c / s of
// softmax(x * it) themselves: `it` is always an argument, its product exact at 1.0f): bit for bit the same score.
// ---- top-k maps: the first K classes of every pixel and their probabilities (csrc/softmax_px.h: TopkPx<S>, comparisons and moves on the float32 probabilities
// p_c the confidence paths form), classes uint8 / probs float32 [K, B, Ho, Wo], rank-major: plane 0 of the classes IS the class map, plane 0 of the
// probabilities IS the confidence map, and probs[0] - probs[1] is the top-2 margin, bit for bit.  The rank list lives in registers (S = 2 / 4 / 8 slots, the
// smallest that holds K: the predicates of the unrolled insert are paid per class).

// ---- the canvas path: one pass over a [B, C, H, W] canvas each, HBM-bound

__global__ __launch_bounds__(256) void bilinear_accum_kernel(const float* __restrict__ src, int C, int hs, int ws, long sstrideB,
                                                             float* __restrict__ dst, int Hd, int Wd, int y0, int x0, int hc, int wc,
                                                             float* __restrict__ count, float rh, float rw, int accumulate) {
  const int j = blockIdx.x * 256 + threadIdx.x;       // column inside the window
  if (j >= wc) return;
  const int i = blockIdx.y % hc, c = blockIdx.y / hc, b = blockIdx.z;
  // PyTorch upsample_bilinear2d, align_corners=False: src = (dst + 0.5) * in/out - 0.5, clamped at 0
  float sh = ((float)i + 0.5f) * rh - 0.5f, sw = ((float)j + 0.5f) * rw - 0.5f;
  sh = sh < 0.f ? 0.f : sh;
  sw = sw < 0.f ? 0.f : sw;
  const int h0 = min((int)sh, hs - 1), w0 = min((int)sw, ws - 1);
  const int h1 = h0 + (h0 < hs - 1 ? 1 : 0), w1 = w0 + (w0 < ws - 1 ? 1 : 0);
  const float lh = sh - (float)h0, lw = sw - (float)w0;
  const float* sp = src + (long)b * sstrideB + (long)c * hs * ws;
  const float v = (1.f - lh) * ((1.f - lw) * sp[h0 * ws + w0] + lw * sp[h0 * ws + w1]) +
                  lh * ((1.f - lw) * sp[h1 * ws + w0] + lw * sp[h1 * ws + w1]);
  const long o = (((long)b * C + c) * Hd + (y0 + i)) * Wd + (x0 + j);
  dst[o] = accumulate ? dst[o] + v : v;
  if (count && c == 0) count[((long)b * Hd + (y0 + i)) * Wd + (x0 + j)] += 1.0f;
}

extern "C" int mmsa_bilinear_accum_nchw(const float* src, long src_strideB, int B, int C, int hs, int ws, float* dst, int Hd, int Wd,
                                        int y0, int x0, int hc, int wc, float* count, int accumulate, hipStream_t stream) {
  MMSA_CHECK_ARG(src && dst && B > 0 && C > 0 && hs > 0 && ws > 0 && hc > 0 && wc > 0, "bilinear_accum_nchw: bad args");
  MMSA_CHECK_ARG(y0 >= 0 && x0 >= 0 && y0 + hc <= Hd && x0 + wc <= Wd, "bilinear_accum_nchw: window (%d,%d)+(%d,%d) outside the %dx%d canvas", y0, x0, hc, wc, Hd, Wd);
  MMSA_CHECK_ARG((long)C * hc <= 65535 && B <= 65535, "bilinear_accum_nchw: C*hc too large for the launch grid");
  dim3 grid(cdiv(wc, 256), C * hc, B);
  hipLaunchKernelGGL(bilinear_accum_kernel, grid, dim3(256), 0, stream, src, C, hs, ws, src_strideB, dst, Hd, Wd, y0, x0, hc, wc, count,
                     (float)hs / (float)hc, (float)ws / (float)wc, accumulate);
  MMSA_CHECK_LAUNCH("bilinear_accum_nchw");
  return MMSA_OK;
}

__global__ __launch_bounds__(256) void div_count_kernel(float* __restrict__ x, const float* __restrict__ count, int C, long HW, long total) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= total) return;
  const long p = i % HW;
  const long b = i / (HW * C);
  x[i] = x[i] / count[b * HW + p];
}

extern "C" int mmsa_div_count_nchw(float* x, const float* count, int B, int C, long HW, hipStream_t stream) {
  MMSA_CHECK_ARG(x && count && B > 0 && C > 0 && HW > 0, "div_count_nchw: bad args");
  const long total = (long)B * C * HW;
  hipLaunchKernelGGL(div_count_kernel, dim3(cdiv(total, 256)), dim3(256), 0, stream, x, count, C, HW, total);
  MMSA_CHECK_LAUNCH("div_count_nchw");
  return MMSA_OK;
}

// first maximum wins, like torch.argmax on ties
__global__ __launch_bounds__(256) void argmax_nchw_kernel(const float* __restrict__ x, unsigned char* __restrict__ out, int C, long HW, long total) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;   // b * HW + p
  if (i >= total) return;
  const long b = i / HW, p = i - b * HW;
  const float* xp = x + b * C * HW + p;
  float best = xp[0];
  int bi = 0;
  for (int c = 1; c < C; ++c) {
    const float v = xp[(long)c * HW];
    if (v > best) { best = v; bi = c; }
  }
  out[i] = (unsigned char)bi;
}

extern "C" int mmsa_argmax_nchw(const float* x, unsigned char* out, int B, int C, long HW, hipStream_t stream) {
  MMSA_CHECK_ARG(x && out && B > 0 && C > 0 && C <= 256 && HW > 0, "argmax_nchw: bad args (C <= 256 for the uint8 map)");
  const long total = (long)B * HW;
  hipLaunchKernelGGL(argmax_nchw_kernel, dim3(cdiv(total, 256)), dim3(256), 0, stream, x, out, C, HW, total);
  MMSA_CHECK_LAUNCH("argmax_nchw");
  return MMSA_OK;
}

// argmax_nchw_kernel that also writes the maximum: on the probabilities of the canvas paths (mmsa_softmax_flip_accum_nchw), the confidence map
// max_c P[b, c, y, x] of ED:449,460 next to the class map, from one read of the canvas.
__global__ __launch_bounds__(256) void argmax_max_nchw_kernel(const float* __restrict__ x, unsigned char* __restrict__ out, float* __restrict__ maxval, int C,
                                                              long HW, long total) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;   // b * HW + p
  if (i >= total) return;
  const long b = i / HW, p = i - b * HW;
  const float* xp = x + b * C * HW + p;
  float best = xp[0];
  int bi = 0;
  for (int c = 1; c < C; ++c) {
    const float v = xp[(long)c * HW];
    if (v > best) { best = v; bi = c; }
  }
  out[i] = (unsigned char)bi;
  maxval[i] = best;
}

extern "C" int mmsa_argmax_max_nchw(const float* x, unsigned char* out, float* maxval, int B, int C, long HW, hipStream_t stream) {
  MMSA_CHECK_ARG(x && out && maxval && B > 0 && C > 0 && C <= 256 && HW > 0, "argmax_max_nchw: bad args (C <= 256 for the uint8 map)");
  const long total = (long)B * HW;
  hipLaunchKernelGGL(argmax_max_nchw_kernel, dim3(cdiv(total, 256)), dim3(256), 0, stream, x, out, maxval, C, HW, total);
  MMSA_CHECK_LAUNCH("argmax_max_nchw");
  return MMSA_OK;
}

// argmax_max_nchw_kernel with the score in the maximum's place: on a canvas of probabilities (one view's, or the mean over augmented views).  `bi` is the
// first maximum of the probabilities; where the logits' argmax is a later class of the same probability, p[bi] and p2 are the same two values.
__global__ __launch_bounds__(256) void argmax_score_nchw_kernel(const float* __restrict__ x, unsigned char* __restrict__ out, float* __restrict__ score, int C,
                                                                long HW, long total, int kind, float ilc) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;   // b * HW + p
  if (i >= total) return;
  const long b = i / HW, p = i - b * HW;
  const float* xp = x + b * C * HW + p;
  float best = xp[0];
  int bi = 0;
  for (int c = 1; c < C; ++c) {
    const float v = xp[(long)c * HW];
    if (v > best) { best = v; bi = c; }
  }
  out[i] = (unsigned char)bi;
  float sa = 0.f, spb = 0.f;
  bool snone = true;
  for (int c = 0; c < C; ++c) score_px_class(kind, bi, c, xp[(long)c * HW], sa, spb, snone);
  score[i] = score_px_finish(kind, sa, spb, snone, ilc);
}

#define MMSA_CHECK_SCORE_KIND(name, kind) MMSA_CHECK_ARG((kind) == SCORE_MARGIN || (kind) == SCORE_ENTROPY, "%s: kind %d is neither 1 (top-2 margin) nor 2 (entropy score)", name, kind)

extern "C" int mmsa_argmax_score_nchw(const float* prob, unsigned char* out, float* score, int B, int C, int H, int W, int kind, float inv_log_c,
                                      hipStream_t stream) {
  MMSA_CHECK_ARG(prob && out && score && B > 0 && C > 0 && C <= 256 && H > 0 && W > 0, "argmax_score_nchw: bad args (C <= 256 for the uint8 map)");
  MMSA_CHECK_SCORE_KIND("argmax_score_nchw", kind);
  MMSA_CHECK_ARG(inv_log_c >= 0.f && inv_log_c < INFINITY, "argmax_score_nchw: inv_log_c must be finite and not negative (1 / log C; 0 for one class)");
  const long HW = (long)H * W, total = (long)B * HW;
  hipLaunchKernelGGL(argmax_score_nchw_kernel, dim3(cdiv(total, 256)), dim3(256), 0, stream, prob, out, score, C, HW, total, kind, inv_log_c);
  MMSA_CHECK_LAUNCH("argmax_score_nchw");
  return MMSA_OK;
}

#define MMSA_CHECK_TOPK(name, K) MMSA_CHECK_ARG((K) >= 1 && (K) <= TOPK_MAX, "%s: K = %d; 1..%d ranks are supported (the rank list of a pixel is kept in registers)", name, K, TOPK_MAX)
#define TOPK_DISPATCH(K, LAUNCH) \
  do {                           \
    if ((K) <= 2) LAUNCH(2);     \
    else if ((K) <= 4) LAUNCH(4); \
    else LAUNCH(8);              \
  } while (0)

// argmax_score_nchw_kernel with the rank list in the score's place: on a canvas of probabilities (one view's, or the mean over augmented views).  `first` NULL:
// bi = the first maximum of the probabilities (the augmented path's map); else bi = first[i], the map of the one-view canvas path, which is the argmax of the
// LOGITS (two logits can round to one probability, and the later one may be the map's).  A lane reads first[i] before it writes classes[i]: `first` may be plane 0.
template <int S>
__global__ __launch_bounds__(256) void argmax_topk_nchw_kernel(const float* __restrict__ x, const unsigned char* first, unsigned char* classes,
                                                               float* __restrict__ probs, int C, long HW, long total, int K) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;   // b * HW + p
  if (i >= total) return;
  const long b = i / HW, p = i - b * HW;
  const float* xp = x + b * C * HW + p;
  int bi = 0;
  if (first) {
    bi = first[i];
    if (bi >= C) {      // 255 = uncovered (any byte that is no class of the canvas is treated alike)
      topk_px_store_none(classes, probs, total, i, K, 0);
      return;
    }
  } else {
    float best = xp[0];
    for (int c = 1; c < C; ++c) {
      const float v = xp[(long)c * HW];
      if (v > best) { best = v; bi = c; }
    }
  }
  TopkPx<S> tk;
  topk_px_init(tk);
  for (int c = 0; c < C; ++c) topk_px_class(tk, bi, c, xp[(long)c * HW]);
  topk_px_store(tk, classes, probs, total, i, K, 0);
}

extern "C" int mmsa_argmax_topk_nchw(const float* prob, const unsigned char* first, unsigned char* classes, float* probs, int B, int C, int H, int W, int K,
                                     hipStream_t stream) {
  MMSA_CHECK_ARG(prob && classes && probs, "argmax_topk_nchw: prob, classes and probs are required");
  MMSA_CHECK_ARG(C > 0 && C <= 255, "argmax_topk_nchw: %d classes; 1..255 are supported (255 is the byte of a rank without a class)", C);
  MMSA_CHECK_TOPK("argmax_topk_nchw", K);
  MMSA_CHECK_ARG(B > 0 && H > 0 && W > 0, "argmax_topk_nchw: bad args");
  const long HW = (long)H * W, total = (long)B * HW;
#define TOPK_LAUNCH(S) hipLaunchKernelGGL(argmax_topk_nchw_kernel<S>, dim3(cdiv(total, 256)), dim3(256), 0, stream, prob, first, classes, probs, C, HW, total, K)
  TOPK_DISPATCH(K, TOPK_LAUNCH);
#undef TOPK_LAUNCH
  MMSA_CHECK_LAUNCH("argmax_topk_nchw");
  return MMSA_OK;
}

// ---- crop extraction of slide inference (ED:205-212: crop_img = img[:, :, y1:y2, x1:x2]) as one launch for a batch of windows:
// dst[k] = src[b_k, :, y0_k : y0_k + hc, x0_k : x0_k + wc].  The window table travels by value in the launch arguments.
__global__ __launch_bounds__(256) void crop_batch_kernel(const float* __restrict__ src, int C, int H, int W, float* __restrict__ dst,
                                                         int hc, int wc, WindowTable wt) {
  const int k = blockIdx.z, c = blockIdx.y / hc, i = blockIdx.y - c * hc;
  const float* s = src + (((long)wt.b[k] * C + c) * H + (wt.y0[k] + i)) * W + wt.x0[k];
  float* d = dst + (((long)k * C + c) * hc + i) * wc;
  for (int j = threadIdx.x; j < wc; j += 256) d[j] = s[j];
}

static int fill_windows(WindowTable& wt, const int* windows, int n, int B, int H, int W, int hc, int wc, const char* name) {
  MMSA_CHECK_ARG(windows && n > 0 && n <= MMSA_MAX_WINDOWS, "%s: 1..%d windows per call", name, MMSA_MAX_WINDOWS);
  wt.n = n;
  for (int k = 0; k < n; ++k) {
    wt.b[k] = windows[3 * k]; wt.y0[k] = windows[3 * k + 1]; wt.x0[k] = windows[3 * k + 2];
    if (int rc = check_window(name, -1, k, wt.b[k], wt.y0[k], wt.x0[k], hc, wc, B, H, W)) return rc;
  }
  return MMSA_OK;
}

extern "C" int mmsa_crop_batch_nchw(const float* src, int B, int C, int H, int W, const int* windows /* HOST [n,3]: image, y0, x0 */, int n,
                                    float* dst, int hc, int wc, hipStream_t stream) {
  MMSA_CHECK_ARG(src && dst && B > 0 && C > 0 && hc > 0 && wc > 0 && (long)C * hc <= 65535, "crop_batch_nchw: bad args");
  WindowTable wt;
  int rc = fill_windows(wt, windows, n, B, H, W, hc, wc, "crop_batch_nchw");
  if (rc) return rc;
  hipLaunchKernelGGL(crop_batch_kernel, dim3(1, C * hc, n), dim3(256), 0, stream, src, C, H, W, dst, hc, wc, wt);
  MMSA_CHECK_LAUNCH("crop_batch_nchw");
  return MMSA_OK;
}

// ---- class map of a whole sliding-window frame in ONE pass (ED:213-225 + ED:449,477 fused): for every pixel of image b,
//   preds[c] = sum over the windows k of image b that cover it, IN WINDOW ORDER, of bilinear_{align_corners=False}(logits_k -> hc x wc)[c]
//   out      = argmax_c preds[c] / count          (first maximum wins; count = number of covering windows, ED:219,225)
// -- the same additions in the same order as bilinear_accum (accumulate) + div_count + argmax, without the [B, C, H, W] fp32 canvas
// (207 MB for a 1080 x 1920 frame and 25 classes, written and re-read once per window).  With one full-size window per image it is
// the whole-image `resize x4 + argmax` of ED:90-94,477.  Pixels no window covers make the call fail (ED:220 asserts the same).
__global__ __launch_bounds__(256) void slide_argmax_kernel(const float* __restrict__ logits, int C, int hs, int ws, unsigned char* __restrict__ out,
                                                           int H, int W, int hc, int wc, float rh, float rw, WindowTable wt, int* __restrict__ uncovered) {
  slide_pixel<PX_MAP>(logits, C, hs, ws, out, nullptr, H, W, hc, wc, rh, rw, wt, uncovered, blockIdx.y);
}

// slide_argmax_kernel + the confusion counts of its class map in the same pass (csrc/evaluate.hip does the same from a stored map): the workgroup's
// 256-pixel segments of SLIDE_EVAL_ROWS rows go into a private LDS histogram, whose non-zero bins are added to the int64 counts of the image's slot.
// One row = one flush per 256-pixel segment is the measured choice (profiles/evaluate.txt): eight rows per workgroup cost + 28 / + 194 us over the
// plain kernel where one row costs + 19 / + 18 us (the rows of a workgroup run one after the other, with an eighth of the workgroups in flight).
// out == NULL: no map is written.
#define SLIDE_EVAL_ROWS 1
__global__ __launch_bounds__(256) void slide_argmax_eval_kernel(const float* __restrict__ logits, int C, int hs, int ws, unsigned char* __restrict__ out,
                                                                int H, int W, int hc, int wc, float rh, float rw, WindowTable wt, int* __restrict__ uncovered,
                                                                EvalLabel ev, EvalSlots es) {
  extern __shared__ unsigned eval_lds[];
  const int nbins = (C + 1) * (C + 1);
  unsigned char* lut_s = (unsigned char*)(eval_lds + nbins);
  eval_hist_init(eval_lds, lut_s, ev.lut, nbins);
  unsigned* hist = eval_lds;
  const int row1 = min(H, ((int)blockIdx.y + 1) * SLIDE_EVAL_ROWS);
  for (int row = (int)blockIdx.y * SLIDE_EVAL_ROWS; row < row1; ++row) {
    // the lanes with x >= W and the 255 pixels leave the pixel, not the kernel: the flush below has a barrier
    slide_pixel<PX_MAP, false, false, 2, true>(logits, C, hs, ws, out, nullptr, H, W, hc, wc, rh, rw, wt, uncovered, row, nullptr, 1.f, 0, 0.f, 0, 0, hist, lut_s, &ev);
  }
  eval_hist_flush(eval_lds, ev.counts + (long)es.s[blockIdx.z] * nbins, nbins);
}

// slide_argmax_kernel + the confidence map: conf[b, y, x] = max_c softmax(preds / count)[c], the probability of the class the map names (ED:449,460).  The
// sum of the exponentials needs the maximum first, so the pixel's C values are needed twice; two forms (slide_pixel.h: LDS), chosen by measurement
// (profiles/confidence.txt, profiles/slide_pixel_template.txt):
//   slide_argmax_conf_lds_kernel : the first pass keeps them in a per-lane LDS column [c][lane], as aug_argmax_kernel does -- C * 256 floats of dynamic LDS,
//                                  so C <= SLIDE_CONF_LDS_CLASSES = 64 (64 KiB); the faster form -- + 36 / + 88 us over the plain kernel where the other costs
//                                  + 70 / + 248 us (two 1024 x 1024 maps / the six-window 1080 x 1920 frame, 25 classes; profiles/slide_pixel_template.txt) --
//                                  and the one the entry takes wherever it fits;
//   slide_argmax_conf_kernel     : a second pass recomputes them (the same operations on the same inputs, the same bits): no LDS, any C the map allows.
// The recomputing form takes 118 registers, the LDS form 130 (profiles/slide_pixel_template_isa.txt).  Bit for bit max over C of
// mmsa_softmax_flip_accum_nchw on the canvas path's logits, either way.
#define SLIDE_CONF_LDS_CLASSES 64
__global__ __launch_bounds__(256) void slide_argmax_conf_kernel(const float* __restrict__ logits, int C, int hs, int ws, unsigned char* __restrict__ out,
                                                                float* __restrict__ conf, int H, int W, int hc, int wc, float rh, float rw, WindowTable wt,
                                                                int* __restrict__ uncovered) {
  slide_pixel<PX_CONF>(logits, C, hs, ws, out, conf, H, W, hc, wc, rh, rw, wt, uncovered, blockIdx.y);
}

__global__ __launch_bounds__(256) void slide_argmax_conf_lds_kernel(const float* __restrict__ logits, int C, int hs, int ws, unsigned char* __restrict__ out,
                                                                    float* __restrict__ conf, int H, int W, int hc, int wc, float rh, float rw, WindowTable wt,
                                                                    int* __restrict__ uncovered) {
  extern __shared__ float conf_lds[];      // the per-lane column [c][lane]
  slide_pixel<PX_CONF, true>(logits, C, hs, ws, out, conf, H, W, hc, wc, rh, rw, wt, uncovered, blockIdx.y, conf_lds + threadIdx.x);
}

// the two confidence kernels with the inverse temperature `it`
__global__ __launch_bounds__(256) void slide_argmax_conf_t_kernel(const float* __restrict__ logits, int C, int hs, int ws, unsigned char* __restrict__ out,
                                                                  float* __restrict__ conf, int H, int W, int hc, int wc, float rh, float rw, WindowTable wt,
                                                                  int* __restrict__ uncovered, float it) {
  slide_pixel<PX_CONF, false, true>(logits, C, hs, ws, out, conf, H, W, hc, wc, rh, rw, wt, uncovered, blockIdx.y, nullptr, it);
}

__global__ __launch_bounds__(256) void slide_argmax_conf_lds_t_kernel(const float* __restrict__ logits, int C, int hs, int ws, unsigned char* __restrict__ out,
                                                                      float* __restrict__ conf, int H, int W, int hc, int wc, float rh, float rw, WindowTable wt,
                                                                      int* __restrict__ uncovered, float it) {
  extern __shared__ float conf_lds[];      // the per-lane column [c][lane]
  slide_pixel<PX_CONF, true, true>(logits, C, hs, ws, out, conf, H, W, hc, wc, rh, rw, wt, uncovered, blockIdx.y, conf_lds + threadIdx.x, it);
}

// slide_argmax_kernel + the score map, in the two forms of the confidence (slide_pixel.h: PX_SCORE): the per-lane LDS column up to SLIDE_CONF_LDS_CLASSES
// classes -- written with x_c by the class-map pass, overwritten with e_c by the sum pass, read once more for p_c = e_c / s -- and three recomputing passes
// above that (65 .. 255 classes; slow, and allowed to be).
__global__ __launch_bounds__(256) void slide_argmax_score_kernel(const float* __restrict__ logits, int C, int hs, int ws, unsigned char* __restrict__ out,
                                                                 float* __restrict__ conf, int H, int W, int hc, int wc, float rh, float rw, WindowTable wt,
                                                                 int* __restrict__ uncovered, int kind, float it, float ilc) {
  slide_pixel<PX_SCORE, false, true>(logits, C, hs, ws, out, conf, H, W, hc, wc, rh, rw, wt, uncovered, blockIdx.y, nullptr, it, kind, ilc);
}

__global__ __launch_bounds__(256) void slide_argmax_score_lds_kernel(const float* __restrict__ logits, int C, int hs, int ws, unsigned char* __restrict__ out,
                                                                     float* __restrict__ conf, int H, int W, int hc, int wc, float rh, float rw, WindowTable wt,
                                                                     int* __restrict__ uncovered, int kind, float it, float ilc) {
  extern __shared__ float conf_lds[];      // the per-lane column [c][lane]
  slide_pixel<PX_SCORE, true, true>(logits, C, hs, ws, out, conf, H, W, hc, wc, rh, rw, wt, uncovered, blockIdx.y, conf_lds + threadIdx.x, it, kind, ilc);
}

// slide_argmax_kernel + the rank planes, in the two forms of the score (slide_pixel.h: PX_TOPK): the per-lane LDS column up to SLIDE_CONF_LDS_CLASSES
// classes, three recomputing passes above that (65 .. 255 classes).  `out` / `conf` are the planes [K, B, H, W], `plane` = B * H * W.
template <int S>
__global__ __launch_bounds__(256) void slide_argmax_topk_kernel(const float* __restrict__ logits, int C, int hs, int ws, unsigned char* __restrict__ out,
                                                                float* __restrict__ conf, int H, int W, int hc, int wc, float rh, float rw, WindowTable wt,
                                                                int* __restrict__ uncovered, int K, long plane, float it) {
  slide_pixel<PX_TOPK, false, true, S>(logits, C, hs, ws, out, conf, H, W, hc, wc, rh, rw, wt, uncovered, blockIdx.y, nullptr, it, 0, 0.f, K, plane);
}

template <int S>
__global__ __launch_bounds__(256) void slide_argmax_topk_lds_kernel(const float* __restrict__ logits, int C, int hs, int ws, unsigned char* __restrict__ out,
                                                                    float* __restrict__ conf, int H, int W, int hc, int wc, float rh, float rw, WindowTable wt,
                                                                    int* __restrict__ uncovered, int K, long plane, float it) {
  extern __shared__ float conf_lds[];      // the per-lane column [c][lane]
  slide_pixel<PX_TOPK, true, true, S>(logits, C, hs, ws, out, conf, H, W, hc, wc, rh, rw, wt, uncovered, blockIdx.y, conf_lds + threadIdx.x, it, 0, 0.f, K, plane);
}

// ---- class map of a frame at a RESCALED size in one pass (ED:227-233, 314-325, 349-360, 393-414 + ED:449,477): what `rescale=True` adds to the
// canvas above -- a second bilinear resize (align_corners=False) of the averaged logits to Hd x Wd, then the crop [:Hcut, :Wcut] -- before the argmax:
//   canvas[c, y, x]  = (sum over covering windows, in window order, of bilinear(logits_k -> hc x wc)[c]) / count       (slide_pixel.h)
//   resized[c, Y, X] = bilinear_{align_corners=False}(canvas -> Hd x Wd)                                                (bilinear_accum_kernel, write mode)
//   out[Y, X]        = first argmax_c resized[c, Y, X]
// with neither the [B, C, H, W] canvas nor the [B, C, Hd, Wd] one in memory.  An output pixel reads a 2 x 2 block of canvas pixels (its four taps; on a
// downscale the blocks of neighbouring output pixels skip canvas pixels, PyTorch's bilinear has no antialiasing); each tap is a canvas pixel of its own,
// with its own covering windows and its own count.  Both stages are the file's formula in the file's operation order (no contraction, see the top), so
// the map equals bilinear_accum + div_count + bilinear_accum + argmax + crop bit for bit.  A pixel with a tap that no window covers, or more than 8
// windows, gets 255 and is counted in `uncovered`.
// The pixel (TwoStagePixel: set-up and value; why a tap keeps four windows in registers): csrc/slide_taps.h.
// CONF: the probability of the predicted class also goes to `conf` float [B, Hcut, Wcut] (0 for a 255 pixel), by a second pass over the classes in the form
// the first one took (slots or scanning), for the reason slide_pixel.h gives: the same values again, now that their maximum `best` is known.
// TEMP (with CONF): the confidence of softmax(x / T) -- the exponentials are softmax_px_exp_t with the inverse temperature `it`; the map does not depend on it.
// SCORE (without CONF / TEMP): an uncertainty score of csrc/softmax_px.h (`kind`, `ilc`) goes to `conf` in the confidence's place, from the probabilities of
// softmax(x * it) -- a third pass over the classes in the recomputing form: the sum needs the maximum, the probabilities need the sum.
template <bool CONF, bool TEMP = false, bool SCORE = false>
__device__ __forceinline__ void slide_resized_pixel(const float* __restrict__ logits, int C, int hs, int ws, unsigned char* __restrict__ out, float* __restrict__ conf,
                                                    int H, int W, int hc, int wc, float rh, float rw, int Hcut, int Wcut, float rh2, float rw2,
                                                    const WindowTable& wt, int* __restrict__ uncovered, float it = 1.f, int kind = 0, float ilc = 0.f) {
  const int X = blockIdx.x * 256 + threadIdx.x, Y = blockIdx.y, b = blockIdx.z;
  if (X >= Wcut) return;
  TwoStagePixel px;
  two_stage_setup(px, wt, b, Y, X, H, W, hc, wc, hs, ws, rh, rw, rh2, rw2);
  const long op = ((long)b * Hcut + Y) * Wcut + X;
  if (px.nmin == 0 || px.nmax > 8) {      // a tap without a window, or with more than 8: counted once per output pixel, and the pixel gets 255
    atomicAdd(uncovered, 1);
    out[op] = 255;
    if constexpr (CONF) conf[op] = 0.f;
    if constexpr (SCORE) conf[op] = 0.f;
    return;
  }
  const bool slots = px.nmax <= RESIZED_SLOTS;
  float best = -INFINITY;
  int bi = 0;
  if (slots) {
    for (int c = 0; c < C; ++c) {
      const float p = two_stage_value<false>(px, wt, b, logits, C, c, hs, ws, hc, wc, rh, rw);
      if (c == 0 || p > best) { best = p; bi = c; }      // first maximum wins, like torch.argmax on ties
    }
  } else {
    for (int c = 0; c < C; ++c) {
      const float p = two_stage_value<true>(px, wt, b, logits, C, c, hs, ws, hc, wc, rh, rw);
      if (c == 0 || p > best) { best = p; bi = c; }
    }
  }
  out[op] = (unsigned char)bi;
  if constexpr (CONF && !TEMP) {
    float s = 0.f;
    if (slots)
      for (int c = 0; c < C; ++c) s = softmax_px_sum(s, softmax_px_exp(two_stage_value<false>(px, wt, b, logits, C, c, hs, ws, hc, wc, rh, rw), best), c == 0);
    else
      for (int c = 0; c < C; ++c) s = softmax_px_sum(s, softmax_px_exp(two_stage_value<true>(px, wt, b, logits, C, c, hs, ws, hc, wc, rh, rw), best), c == 0);
    conf[op] = softmax_px_prob(softmax_px_exp(best, best), s);
  }
  // The tempered block is written out next to the untempered one, not folded into it with `TEMP ? ... : ...` on a named value: that form, the same
  // arithmetic, gave slide_argmax_resized_conf_kernel another instruction stream (profiles/temperature_isa.txt); this one leaves it as it was.
  if constexpr (CONF && TEMP) {
    float s = 0.f;
    if (slots)
      for (int c = 0; c < C; ++c) s = softmax_px_sum(s, softmax_px_exp_t(two_stage_value<false>(px, wt, b, logits, C, c, hs, ws, hc, wc, rh, rw), best, it), c == 0);
    else
      for (int c = 0; c < C; ++c) s = softmax_px_sum(s, softmax_px_exp_t(two_stage_value<true>(px, wt, b, logits, C, c, hs, ws, hc, wc, rh, rw), best, it), c == 0);
    conf[op] = softmax_px_prob(softmax_px_exp_t(best, best, it), s);
  }
  if constexpr (SCORE) {
    float s = 0.f, sa = 0.f, spb = 0.f;
    bool snone = true;
    for (int pass = 0; pass < 2; ++pass)      // 0: the sum of the exponentials; 1: the probabilities, class by class, into the score
      for (int c = 0; c < C; ++c) {
        const float v = slots ? two_stage_value<false>(px, wt, b, logits, C, c, hs, ws, hc, wc, rh, rw) : two_stage_value<true>(px, wt, b, logits, C, c, hs, ws, hc, wc, rh, rw);
        const float e = softmax_px_exp_t(v, best, it);
        if (pass == 0) s = softmax_px_sum(s, e, c == 0);
        else score_px_class(kind, bi, c, softmax_px_prob(e, s), sa, spb, snone);
      }
    conf[op] = score_px_finish(kind, sa, spb, snone, ilc);
  }
}

__global__ __launch_bounds__(256) void slide_argmax_resized_kernel(const float* __restrict__ logits, int C, int hs, int ws, unsigned char* __restrict__ out,
                                                                   int H, int W, int hc, int wc, float rh, float rw, int Hcut, int Wcut, float rh2, float rw2,
                                                                   WindowTable wt, int* __restrict__ uncovered) {
  slide_resized_pixel<false>(logits, C, hs, ws, out, nullptr, H, W, hc, wc, rh, rw, Hcut, Wcut, rh2, rw2, wt, uncovered);
}

// slide_argmax_resized_kernel + the confidence map at the rescaled / cut size: conf = max_c softmax(resized)[c] (ED:449,460), slot form and scanning form.
__global__ __launch_bounds__(256) void slide_argmax_resized_conf_kernel(const float* __restrict__ logits, int C, int hs, int ws, unsigned char* __restrict__ out,
                                                                        float* __restrict__ conf, int H, int W, int hc, int wc, float rh, float rw, int Hcut,
                                                                        int Wcut, float rh2, float rw2, WindowTable wt, int* __restrict__ uncovered) {
  slide_resized_pixel<true>(logits, C, hs, ws, out, conf, H, W, hc, wc, rh, rw, Hcut, Wcut, rh2, rw2, wt, uncovered);
}

// ... tempered
__global__ __launch_bounds__(256) void slide_argmax_resized_conf_t_kernel(const float* __restrict__ logits, int C, int hs, int ws, unsigned char* __restrict__ out,
                                                                          float* __restrict__ conf, int H, int W, int hc, int wc, float rh, float rw, int Hcut,
                                                                          int Wcut, float rh2, float rw2, WindowTable wt, int* __restrict__ uncovered, float it) {
  slide_resized_pixel<true, true>(logits, C, hs, ws, out, conf, H, W, hc, wc, rh, rw, Hcut, Wcut, rh2, rw2, wt, uncovered, it);
}

// slide_argmax_resized_kernel + the score map: a third pass over the classes in the recomputing form
__global__ __launch_bounds__(256) void slide_argmax_resized_score_kernel(const float* __restrict__ logits, int C, int hs, int ws, unsigned char* __restrict__ out,
                                                                         float* __restrict__ conf, int H, int W, int hc, int wc, float rh, float rw, int Hcut,
                                                                         int Wcut, float rh2, float rw2, WindowTable wt, int* __restrict__ uncovered, int kind,
                                                                         float it, float ilc) {
  slide_resized_pixel<false, false, true>(logits, C, hs, ws, out, conf, H, W, hc, wc, rh, rw, Hcut, Wcut, rh2, rw2, wt, uncovered, it, kind, ilc);
}

// ---- the host side of the fused evaluation entry
extern "C" int mmsa_slide_argmax_eval(const float* logits, int n, int C, int hs, int ws, const int* windows /* HOST [n,3] */, unsigned char* out /* or NULL */,
                                      int B, int H, int W, int hc, int wc, int* uncovered, const unsigned char* label, int Hl, int Wl,
                                      const unsigned char* lut, const int* ymap, const int* xmap, const int* slots /* HOST [B] */, int n_slots,
                                      int64_t* counts, hipStream_t stream) {
  MMSA_CHECK_ARG(logits && uncovered && hs > 0 && ws > 0 && hc > 0 && wc > 0 && B > 0 && H <= 65535 && B <= 65535, "slide_argmax_eval: bad args");
  EvalSlots es;
  int rc = eval_check("slide_argmax_eval", label, B, H, W, Hl, Wl, lut, C, ymap, xmap, slots, n_slots, counts, es);
  if (rc) return rc;
  WindowTable wt;
  rc = fill_windows(wt, windows, n, B, H, W, hc, wc, "slide_argmax_eval");
  if (rc) return rc;
  const EvalLabel ev = {label, lut, ymap, xmap, (unsigned long long*)counts, Hl, Wl, C};
  hipLaunchKernelGGL(slide_argmax_eval_kernel, dim3(cdiv(W, 256), cdiv(H, SLIDE_EVAL_ROWS), B), dim3(256), (size_t)(C + 1) * (C + 1) * 4 + 256, stream, logits, C, hs, ws, out,
                     H, W, hc, wc, (float)hs / (float)hc, (float)ws / (float)wc, wt, uncovered, ev, es);
  MMSA_CHECK_LAUNCH("slide_argmax_eval");
  return MMSA_OK;
}

// ---- the host side of the eight class-map entries mmsa_slide_argmax[_resized][_conf[_t] | _score]: one launcher per geometry, below every kernel it may launch.
// `conf`: the confidence (or score) map, NULL for the plain map; `it` (with `conf`): the inverse temperature of the `_t` and `_score` kernels; `kind` (with
// `conf` and `it`): the score the `_score` kernels write there, with `ilc` = 1 / log C.  The checks come in one order for every entry: the "bad args" of the
// geometry, the score arguments or the inverse temperature, the cut, the windows.
static int score_check(const char* name, const float* score, int kind, float it, float ilc) {
  MMSA_CHECK_ARG(score, "%s: bad args", name);
  MMSA_CHECK_SCORE_KIND(name, kind);
  MMSA_CHECK_INV_TEMPERATURE(name, it);
  MMSA_CHECK_ARG(ilc >= 0.f && ilc < INFINITY, "%s: inv_log_c must be finite and not negative (1 / log C; 0 for one class)", name);
  return MMSA_OK;
}

// frame size.  With `conf`: the LDS-column form of the kernel where it fits, the recomputing form otherwise.
static int slide_argmax_launch(const char* name, const float* logits, int n, int C, int hs, int ws, const int* windows, unsigned char* out, float* conf, int B, int H,
                               int W, int hc, int wc, int* uncovered, hipStream_t stream, const float* it = nullptr, const int* kind = nullptr, float ilc = 0.f) {
  MMSA_CHECK_ARG(logits && out && uncovered && C > 0 && C <= 255 && hs > 0 && ws > 0 && hc > 0 && wc > 0 && B > 0 && H <= 65535 && B <= 65535, "%s: bad args", name);
  if (kind) {
    if (int rc = score_check(name, conf, *kind, *it, ilc)) return rc;
  } else if (it) MMSA_CHECK_INV_TEMPERATURE(name, *it);
  WindowTable wt;
  if (int rc = fill_windows(wt, windows, n, B, H, W, hc, wc, name)) return rc;
#ifdef MMSA_CONF_SECOND_PASS      // measurement build only (tools/exp/confidence_bench.py): the second-pass form of the confidence for every C
  const bool lds = kind && C <= SLIDE_CONF_LDS_CLASSES;
#else
  const bool lds = C <= SLIDE_CONF_LDS_CLASSES;
#endif
  const dim3 grid(cdiv(W, 256), H, B);
  const size_t col = lds ? (size_t)C * 256 * sizeof(float) : 0;      // the per-lane LDS column
  const float rh = (float)hs / (float)hc, rw = (float)ws / (float)wc;
#define SLIDE_LAUNCH(kernel, ...) hipLaunchKernelGGL(kernel, grid, dim3(256), col, stream, logits, C, hs, ws, out, conf, H, W, hc, wc, rh, rw, wt, uncovered, ##__VA_ARGS__)
  if (!conf) hipLaunchKernelGGL(slide_argmax_kernel, grid, dim3(256), 0, stream, logits, C, hs, ws, out, H, W, hc, wc, rh, rw, wt, uncovered);
  else if (kind && lds) SLIDE_LAUNCH(slide_argmax_score_lds_kernel, *kind, *it, ilc);
  else if (kind) SLIDE_LAUNCH(slide_argmax_score_kernel, *kind, *it, ilc);
  else if (it && lds) SLIDE_LAUNCH(slide_argmax_conf_lds_t_kernel, *it);
  else if (it) SLIDE_LAUNCH(slide_argmax_conf_t_kernel, *it);
  else if (lds) SLIDE_LAUNCH(slide_argmax_conf_lds_kernel);
  else SLIDE_LAUNCH(slide_argmax_conf_kernel);
#undef SLIDE_LAUNCH
  MMSA_CHECK_LAUNCH(name);
  return MMSA_OK;
}

// rescaled or cut size
static int slide_argmax_resized_launch(const char* name, const float* logits, int n, int C, int hs, int ws, const int* windows, unsigned char* out, float* conf, int B,
                                       int H, int W, int hc, int wc, int Hd, int Wd, int Hcut, int Wcut, int* uncovered, hipStream_t stream,
                                       const float* it = nullptr, const int* kind = nullptr, float ilc = 0.f) {
  MMSA_CHECK_ARG(logits && out && uncovered && C > 0 && C <= 255 && hs > 0 && ws > 0 && hc > 0 && wc > 0 && B > 0 && H > 0 && W > 0 && B <= 65535, "%s: bad args", name);
  if (kind) {
    if (int rc = score_check(name, conf, *kind, *it, ilc)) return rc;
  } else if (it) MMSA_CHECK_INV_TEMPERATURE(name, *it);
  MMSA_CHECK_ARG(Hd > 0 && Wd > 0 && Hcut > 0 && Wcut > 0 && Hcut <= Hd && Wcut <= Wd && Hcut <= 65535,
                 "%s: the cut %dx%d must lie inside the target %dx%d (and have at most 65535 rows)", name, Hcut, Wcut, Hd, Wd);
  WindowTable wt;
  if (int rc = fill_windows(wt, windows, n, B, H, W, hc, wc, name)) return rc;
  const dim3 grid(cdiv(Wcut, 256), Hcut, B);
  const float rh = (float)hs / (float)hc, rw = (float)ws / (float)wc, rh2 = (float)H / (float)Hd, rw2 = (float)W / (float)Wd;
#define SLIDE_LAUNCH(kernel, ...) \
  hipLaunchKernelGGL(kernel, grid, dim3(256), 0, stream, logits, C, hs, ws, out, conf, H, W, hc, wc, rh, rw, Hcut, Wcut, rh2, rw2, wt, uncovered, ##__VA_ARGS__)
  if (!conf) hipLaunchKernelGGL(slide_argmax_resized_kernel, grid, dim3(256), 0, stream, logits, C, hs, ws, out, H, W, hc, wc, rh, rw, Hcut, Wcut, rh2, rw2, wt, uncovered);
  else if (kind) SLIDE_LAUNCH(slide_argmax_resized_score_kernel, *kind, *it, ilc);
  else if (it) SLIDE_LAUNCH(slide_argmax_resized_conf_t_kernel, *it);
  else SLIDE_LAUNCH(slide_argmax_resized_conf_kernel);
#undef SLIDE_LAUNCH
  MMSA_CHECK_LAUNCH(name);
  return MMSA_OK;
}

extern "C" int mmsa_slide_argmax(const float* logits, int n, int C, int hs, int ws, const int* windows /* HOST [n,3] */, unsigned char* out,
                                 int B, int H, int W, int hc, int wc, int* uncovered /* device int, zeroed by the caller */, hipStream_t stream) {
  return slide_argmax_launch("slide_argmax", logits, n, C, hs, ws, windows, out, nullptr, B, H, W, hc, wc, uncovered, stream);
}

extern "C" int mmsa_slide_argmax_conf(const float* logits, int n, int C, int hs, int ws, const int* windows /* HOST [n,3] */, unsigned char* out, float* conf,
                                      int B, int H, int W, int hc, int wc, int* uncovered /* device int, zeroed by the caller */, hipStream_t stream) {
  MMSA_CHECK_ARG(conf, "slide_argmax_conf: bad args");
  return slide_argmax_launch("slide_argmax_conf", logits, n, C, hs, ws, windows, out, conf, B, H, W, hc, wc, uncovered, stream);
}

extern "C" int mmsa_slide_argmax_conf_t(const float* logits, int n, int C, int hs, int ws, const int* windows /* HOST [n,3] */, unsigned char* out, float* conf,
                                        int B, int H, int W, int hc, int wc, int* uncovered /* device int, zeroed by the caller */, float inv_temperature,
                                        hipStream_t stream) {
  MMSA_CHECK_ARG(conf, "slide_argmax_conf_t: bad args");
  return slide_argmax_launch("slide_argmax_conf_t", logits, n, C, hs, ws, windows, out, conf, B, H, W, hc, wc, uncovered, stream, &inv_temperature);
}

extern "C" int mmsa_slide_argmax_score(const float* logits, int n, int C, int hs, int ws, const int* windows /* HOST [n,3] */, unsigned char* out, float* score,
                                       int B, int H, int W, int hc, int wc, int* uncovered /* device int, zeroed by the caller */, int kind, float inv_temperature,
                                       float inv_log_c, hipStream_t stream) {
  return slide_argmax_launch("slide_argmax_score", logits, n, C, hs, ws, windows, out, score, B, H, W, hc, wc, uncovered, stream, &inv_temperature, &kind, inv_log_c);
}

extern "C" int mmsa_slide_argmax_resized(const float* logits, int n, int C, int hs, int ws, const int* windows /* HOST [n,3] */, unsigned char* out,
                                         int B, int H, int W, int hc, int wc, int Hd, int Wd, int Hcut, int Wcut,
                                         int* uncovered /* device int, zeroed by the caller */, hipStream_t stream) {
  return slide_argmax_resized_launch("slide_argmax_resized", logits, n, C, hs, ws, windows, out, nullptr, B, H, W, hc, wc, Hd, Wd, Hcut, Wcut, uncovered, stream);
}

extern "C" int mmsa_slide_argmax_resized_conf(const float* logits, int n, int C, int hs, int ws, const int* windows /* HOST [n,3] */, unsigned char* out,
                                              float* conf, int B, int H, int W, int hc, int wc, int Hd, int Wd, int Hcut, int Wcut,
                                              int* uncovered /* device int, zeroed by the caller */, hipStream_t stream) {
  MMSA_CHECK_ARG(conf, "slide_argmax_resized_conf: bad args");
  return slide_argmax_resized_launch("slide_argmax_resized_conf", logits, n, C, hs, ws, windows, out, conf, B, H, W, hc, wc, Hd, Wd, Hcut, Wcut, uncovered, stream);
}

extern "C" int mmsa_slide_argmax_resized_conf_t(const float* logits, int n, int C, int hs, int ws, const int* windows /* HOST [n,3] */, unsigned char* out,
                                                float* conf, int B, int H, int W, int hc, int wc, int Hd, int Wd, int Hcut, int Wcut,
                                                int* uncovered /* device int, zeroed by the caller */, float inv_temperature, hipStream_t stream) {
  MMSA_CHECK_ARG(conf, "slide_argmax_resized_conf_t: bad args");
  return slide_argmax_resized_launch("slide_argmax_resized_conf_t", logits, n, C, hs, ws, windows, out, conf, B, H, W, hc, wc, Hd, Wd, Hcut, Wcut, uncovered, stream,
                                     &inv_temperature);
}

extern "C" int mmsa_slide_argmax_resized_score(const float* logits, int n, int C, int hs, int ws, const int* windows /* HOST [n,3] */, unsigned char* out,
                                               float* score, int B, int H, int W, int hc, int wc, int Hd, int Wd, int Hcut, int Wcut,
                                               int* uncovered /* device int, zeroed by the caller */, int kind, float inv_temperature, float inv_log_c,
                                               hipStream_t stream) {
  return slide_argmax_resized_launch("slide_argmax_resized_score", logits, n, C, hs, ws, windows, out, score, B, H, W, hc, wc, Hd, Wd, Hcut, Wcut, uncovered, stream,
                                     &inv_temperature, &kind, inv_log_c);
}

// mmsa_slide_argmax_conf_t with the K planes in the place of out / conf: the same checks in the same order, K's behind the geometry's.
extern "C" int mmsa_slide_argmax_topk(const float* logits, int n, int C, int hs, int ws, const int* windows /* HOST [n,3] */, unsigned char* classes, float* probs,
                                      int B, int H, int W, int hc, int wc, int* uncovered /* device int, zeroed by the caller */, int K, float inv_temperature,
                                      hipStream_t stream) {
  const char* name = "slide_argmax_topk";
  MMSA_CHECK_ARG(logits && classes && probs && uncovered, "%s: logits, classes, probs and uncovered are required", name);
  MMSA_CHECK_ARG(C > 0 && C <= 255, "%s: %d classes; 1..255 are supported (255 is the byte of a rank without a class)", name, C);
  MMSA_CHECK_ARG(hs > 0 && ws > 0 && hc > 0 && wc > 0 && B > 0 && H <= 65535 && B <= 65535, "%s: bad args", name);
  MMSA_CHECK_TOPK(name, K);
  MMSA_CHECK_INV_TEMPERATURE(name, inv_temperature);
  WindowTable wt;
  if (int rc = fill_windows(wt, windows, n, B, H, W, hc, wc, name)) return rc;
  const bool lds = C <= SLIDE_CONF_LDS_CLASSES;
  const dim3 grid(cdiv(W, 256), H, B);
  const size_t col = lds ? (size_t)C * 256 * sizeof(float) : 0;      // the per-lane LDS column
  const float rh = (float)hs / (float)hc, rw = (float)ws / (float)wc;
  const long plane = (long)B * H * W;
#define TOPK_LAUNCH(S)                                                                                                                                    \
  do {                                                                                                                                                    \
    if (lds) hipLaunchKernelGGL(slide_argmax_topk_lds_kernel<S>, grid, dim3(256), col, stream, logits, C, hs, ws, classes, probs, H, W, hc, wc, rh, rw, wt, \
                                uncovered, K, plane, inv_temperature);                                                                                    \
    else hipLaunchKernelGGL(slide_argmax_topk_kernel<S>, grid, dim3(256), 0, stream, logits, C, hs, ws, classes, probs, H, W, hc, wc, rh, rw, wt,         \
                            uncovered, K, plane, inv_temperature);                                                                                        \
  } while (0)
  TOPK_DISPATCH(K, TOPK_LAUNCH);
#undef TOPK_LAUNCH
  MMSA_CHECK_LAUNCH(name);
  return MMSA_OK;
}
