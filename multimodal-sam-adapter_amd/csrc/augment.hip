// Test-time augmentation on device: EncoderDecoder.aug_test (segmentation/mmseg_custom/models/segmentors/encoder_decoder.py:509-546) after the head --
//   softmax_flip_accum_nchw : F.softmax(seg_logit, dim=1), flipped back when the view was flipped (ED:448-469), written or ADDED to the frame's
//                             probabilities (seg_logit += cur_seg_logit, ED:540) and divided by the number of views with the last one (ED:541): the canvas path;
//   aug_argmax              : all of that for every view, from the views' head-resolution logits, plus the argmax (ED:542), in ONE launch that writes
//                             only the uint8 class map.
#include "common.h"

// No fused multiply-add contraction in this file, for the reason given at the top of segment.hip: the one-pass kernel restates the interpolation of the
// canvas path (bilinear_accum + div_count + bilinear_accum) and must round it identically; the same holds for the softmax of the two kernels here.
#pragma clang fp contract(off)
#include "slide_taps.h"
#include "softmax_px.h"

// One lane per pixel of logits [B, C, H, W]: p = softmax over C, written (accumulate = 0) or added to acc [B, C, H, W] at the pixel's mirror image
// (flip 1: horizontal, x' = W - 1 - x; 2: vertical, y' = H - 1 - y); finish_div > 0: the stored value is divided by it.  The exponentials are evaluated
// twice (once for the sum, once for p) instead of being kept: the same instructions on the same inputs, the same bits.
// TEMP: the softmax of x / T -- every exponential is softmax_px_exp_t with the inverse temperature `it` (softmax_flip_accum_t_kernel, at the end of the file).
template <bool TEMP>
__device__ __forceinline__ void softmax_flip_accum_pixel(const float* __restrict__ logits, float* __restrict__ acc, int C, int H, int W, int flip, int accumulate,
                                                         int finish_div, float it) {
  const int x = blockIdx.x * 256 + threadIdx.x, y = blockIdx.y, b = blockIdx.z;
  if (x >= W) return;
  const long HW = (long)H * W;
  const float* xp = logits + (long)b * C * HW + (long)y * W + x;
  float* ap = acc + (long)b * C * HW + (long)(flip == 2 ? H - 1 - y : y) * W + (flip == 1 ? W - 1 - x : x);
  float m = xp[0];
  for (int c = 1; c < C; ++c) m = softmax_px_max(m, xp[c * HW]);
  float s = 0.f;
  for (int c = 0; c < C; ++c) s = softmax_px_sum(s, TEMP ? softmax_px_exp_t(xp[c * HW], m, it) : softmax_px_exp(xp[c * HW], m), c == 0);
  for (int c = 0; c < C; ++c) {
    const float p = softmax_px_prob(TEMP ? softmax_px_exp_t(xp[c * HW], m, it) : softmax_px_exp(xp[c * HW], m), s);
    float v = softmax_px_accum(accumulate ? ap[c * HW] : 0.f, p, !accumulate);
    if (finish_div > 0) v = softmax_px_mean(v, finish_div);
    ap[c * HW] = v;
  }
}

__global__ __launch_bounds__(256) void softmax_flip_accum_kernel(const float* __restrict__ logits, float* __restrict__ acc, int C, int H, int W, int flip,
                                                                 int accumulate, int finish_div) {
  softmax_flip_accum_pixel<false>(logits, acc, C, H, W, flip, accumulate, finish_div, 1.f);
}

__global__ void softmax_flip_accum_t_kernel(const float* __restrict__ logits, float* __restrict__ acc, int C, int H, int W, int flip, int accumulate, int finish_div,
                                            float it);      // at the end of the file, below the kernels that were here before it (profiles/temperature_isa.txt)

// the checks and the launch of mmsa_softmax_flip_accum_nchw and mmsa_softmax_flip_accum_nchw_t (`it` given)
static int softmax_flip_accum_launch(const char* name, const float* logits, float* acc, int B, int C, int H, int W, int flip, int accumulate, int finish_div,
                                     hipStream_t stream, const float* it = nullptr) {
  MMSA_CHECK_ARG(logits && acc && logits != acc && B > 0 && C > 0 && H > 0 && W > 0 && H <= 65535 && B <= 65535, "%s: bad args", name);
  MMSA_CHECK_ARG(flip >= 0 && flip <= 2 && finish_div >= 0, "%s: flip is 0 (none), 1 (horizontal) or 2 (vertical), finish_div >= 0", name);
  if (it) MMSA_CHECK_INV_TEMPERATURE(name, *it);
  if (it)
    hipLaunchKernelGGL(softmax_flip_accum_t_kernel, dim3(cdiv(W, 256), H, B), dim3(256), 0, stream, logits, acc, C, H, W, flip, accumulate, finish_div, *it);
  else hipLaunchKernelGGL(softmax_flip_accum_kernel, dim3(cdiv(W, 256), H, B), dim3(256), 0, stream, logits, acc, C, H, W, flip, accumulate, finish_div);
  MMSA_CHECK_LAUNCH(name);
  return MMSA_OK;
}

extern "C" int mmsa_softmax_flip_accum_nchw(const float* logits, float* acc, int B, int C, int H, int W, int flip, int accumulate, int finish_div,
                                            hipStream_t stream) {
  return softmax_flip_accum_launch("softmax_flip_accum_nchw", logits, acc, B, C, H, W, flip, accumulate, finish_div, stream);
}

extern "C" int mmsa_softmax_flip_accum_nchw_t(const float* logits, float* acc, int B, int C, int H, int W, int flip, int accumulate, int finish_div,
                                              float inv_temperature, hipStream_t stream) {
  return softmax_flip_accum_launch("softmax_flip_accum_nchw_t", logits, acc, B, C, H, W, flip, accumulate, finish_div, stream, &inv_temperature);
}

// ---- the class map of an augmented frame in ONE pass.  A view is what mmsa_slide_argmax_resized takes for one frame: head-resolution logits
// [n, C, hs, ws] of n windows (hc x wc) on an H x W canvas, resized to Hd x Wd; all views share the cut [B, Ho, Wo].  The descriptors travel by value in the
// launch arguments (64 bytes each); the window tables of all views are one device int [total, 3] array (12 views x 64 windows x 12 bytes do not fit the
// argument block), view a's rows being w0 .. w0 + n - 1.
#define MMSA_MAX_AUGS 12
struct AugView { const float* logits; int w0, n, hs, ws, H, W, hc, wc, flip; float rh, rw, rh2, rw2; };
struct AugViews { int A; AugView v[MMSA_MAX_AUGS]; };

// The logits of view `v` at position (Y, X) of its Hd x Wd map -> xs[c * T], c = 0 .. C-1: the two-stage pixel of slide_taps.h, as slide_argmax_resized_kernel
// (segment.hip) takes it, with the argmax taken out.  false: a tap has no window, or more than 8.  The view's fields are copied to locals first, as this
// function always did: handing v.* straight to the two functions is the same arithmetic in another instruction stream, and aug_argmax_conf_kernel measured
// 75 us (1 %) slower that way (profiles/class_map_pixel_refactor.txt).
__device__ __forceinline__ bool aug_view_logits(const AugView& v, const int* __restrict__ windows, int C, int b, int Y, int X, float* xs, int T) {
  const float* __restrict__ logits = v.logits;
  const DevWindows wt = {windows + 3 * (long)v.w0, v.n};
  const int hs = v.hs, ws = v.ws, H = v.H, W = v.W, hc = v.hc, wc = v.wc;
  const float rh = v.rh, rw = v.rw;
  TwoStagePixel px;
  two_stage_setup(px, wt, b, Y, X, H, W, hc, wc, hs, ws, rh, rw, v.rh2, v.rw2);
  if (px.nmin == 0 || px.nmax > 8) return false;
  if (px.nmax <= RESIZED_SLOTS) {
    for (int c = 0; c < C; ++c) xs[c * T] = two_stage_value<false>(px, wt, b, logits, C, c, hs, ws, hc, wc, rh, rw);
  } else {
    for (int c = 0; c < C; ++c) xs[c * T] = two_stage_value<true>(px, wt, b, logits, C, c, hs, ws, hc, wc, rh, rw);
  }
  return true;
}

// One lane owns one output pixel and two columns of C floats in LDS, laid out [c][lane] (consecutive lanes, consecutive banks): this view's logits,
// overwritten by their exponentials, and the probabilities summed over the views so far.  The columns are private to the lane: no barrier anywhere.
// T = blockDim.x = 256 / 128 / 64 lanes for C <= 32 / 64 / 128 keeps the 2 C T floats within 64 KiB.
// CONF: `best`, the mean probability of the predicted class, also goes to conf float [B, Ho, Wo] (0 for a 255 pixel).
template <bool CONF>
__device__ __forceinline__ void aug_pixel(const AugViews& av, int C, const int* __restrict__ windows, unsigned char* __restrict__ out, float* __restrict__ conf,
                                          int Ho, int Wo, int* __restrict__ uncovered) {
  extern __shared__ float aug_lds[];
  const int T = blockDim.x;
  const int X = blockIdx.x * T + threadIdx.x, Y = blockIdx.y, b = blockIdx.z;
  if (X >= Wo) return;
  float* xs = aug_lds + threadIdx.x;
  float* acc = aug_lds + C * T + threadIdx.x;
  const long op = ((long)b * Ho + Y) * Wo + X;
  for (int a = 0; a < av.A; ++a) {
    const AugView& v = av.v[a];
    // the view's probabilities are flipped back (ED:448-469): output pixel (Y, X) takes them from its mirror image in the view's map
    if (!aug_view_logits(v, windows, C, b, v.flip == 2 ? Ho - 1 - Y : Y, v.flip == 1 ? Wo - 1 - X : X, xs, T)) {
      atomicAdd(uncovered, 1);      // a tap without a window, or with more than 8, in ANY view: counted once per output pixel, and the pixel gets 255
      out[op] = 255;
      if constexpr (CONF) conf[op] = 0.f;
      return;
    }
    float m = xs[0];
    for (int c = 1; c < C; ++c) m = softmax_px_max(m, xs[c * T]);
    float s = 0.f;
    for (int c = 0; c < C; ++c) {
      const float e = softmax_px_exp(xs[c * T], m);
      xs[c * T] = e;
      s = softmax_px_sum(s, e, c == 0);
    }
    for (int c = 0; c < C; ++c) acc[c * T] = softmax_px_accum(a == 0 ? 0.f : acc[c * T], softmax_px_prob(xs[c * T], s), a == 0);
  }
  float best = -INFINITY;
  int bi = 0;
  for (int c = 0; c < C; ++c) {
    const float p = softmax_px_mean(acc[c * T], av.A);
    if (c == 0 || p > best) { best = p; bi = c; }      // first maximum wins, like torch.argmax on ties
  }
  out[op] = (unsigned char)bi;
  if constexpr (CONF) conf[op] = best;      // max_c of the mean probabilities: what the argmax above compared
}

__global__ __launch_bounds__(256) void aug_argmax_kernel(AugViews av, int C, const int* __restrict__ windows, unsigned char* __restrict__ out, int Ho, int Wo,
                                                         int* __restrict__ uncovered) {
  aug_pixel<false>(av, C, windows, out, nullptr, Ho, Wo, uncovered);
}

// aug_argmax_kernel + the confidence map of the augmented frame: conf = max_c mean_a P_a[c] (ED:449,460 + ED:538-541).
__global__ __launch_bounds__(256) void aug_argmax_conf_kernel(AugViews av, int C, const int* __restrict__ windows, unsigned char* __restrict__ out,
                                                              float* __restrict__ conf, int Ho, int Wo, int* __restrict__ uncovered) {
  aug_pixel<true>(av, C, windows, out, conf, Ho, Wo, uncovered);
}

#define AUG_VIEW_INTS 11      // one row of `views`: w0, n, hs, ws, H, W, hc, wc, Hd, Wd, flip

// the checks and the launch of both entries; `conf` given: aug_argmax_conf_kernel
static int aug_argmax_launch(const char* name, const float* const* logits, const int* views, int A, int C, const int* windows, const int* windows_host, int total,
                             unsigned char* out, float* conf, int B, int Ho, int Wo, int* uncovered, hipStream_t stream) {
  MMSA_CHECK_ARG(A >= 1 && A <= MMSA_MAX_AUGS, "%s: %d views, 1..%d per call", name, A, MMSA_MAX_AUGS);
  MMSA_CHECK_ARG(C >= 1 && C <= 128, "%s: %d classes; the per-pixel columns of more than 128 do not fit 64 KiB of LDS (use the canvas path: "
                 "mmsa_softmax_flip_accum_nchw per view + mmsa_argmax_nchw)", name, C);
  MMSA_CHECK_ARG(logits && views && windows && windows_host && out && uncovered && total > 0 && B > 0 && Ho > 0 && Wo > 0 && Ho <= 65535 && B <= 65535,
                 "%s: bad args", name);
  AugViews av;
  av.A = A;
  for (int a = 0; a < A; ++a) {
    const int* r = views + AUG_VIEW_INTS * a;
    AugView& v = av.v[a];
    v.logits = logits[a];
    v.w0 = r[0]; v.n = r[1]; v.hs = r[2]; v.ws = r[3]; v.H = r[4]; v.W = r[5]; v.hc = r[6]; v.wc = r[7]; v.flip = r[10];
    const int Hd = r[8], Wd = r[9];
    MMSA_CHECK_ARG(v.logits && v.hs > 0 && v.ws > 0 && v.H > 0 && v.W > 0 && v.hc > 0 && v.wc > 0 && v.flip >= 0 && v.flip <= 2,
                   "%s: view %d: bad sizes or flip (0 none, 1 horizontal, 2 vertical)", name, a);
    MMSA_CHECK_ARG(Hd > 0 && Wd > 0 && Ho <= Hd && Wo <= Wd, "%s: view %d: the cut %dx%d must lie inside the target %dx%d", name, a, Ho, Wo, Hd, Wd);
    MMSA_CHECK_ARG(v.n > 0 && v.n <= MMSA_MAX_WINDOWS && v.w0 >= 0 && (long)v.w0 + v.n <= total, "%s: view %d: 1..%d windows per view, inside the table of %d rows",
                   name, a, MMSA_MAX_WINDOWS, total);
    for (int k = 0; k < v.n; ++k) {
      const int* w = windows_host + 3 * (long)(v.w0 + k);
      if (int rc = check_window(name, a, k, w[0], w[1], w[2], v.hc, v.wc, B, v.H, v.W)) return rc;
    }
    v.rh = (float)v.hs / (float)v.hc; v.rw = (float)v.ws / (float)v.wc;
    v.rh2 = (float)v.H / (float)Hd; v.rw2 = (float)v.W / (float)Wd;
  }
  const int T = C <= 32 ? 256 : C <= 64 ? 128 : 64;
  const size_t lds = (size_t)2 * C * T * sizeof(float);
  if (conf) hipLaunchKernelGGL(aug_argmax_conf_kernel, dim3(cdiv(Wo, T), Ho, B), dim3(T), lds, stream, av, C, windows, out, conf, Ho, Wo, uncovered);
  else hipLaunchKernelGGL(aug_argmax_kernel, dim3(cdiv(Wo, T), Ho, B), dim3(T), lds, stream, av, C, windows, out, Ho, Wo, uncovered);
  MMSA_CHECK_LAUNCH(name);
  return MMSA_OK;
}

extern "C" int mmsa_aug_argmax(const float* const* logits /* HOST [A] device pointers */, const int* views /* HOST [A, 11] */, int A, int C,
                               const int* windows /* DEVICE [total, 3] */, const int* windows_host /* HOST copy of it */, int total, unsigned char* out,
                               int B, int Ho, int Wo, int* uncovered /* device int, zeroed by the caller */, hipStream_t stream) {
  return aug_argmax_launch("aug_argmax", logits, views, A, C, windows, windows_host, total, out, nullptr, B, Ho, Wo, uncovered, stream);
}

extern "C" int mmsa_aug_argmax_conf(const float* const* logits /* HOST [A] device pointers */, const int* views /* HOST [A, 11] */, int A, int C,
                                    const int* windows /* DEVICE [total, 3] */, const int* windows_host /* HOST copy of it */, int total, unsigned char* out,
                                    float* conf, int B, int Ho, int Wo, int* uncovered /* device int, zeroed by the caller */, hipStream_t stream) {
  MMSA_CHECK_ARG(conf, "aug_argmax_conf: bad args (conf is NULL)");
  return aug_argmax_launch("aug_argmax_conf", logits, views, A, C, windows, windows_host, total, out, conf, B, Ho, Wo, uncovered, stream);
}

// ---- the canvas softmax of x / T: softmax_flip_accum_kernel with softmax_px_exp_t (csrc/softmax_px.h), for `probabilities(..., temperature=)` and the canvas
// path of a tempered confidence map.  At it == 1.0f it is that kernel bit for bit.
__global__ __launch_bounds__(256) void softmax_flip_accum_t_kernel(const float* __restrict__ logits, float* __restrict__ acc, int C, int H, int W, int flip,
                                                                   int accumulate, int finish_div, float it) {
  softmax_flip_accum_pixel<true>(logits, acc, C, H, W, flip, accumulate, finish_div, it);
}
