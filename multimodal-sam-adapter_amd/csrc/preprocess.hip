// Input side of the segmentor on device: what the reference's test pipelines do on the host between the loader and the network
// (segmentation/mmseg_custom/datasets/pipelines/transform.py):
//   Pad_multimodal (2934-3010: impad bottom / right with pad_val)  ->  Normalize_multimodal / Normalize_multimodal_Muses (2601-2825:
//   per modality `img / 255` when norm_by_max, then mmcv.imnormalize = BGR->RGB channel reversal when to_rgb, cv2.subtract(mean),
//   cv2.multiply(1 / float64(std)))  ->  ImageToTensor (HWC -> CHW)  ->  Collectmod,
// and, for slide inference, the crop of encoder_decoder.py:205-212 on top of it -- as ONE pass from the loaders' HWC frames (uint8 or
// float32, one tensor [B, Hs, Ws, 3] per modality) to float32 NCHW, whole ([B, 6, H, W]) or as the windows of a frame ([n, 6, hc, wc]).
// HBM-bound: a transpose from interleaved 3-channel pixels to planes.  A lane owns 4 consecutive pixels of an output row: 12 source bytes
// (three dwords) or 48 (three float4) per modality in, one float4 per plane out; a workgroup covers 1024 pixels of one row, so both sides
// are whole lines.  Four pixels that lie wholly in the padding are written the same way without a load.  Lanes whose 4 pixels straddle the
// source's right edge, rows / windows whose start is not 16-byte (float32) / 4-byte (uint8) aligned in the source or not 16-byte aligned in the
// output, and the last lanes of a width that is no multiple of 4 take the edge path, pixel by pixel.
#include "common.h"

// The arithmetic is the reference's float32 sequence with one rounding per step: a = x / 255.0f (a true, correctly rounded division: the build
// uses no fast-math), a - mean, * sinv.  A subtraction followed by a multiplication has no fused form; contraction is switched off all the same.
#pragma clang fp contract(off)

#define MMSA_MAX_WINDOWS 64
struct WindowTable { int n; int b[MMSA_MAX_WINDOWS], y0[MMSA_MAX_WINDOWS], x0[MMSA_MAX_WINDOWS]; };   // as in segment.hip
struct NoWindows {};

struct PreParams {
  float mean[6], sinv[6];      // per OUTPUT channel
  float pad_val[2];            // per modality: the value of a pixel outside the source, BEFORE normalisation
  int div255[2], swap[2];      // per modality: norm_by_max division; to_rgb = the modality's three channels reversed
};

__device__ __forceinline__ float pre_norm(float x, float mean, float sinv, int div255) {
  const float a = div255 ? x / 255.0f : x;
  return (a - mean) * sinv;
}

__device__ __forceinline__ void pre_load4(const unsigned char* sp, float (&v)[4][3]) {
  const uint32_t* w = (const uint32_t*)sp;
  const uint32_t w0 = w[0], w1 = w[1], w2 = w[2];
  v[0][0] = (float)(w0 & 255u); v[0][1] = (float)((w0 >> 8) & 255u); v[0][2] = (float)((w0 >> 16) & 255u);
  v[1][0] = (float)(w0 >> 24);  v[1][1] = (float)(w1 & 255u);        v[1][2] = (float)((w1 >> 8) & 255u);
  v[2][0] = (float)((w1 >> 16) & 255u); v[2][1] = (float)(w1 >> 24); v[2][2] = (float)(w2 & 255u);
  v[3][0] = (float)((w2 >> 8) & 255u);  v[3][1] = (float)((w2 >> 16) & 255u); v[3][2] = (float)(w2 >> 24);
}

__device__ __forceinline__ void pre_load4(const float* sp, float (&v)[4][3]) {
  const float4* w = (const float4*)sp;
  const float4 a = w[0], b = w[1], c = w[2];
  v[0][0] = a.x; v[0][1] = a.y; v[0][2] = a.z;
  v[1][0] = a.w; v[1][1] = b.x; v[1][2] = b.y;
  v[2][0] = b.z; v[2][1] = b.w; v[2][2] = c.x;
  v[3][0] = c.y; v[3][1] = c.z; v[3][2] = c.w;
}

// One modality (M = 0, 1) of up to 4 consecutive output pixels: source pixels (b, y, x .. x+3), output planes 3M .. 3M+2 at d.
template <int M, typename T>
__device__ __forceinline__ void pre_modality(const T* __restrict__ src, int b, int y, int x, int Hs, int Ws, const PreParams& p,
                                             float* __restrict__ d, long plane, int nvalid) {
  const bool inrow = y < Hs;
  const T* sp = src + (((long)b * Hs + y) * Ws + x) * 3;
  constexpr uintptr_t amask = sizeof(T) == 1 ? 3 : 15;
  const int sw = p.swap[M], dv = p.div255[M];
  const float pad = p.pad_val[M];
  const bool vec_dst = nvalid >= 4 && (((uintptr_t)d | (uintptr_t)(plane * 4)) & 15) == 0;
  const bool allpad = !inrow || x >= Ws;                                   // nothing outside the [B, Hs, Ws, 3] source is ever read
  const bool vec_src = inrow && x + 3 < Ws && ((uintptr_t)sp & amask) == 0;
  if (vec_dst && (allpad || vec_src)) {
    float v[4][3];
    if (allpad) {
#pragma unroll
      for (int q = 0; q < 4; ++q) v[q][0] = v[q][1] = v[q][2] = pad;
    } else {
      pre_load4(sp, v);
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      float o[4];
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const float xin = c == 1 ? v[q][1] : (c == 0 ? (sw ? v[q][2] : v[q][0]) : (sw ? v[q][0] : v[q][2]));
        o[q] = pre_norm(xin, p.mean[3 * M + c], p.sinv[3 * M + c], dv);
      }
      *(float4*)(d + (3 * M + c) * plane) = make_float4(o[0], o[1], o[2], o[3]);
    }
  } else {                                                                 // edge path: pixel by pixel
#pragma unroll 1
    for (int q = 0; q < nvalid && q < 4; ++q) {
      float r0 = pad, r1 = pad, r2 = pad;
      if (inrow && x + q < Ws) { r0 = (float)sp[3 * q]; r1 = (float)sp[3 * q + 1]; r2 = (float)sp[3 * q + 2]; }
      d[(3 * M + 0) * plane + q] = pre_norm(sw ? r2 : r0, p.mean[3 * M + 0], p.sinv[3 * M + 0], dv);
      d[(3 * M + 1) * plane + q] = pre_norm(r1, p.mean[3 * M + 1], p.sinv[3 * M + 1], dv);
      d[(3 * M + 2) * plane + q] = pre_norm(sw ? r0 : r2, p.mean[3 * M + 2], p.sinv[3 * M + 2], dv);
    }
  }
}

// grid (cdiv(wc, 1024), hc, n): output row i of window / image k.  WT = WindowTable: window k = (image, y0, x0) of the padded canvas;
// WT = NoWindows: image k at (0, 0), hc x wc = the canvas.
template <typename T0, typename T1, typename WT>
__global__ __launch_bounds__(256) void preprocess_kernel(const T0* __restrict__ src0, const T1* __restrict__ src1, int Hs, int Ws,
                                                         float* __restrict__ dst, int hc, int wc, PreParams p, WT wt) {
  const int j = (blockIdx.x * 256 + threadIdx.x) * 4;
  if (j >= wc) return;
  const int i = blockIdx.y, k = blockIdx.z;
  int b = k, y = i, x = j;
  if constexpr (sizeof(WT) > 1) { b = wt.b[k]; y += wt.y0[k]; x += wt.x0[k]; }
  const long plane = (long)hc * wc;
  float* d = dst + (long)k * 6 * plane + (long)i * wc + j;
  pre_modality<0>(src0, b, y, x, Hs, Ws, p, d, plane, wc - j);
  pre_modality<1>(src1, b, y, x, Hs, Ws, p, d, plane, wc - j);
}

template <typename WT>
static void pre_launch(const void* s0, int t0, const void* s1, int t1, int Hs, int Ws, float* dst, int hc, int wc, int n, const PreParams& p,
                       const WT& wt, hipStream_t stream) {
  const dim3 grid(cdiv(wc, 1024), hc, n), block(256);
  typedef unsigned char u8;
  if (t0 == MMSA_PRE_U8 && t1 == MMSA_PRE_U8)
    hipLaunchKernelGGL((preprocess_kernel<u8, u8, WT>), grid, block, 0, stream, (const u8*)s0, (const u8*)s1, Hs, Ws, dst, hc, wc, p, wt);
  else if (t0 == MMSA_PRE_U8)
    hipLaunchKernelGGL((preprocess_kernel<u8, float, WT>), grid, block, 0, stream, (const u8*)s0, (const float*)s1, Hs, Ws, dst, hc, wc, p, wt);
  else if (t1 == MMSA_PRE_U8)
    hipLaunchKernelGGL((preprocess_kernel<float, u8, WT>), grid, block, 0, stream, (const float*)s0, (const u8*)s1, Hs, Ws, dst, hc, wc, p, wt);
  else
    hipLaunchKernelGGL((preprocess_kernel<float, float, WT>), grid, block, 0, stream, (const float*)s0, (const float*)s1, Hs, Ws, dst, hc, wc, p, wt);
}

static int pre_params(PreParams& p, const void* src0, int dtype0, const void* src1, int dtype1, int B, int Hs, int Ws, const float* mean,
                      const float* sinv, const int* div255, const int* swap, const float* pad_val, const float* dst, int H, int W, const char* name) {
  MMSA_CHECK_ARG(src0 && src1 && dst && mean && sinv && div255 && swap && pad_val, "%s: null argument", name);
  MMSA_CHECK_ARG((dtype0 == MMSA_PRE_U8 || dtype0 == MMSA_PRE_F32) && (dtype1 == MMSA_PRE_U8 || dtype1 == MMSA_PRE_F32),
                 "%s: source dtypes (%d, %d) must be MMSA_PRE_U8 or MMSA_PRE_F32", name, dtype0, dtype1);
  MMSA_CHECK_ARG(B > 0 && B <= 65535 && Hs > 0 && Ws > 0, "%s: bad source shape [%d, %d, %d, 3]", name, B, Hs, Ws);
  MMSA_CHECK_ARG(H >= Hs && W >= Ws, "%s: the %d x %d canvas is smaller than the %d x %d source (padding only grows a frame)", name, H, W, Hs, Ws);
  for (int c = 0; c < 6; ++c) {
    MMSA_CHECK_ARG(mean[c] == mean[c] && sinv[c] - sinv[c] == 0.f && sinv[c] != 0.f, "%s: mean / sinv of channel %d is not a finite, non-zero scale", name, c);
    p.mean[c] = mean[c];
    p.sinv[c] = sinv[c];
  }
  for (int m = 0; m < 2; ++m) { p.pad_val[m] = pad_val[m]; p.div255[m] = div255[m] != 0; p.swap[m] = swap[m] != 0; }
  return MMSA_OK;
}

extern "C" int mmsa_preprocess_nhwc(const void* src0, int dtype0, const void* src1, int dtype1, int B, int Hs, int Ws, const float* mean,
                                    const float* sinv, const int* div255, const int* swap, const float* pad_val, float* dst, int H, int W,
                                    hipStream_t stream) {
  PreParams p;
  int rc = pre_params(p, src0, dtype0, src1, dtype1, B, Hs, Ws, mean, sinv, div255, swap, pad_val, dst, H, W, "preprocess_nhwc");
  if (rc) return rc;
  MMSA_CHECK_ARG(H <= 65535, "preprocess_nhwc: H too large for the launch grid");
  pre_launch(src0, dtype0, src1, dtype1, Hs, Ws, dst, H, W, B, p, NoWindows(), stream);
  MMSA_CHECK_LAUNCH("preprocess_nhwc");
  return MMSA_OK;
}

extern "C" int mmsa_preprocess_crops(const void* src0, int dtype0, const void* src1, int dtype1, int B, int Hs, int Ws, const float* mean,
                                     const float* sinv, const int* div255, const int* swap, const float* pad_val, int H, int W,
                                     const int* windows /* HOST [n,3]: image, y0, x0 */, int n, float* dst, int hc, int wc, hipStream_t stream) {
  PreParams p;
  int rc = pre_params(p, src0, dtype0, src1, dtype1, B, Hs, Ws, mean, sinv, div255, swap, pad_val, dst, H, W, "preprocess_crops");
  if (rc) return rc;
  MMSA_CHECK_ARG(hc > 0 && wc > 0 && hc <= 65535, "preprocess_crops: bad crop size %d x %d", hc, wc);
  MMSA_CHECK_ARG(windows && n > 0 && n <= MMSA_MAX_WINDOWS, "preprocess_crops: 1..%d windows per call", MMSA_MAX_WINDOWS);
  WindowTable wt;
  wt.n = n;
  for (int k = 0; k < n; ++k) {      // checked against the PADDED canvas: a window may reach into the padding, never beyond it
    wt.b[k] = windows[3 * k]; wt.y0[k] = windows[3 * k + 1]; wt.x0[k] = windows[3 * k + 2];
    MMSA_CHECK_ARG(wt.b[k] >= 0 && wt.b[k] < B && wt.y0[k] >= 0 && wt.x0[k] >= 0 && wt.y0[k] + hc <= H && wt.x0[k] + wc <= W,
                   "preprocess_crops: window %d (image %d, y0 %d, x0 %d, %dx%d) outside the [%d, %d, %d] canvas", k, wt.b[k], wt.y0[k], wt.x0[k], hc, wc, B, H, W);
  }
  pre_launch(src0, dtype0, src1, dtype1, Hs, Ws, dst, hc, wc, n, p, wt, stream);
  MMSA_CHECK_LAUNCH("preprocess_crops");
  return MMSA_OK;
}
