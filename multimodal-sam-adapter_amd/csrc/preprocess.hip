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
//
// The resizing form (Resize_multimodal first: transform.py:1136-1167, mmcv.imrescale / imresize = cv2.resize INTER_LINEAR per modality) produces
// the same outputs from sources of another size: canvas pixel (y, x) inside the Hr x Wr resized frame is the bilinear value of source rows
// ys[y], ys[y] + 1 and columns xs[x], xs[x] + 1 with the coefficient pairs of the per-axis device tables (built on the host, mmsa/preprocess.py).
// Same ownership (a lane = 4 pixels of an output row, planes out as float4).  The workgroup's 1024 output pixels read one contiguous span of two
// source rows per modality; the span is staged through LDS with coalesced dword loads (interleaved 3-byte pixels make a lane's own taps
// unaligned) and the taps are read from there -- consecutive lanes are about 3 dwords apart, an odd stride over the banks.  A span that does not
// fit the staging buffer (strong downscaling) takes the same arithmetic with the taps read from global memory.  The resized frame is never written.
#include <type_traits>

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

// ---- the resizing form ----
// uint8 + uint8 sources (FX): OpenCV's 8-bit fixed-point bilinear, coefficients int16 pairs scaled by 2048:
//   horizontal D = S[s] * a0 + S[s+1] * a1 (int32); vertical (((b0 * (D0 >> 4)) >> 16) + ((b1 * (D1 >> 4)) >> 16) + 2) >> 2; the result is a byte.
// otherwise: float32, D = S[s] * a0 + S[s+1] * a1, D0 * b0 + D1 * b1, every product and sum rounded once (contraction is off in this file);
// a uint8 source is converted exactly first (the loaders' concatenated array is float32 as soon as one modality is).
template <bool FX> struct ResizeTables {
  typedef typename std::conditional<FX, short2, float2>::type Coef;
  int Hr, Wr;                                 // the resized frame inside the H x W canvas
  const int* xs; const Coef* xc;              // [Wr] first tap (the second is xs + 1, clamped), [Wr] coefficient pair
  const int* ys; const Coef* yc;              // [Hr] likewise
  int cap;                                    // source pixels per staged row that the LDS buffer holds; 0 = no staging
};
struct NoResize {};
template <typename RS> struct pre_is_fixed { static constexpr bool value = false; };
template <> struct pre_is_fixed<ResizeTables<true>> { static constexpr bool value = true; };

// dwords of one staged row of `cap` pixels: the row starts at the dword that holds its first byte (up to 3 bytes before it)
__host__ __device__ constexpr int pre_stage_dwords(int elem_bytes, int cap) { return (cap * 3 * elem_bytes + 3) / 4 + 1; }

// Elements [first, first + nelem) of src -> lds, as whole dwords from the dword that holds the first byte.  Nothing outside src's `total`
// elements is read: a last dword that would cross the end of the array is assembled from bytes.  src is 4-byte aligned (checked by the host).
template <typename T>
__device__ __forceinline__ void pre_stage(const T* __restrict__ src, long total, long first, int nelem, uint32_t* lds) {
  const unsigned char* g = (const unsigned char*)src;
  const long byte0 = first * (long)sizeof(T), a0 = byte0 & ~3L, end = byte0 + (long)nelem * (long)sizeof(T), tot = total * (long)sizeof(T);
  const int ndw = (int)((end - a0 + 3) >> 2);
  for (int w = threadIdx.x; w < ndw; w += 256) {
    const long off = a0 + 4L * w;
    uint32_t v = 0;
    if (off + 4 <= tot) v = *(const uint32_t*)(g + off);
    else for (int t = 0; off + t < tot; ++t) v |= (uint32_t)g[off + t] << (8 * t);
    lds[w] = v;
  }
}

// One modality of up to 4 consecutive output pixels of the resizing form.  r0 / r1: the two source rows, element (x, c) at [(x - xoff) * 3 + c]
// (global memory with xoff = 0, or the staged span that starts at source column xoff).  in[q]: pixel q lies inside the resized frame.
template <int M, bool FX, typename T, typename Coef>
__device__ __forceinline__ void pre_resize_modality(const T* r0, const T* r1, int xoff, const int (&s0)[4], const int (&s1)[4], const Coef (&a)[4], Coef bq,
                                                    const bool (&in)[4], const PreParams& p, float* __restrict__ d, long plane, int nvalid) {
  const int sw = p.swap[M], dv = p.div255[M];
  const float pad = p.pad_val[M];
  float v[4][3];
#pragma unroll
  for (int q = 0; q < 4; ++q) {
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      float val = pad;
      if (in[q]) {
        const int e0 = (s0[q] - xoff) * 3 + c, e1 = (s1[q] - xoff) * 3 + c;
        if constexpr (FX) {
          const int D0 = (int)r0[e0] * a[q].x + (int)r0[e1] * a[q].y;
          const int D1 = (int)r1[e0] * a[q].x + (int)r1[e1] * a[q].y;
          val = (float)((((bq.x * (D0 >> 4)) >> 16) + ((bq.y * (D1 >> 4)) >> 16) + 2) >> 2);
        } else {
          const float D0 = (float)r0[e0] * a[q].x + (float)r0[e1] * a[q].y;
          const float D1 = (float)r1[e0] * a[q].x + (float)r1[e1] * a[q].y;
          val = D0 * bq.x + D1 * bq.y;
        }
      }
      v[q][c] = val;
    }
  }
  const bool vec_dst = nvalid >= 4 && (((uintptr_t)d | (uintptr_t)(plane * 4)) & 15) == 0;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    float o[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const float xin = c == 1 ? v[q][1] : (c == 0 ? (sw ? v[q][2] : v[q][0]) : (sw ? v[q][0] : v[q][2]));
      o[q] = pre_norm(xin, p.mean[3 * M + c], p.sinv[3 * M + c], dv);
    }
    float* dc = d + (3 * M + c) * plane;
    if (vec_dst) {
      *(float4*)dc = make_float4(o[0], o[1], o[2], o[3]);
    } else {                                                               // edge path: pixel by pixel
#pragma unroll
      for (int q = 0; q < 4; ++q)
        if (q < nvalid) dc[q] = o[q];
    }
  }
}

template <typename T0, typename T1, typename WT, bool FX>
__device__ __forceinline__ void pre_resize_block(const T0* __restrict__ src0, const T1* __restrict__ src1, int B, int Hs, int Ws, float* __restrict__ dst,
                                                 int hc, int wc, const PreParams& p, const WT& wt, const ResizeTables<FX>& rs) {
  typedef typename ResizeTables<FX>::Coef Coef;
  extern __shared__ uint32_t pre_lds[];
  const int i = blockIdx.y, k = blockIdx.z, jb = blockIdx.x * 1024;
  int b = k, y = i, xw = 0;
  if constexpr (sizeof(WT) > 1) { b = wt.b[k]; y += wt.y0[k]; xw = wt.x0[k]; }
  const int xb = xw + jb;                                                  // canvas columns [xb, xe) belong to this workgroup
  const int xe = min(xb + 1024, xw + wc), xer = min(xe, rs.Wr);
  const bool any = y < rs.Hr && xb < rs.Wr;                                // workgroup-uniform: otherwise all padding, nothing is loaded
  int sy0 = 0, sy1 = 0, lo = 0, hi = Ws - 1;
  Coef bq = Coef();
  bool staged = false;
  if (any) {
    sy0 = min(max(rs.ys[y], 0), Hs - 1);                                   // taps are clamped here: whatever the tables hold, none leaves the source
    sy1 = min(sy0 + 1, Hs - 1);
    bq = rs.yc[y];
    const int x_lo = min(max(rs.xs[xb], 0), Ws - 1), x_hi = min(max(rs.xs[xer - 1], x_lo) + 1, Ws - 1);
    staged = x_hi - x_lo + 1 <= rs.cap;
    if (staged) { lo = x_lo; hi = x_hi; }
  }
  const long row0 = ((long)b * Hs + sy0) * Ws * 3, row1 = ((long)b * Hs + sy1) * Ws * 3, total = (long)B * Hs * Ws * 3;
  const int dw0 = pre_stage_dwords(sizeof(T0), rs.cap), dw1 = pre_stage_dwords(sizeof(T1), rs.cap);
  if (staged) {                                                            // workgroup-uniform, and so is the barrier
    const int ne = (hi - lo + 1) * 3;
    pre_stage(src0, total, row0 + (long)lo * 3, ne, pre_lds);
    pre_stage(src0, total, row1 + (long)lo * 3, ne, pre_lds + dw0);
    pre_stage(src1, total, row0 + (long)lo * 3, ne, pre_lds + 2 * dw0);
    pre_stage(src1, total, row1 + (long)lo * 3, ne, pre_lds + 2 * dw0 + dw1);
    __syncthreads();
  }
  const int j = jb + threadIdx.x * 4;
  if (j >= wc) return;
  const int x = xw + j, nvalid = wc - j;
  int s0[4], s1[4];
  Coef a[4];
  bool in[4];
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    in[q] = any && q < nvalid && x + q < rs.Wr;
    s0[q] = s1[q] = lo;
    a[q] = Coef();
    if (in[q]) {
      s0[q] = min(max(rs.xs[x + q], lo), hi);
      s1[q] = min(s0[q] + 1, hi);
      a[q] = rs.xc[x + q];
    }
  }
  const long plane = (long)hc * wc;
  float* d = dst + (long)k * 6 * plane + (long)i * wc + j;
  if (staged) {                                                            // a staged row starts at byte (its first byte & 3) of its first dword
    const long f0 = row0 + (long)lo * 3, f1 = row1 + (long)lo * 3;
    const unsigned char* l = (const unsigned char*)pre_lds;
    pre_resize_modality<0, FX>((const T0*)(l + ((f0 * (long)sizeof(T0)) & 3)), (const T0*)(l + 4 * dw0 + ((f1 * (long)sizeof(T0)) & 3)), lo, s0, s1, a, bq,
                               in, p, d, plane, nvalid);
    pre_resize_modality<1, FX>((const T1*)(l + 8 * dw0 + ((f0 * (long)sizeof(T1)) & 3)), (const T1*)(l + 8 * dw0 + 4 * dw1 + ((f1 * (long)sizeof(T1)) & 3)), lo,
                               s0, s1, a, bq, in, p, d, plane, nvalid);
  } else {
    pre_resize_modality<0, FX>(src0 + row0, src0 + row1, 0, s0, s1, a, bq, in, p, d, plane, nvalid);
    pre_resize_modality<1, FX>(src1 + row0, src1 + row1, 0, s0, s1, a, bq, in, p, d, plane, nvalid);
  }
}

// grid (cdiv(wc, 1024), hc, n): output row i of window / image k.  WT = WindowTable: window k = (image, y0, x0) of the padded canvas;
// WT = NoWindows: image k at (0, 0), hc x wc = the canvas.  RS = NoResize: the canvas holds the source itself at (0, 0); RS = ResizeTables: the
// source resized to Hr x Wr (B = images in the source: the bound of the staged loads).
template <typename T0, typename T1, typename WT, typename RS>
__global__ __launch_bounds__(256) void preprocess_kernel(const T0* __restrict__ src0, const T1* __restrict__ src1, int B, int Hs, int Ws,
                                                         float* __restrict__ dst, int hc, int wc, PreParams p, WT wt, RS rs) {
  if constexpr (sizeof(RS) > 1) {
    pre_resize_block<T0, T1, WT, pre_is_fixed<RS>::value>(src0, src1, B, Hs, Ws, dst, hc, wc, p, wt, rs);
  } else {
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
}

template <typename WT, typename RS>
static void pre_launch(const void* s0, int t0, const void* s1, int t1, int B, int Hs, int Ws, float* dst, int hc, int wc, int n, const PreParams& p,
                       const WT& wt, const RS& rs, size_t lds, hipStream_t stream) {
  const dim3 grid(cdiv(wc, 1024), hc, n), block(256);
  typedef unsigned char u8;
  if (t0 == MMSA_PRE_U8 && t1 == MMSA_PRE_U8) {
    hipLaunchKernelGGL((preprocess_kernel<u8, u8, WT, RS>), grid, block, lds, stream, (const u8*)s0, (const u8*)s1, B, Hs, Ws, dst, hc, wc, p, wt, rs);
  } else if constexpr (!pre_is_fixed<RS>::value) {                         // the fixed-point form exists for uint8 + uint8 only (checked by the entries)
    if (t0 == MMSA_PRE_U8)
      hipLaunchKernelGGL((preprocess_kernel<u8, float, WT, RS>), grid, block, lds, stream, (const u8*)s0, (const float*)s1, B, Hs, Ws, dst, hc, wc, p, wt, rs);
    else if (t1 == MMSA_PRE_U8)
      hipLaunchKernelGGL((preprocess_kernel<float, u8, WT, RS>), grid, block, lds, stream, (const float*)s0, (const u8*)s1, B, Hs, Ws, dst, hc, wc, p, wt, rs);
    else
      hipLaunchKernelGGL((preprocess_kernel<float, float, WT, RS>), grid, block, lds, stream, (const float*)s0, (const float*)s1, B, Hs, Ws, dst, hc, wc, p, wt, rs);
  }
}

// Hfit x Wfit: what must fit into the H x W canvas -- the source itself, or the resized frame (`what` names it in the message)
static int pre_params(PreParams& p, const void* src0, int dtype0, const void* src1, int dtype1, int B, int Hs, int Ws, const float* mean,
                      const float* sinv, const int* div255, const int* swap, const float* pad_val, const float* dst, int H, int W, int Hfit, int Wfit,
                      const char* what, const char* name) {
  MMSA_CHECK_ARG(src0 && src1 && dst && mean && sinv && div255 && swap && pad_val, "%s: null argument", name);
  MMSA_CHECK_ARG((dtype0 == MMSA_PRE_U8 || dtype0 == MMSA_PRE_F32) && (dtype1 == MMSA_PRE_U8 || dtype1 == MMSA_PRE_F32),
                 "%s: source dtypes (%d, %d) must be MMSA_PRE_U8 or MMSA_PRE_F32", name, dtype0, dtype1);
  MMSA_CHECK_ARG(B > 0 && B <= 65535 && Hs > 0 && Ws > 0, "%s: bad source shape [%d, %d, %d, 3]", name, B, Hs, Ws);
  MMSA_CHECK_ARG(H >= Hfit && W >= Wfit, "%s: the %d x %d canvas is smaller than the %d x %d %s (padding only grows a frame)", name, H, W, Hfit, Wfit, what);
  for (int c = 0; c < 6; ++c) {
    MMSA_CHECK_ARG(mean[c] == mean[c] && sinv[c] - sinv[c] == 0.f && sinv[c] != 0.f, "%s: mean / sinv of channel %d is not a finite, non-zero scale", name, c);
    p.mean[c] = mean[c];
    p.sinv[c] = sinv[c];
  }
  for (int m = 0; m < 2; ++m) { p.pad_val[m] = pad_val[m]; p.div255[m] = div255[m] != 0; p.swap[m] = swap[m] != 0; }
  return MMSA_OK;
}

static int pre_windows(WindowTable& wt, const int* windows, int n, int B, int H, int W, int hc, int wc, const char* name) {
  MMSA_CHECK_ARG(hc > 0 && wc > 0 && hc <= 65535, "%s: bad crop size %d x %d", name, hc, wc);
  MMSA_CHECK_ARG(windows && n > 0 && n <= MMSA_MAX_WINDOWS, "%s: 1..%d windows per call", name, MMSA_MAX_WINDOWS);
  wt.n = n;
  for (int k = 0; k < n; ++k) {      // checked against the PADDED canvas: a window may reach into the padding, never beyond it
    wt.b[k] = windows[3 * k]; wt.y0[k] = windows[3 * k + 1]; wt.x0[k] = windows[3 * k + 2];
    MMSA_CHECK_ARG(wt.b[k] >= 0 && wt.b[k] < B && wt.y0[k] >= 0 && wt.x0[k] >= 0 && wt.y0[k] + hc <= H && wt.x0[k] + wc <= W,
                   "%s: window %d (image %d, y0 %d, x0 %d, %dx%d) outside the [%d, %d, %d] canvas", name, k, wt.b[k], wt.y0[k], wt.x0[k], hc, wc, B, H, W);
  }
  return MMSA_OK;
}

extern "C" int mmsa_preprocess_nhwc(const void* src0, int dtype0, const void* src1, int dtype1, int B, int Hs, int Ws, const float* mean,
                                    const float* sinv, const int* div255, const int* swap, const float* pad_val, float* dst, int H, int W,
                                    hipStream_t stream) {
  PreParams p;
  int rc = pre_params(p, src0, dtype0, src1, dtype1, B, Hs, Ws, mean, sinv, div255, swap, pad_val, dst, H, W, Hs, Ws, "source", "preprocess_nhwc");
  if (rc) return rc;
  MMSA_CHECK_ARG(H <= 65535, "preprocess_nhwc: H too large for the launch grid");
  pre_launch(src0, dtype0, src1, dtype1, B, Hs, Ws, dst, H, W, B, p, NoWindows(), NoResize(), 0, stream);
  MMSA_CHECK_LAUNCH("preprocess_nhwc");
  return MMSA_OK;
}

extern "C" int mmsa_preprocess_crops(const void* src0, int dtype0, const void* src1, int dtype1, int B, int Hs, int Ws, const float* mean,
                                     const float* sinv, const int* div255, const int* swap, const float* pad_val, int H, int W,
                                     const int* windows /* HOST [n,3]: image, y0, x0 */, int n, float* dst, int hc, int wc, hipStream_t stream) {
  PreParams p;
  int rc = pre_params(p, src0, dtype0, src1, dtype1, B, Hs, Ws, mean, sinv, div255, swap, pad_val, dst, H, W, Hs, Ws, "source", "preprocess_crops");
  if (rc) return rc;
  WindowTable wt;
  rc = pre_windows(wt, windows, n, B, H, W, hc, wc, "preprocess_crops");
  if (rc) return rc;
  pre_launch(src0, dtype0, src1, dtype1, B, Hs, Ws, dst, hc, wc, n, p, wt, NoResize(), 0, stream);
  MMSA_CHECK_LAUNCH("preprocess_crops");
  return MMSA_OK;
}

// ---- the resizing entries ----
static int pre_resize_args(int dtype0, int dtype1, int Hr, int Wr, const int* xofs, const void* xcoef, const int* yofs, const void* ycoef, int fixed_point,
                           const char* name) {
  MMSA_CHECK_ARG(Hr > 0 && Wr > 0 && xofs && xcoef && yofs && ycoef, "%s: bad resized size %d x %d or a null table", name, Hr, Wr);
  MMSA_CHECK_ARG(!fixed_point || (dtype0 == MMSA_PRE_U8 && dtype1 == MMSA_PRE_U8),
                 "%s: the fixed-point resize needs two uint8 sources (dtypes %d, %d): a pair with a float32 modality is resized in float32", name, dtype0, dtype1);
  return MMSA_OK;
}

// Staging buffer of a launch: `cap` source pixels per row cover every workgroup's span (seg output pixels at scale Ws / Wr, plus the second tap and
// the two roundings); two rows per modality.  No staging (cap 0, the taps are read from global memory) when that exceeds the 64 KiB a launch
// gets without an attribute, or when a source pointer is not dword-aligned.
template <typename WT>
static void pre_resize_launch(const void* s0, int t0, const void* s1, int t1, int B, int Hs, int Ws, float* dst, int hc, int wc, int n, const PreParams& p,
                              const WT& wt, int Hr, int Wr, const int* xofs, const void* xcoef, const int* yofs, const void* ycoef, int fixed_point,
                              hipStream_t stream) {
  const int seg = wc < 1024 ? wc : 1024, e0 = t0 == MMSA_PRE_U8 ? 1 : 4, e1 = t1 == MMSA_PRE_U8 ? 1 : 4;
  long cap = ((long)seg * Ws + Wr - 1) / Wr + 3;
  if (cap > Ws) cap = Ws;
  size_t lds = 8 * ((size_t)pre_stage_dwords(e0, (int)cap) + (size_t)pre_stage_dwords(e1, (int)cap));
  if (lds > 65536 || ((((uintptr_t)s0) | ((uintptr_t)s1)) & 3) != 0) { cap = 0; lds = 0; }
  if (fixed_point) {
    const ResizeTables<true> rs = {Hr, Wr, xofs, (const short2*)xcoef, yofs, (const short2*)ycoef, (int)cap};
    pre_launch(s0, t0, s1, t1, B, Hs, Ws, dst, hc, wc, n, p, wt, rs, lds, stream);
  } else {
    const ResizeTables<false> rs = {Hr, Wr, xofs, (const float2*)xcoef, yofs, (const float2*)ycoef, (int)cap};
    pre_launch(s0, t0, s1, t1, B, Hs, Ws, dst, hc, wc, n, p, wt, rs, lds, stream);
  }
}

extern "C" int mmsa_preprocess_resize_nhwc(const void* src0, int dtype0, const void* src1, int dtype1, int B, int Hs, int Ws, const float* mean,
                                           const float* sinv, const int* div255, const int* swap, const float* pad_val, float* dst, int H, int W,
                                           int Hr, int Wr, const int* xofs, const void* xcoef, const int* yofs, const void* ycoef, int fixed_point,
                                           hipStream_t stream) {
  PreParams p;
  int rc = pre_params(p, src0, dtype0, src1, dtype1, B, Hs, Ws, mean, sinv, div255, swap, pad_val, dst, H, W, Hr, Wr, "resized frame", "preprocess_resize_nhwc");
  if (rc) return rc;
  rc = pre_resize_args(dtype0, dtype1, Hr, Wr, xofs, xcoef, yofs, ycoef, fixed_point, "preprocess_resize_nhwc");
  if (rc) return rc;
  MMSA_CHECK_ARG(H <= 65535, "preprocess_resize_nhwc: H too large for the launch grid");
  pre_resize_launch(src0, dtype0, src1, dtype1, B, Hs, Ws, dst, H, W, B, p, NoWindows(), Hr, Wr, xofs, xcoef, yofs, ycoef, fixed_point, stream);
  MMSA_CHECK_LAUNCH("preprocess_resize_nhwc");
  return MMSA_OK;
}

extern "C" int mmsa_preprocess_resize_crops(const void* src0, int dtype0, const void* src1, int dtype1, int B, int Hs, int Ws, const float* mean,
                                            const float* sinv, const int* div255, const int* swap, const float* pad_val, int H, int W,
                                            const int* windows /* HOST [n,3]: image, y0, x0 */, int n, float* dst, int hc, int wc, int Hr, int Wr,
                                            const int* xofs, const void* xcoef, const int* yofs, const void* ycoef, int fixed_point, hipStream_t stream) {
  PreParams p;
  int rc = pre_params(p, src0, dtype0, src1, dtype1, B, Hs, Ws, mean, sinv, div255, swap, pad_val, dst, H, W, Hr, Wr, "resized frame", "preprocess_resize_crops");
  if (rc) return rc;
  rc = pre_resize_args(dtype0, dtype1, Hr, Wr, xofs, xcoef, yofs, ycoef, fixed_point, "preprocess_resize_crops");
  if (rc) return rc;
  WindowTable wt;
  rc = pre_windows(wt, windows, n, B, H, W, hc, wc, "preprocess_resize_crops");
  if (rc) return rc;
  pre_resize_launch(src0, dtype0, src1, dtype1, B, Hs, Ws, dst, hc, wc, n, p, wt, Hr, Wr, xofs, xcoef, yofs, ycoef, fixed_point, stream);
  MMSA_CHECK_LAUNCH("preprocess_resize_crops");
  return MMSA_OK;
}
