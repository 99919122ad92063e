// The tap arithmetic of the rescaled class map, shared by csrc/segment.hip (mmsa_slide_argmax_resized) and csrc/augment.hip (mmsa_aug_argmax): which windows
// cover a canvas pixel, one window's interpolated term, and a canvas pixel's averaged value in window order.  The functions are templates on the window
// table, which says where a window's (image, y0, x0) comes from:
//   WindowTable : by value in the launch arguments (at most MMSA_MAX_WINDOWS windows; segment.hip);
//   DevWindows  : a device int [n, 3] array (augment.hip: the tables of all views of an augmented frame do not fit the argument block).
// Include it AFTER `#pragma clang fp contract(off)`: both files must round these formulas the same way (see the top of segment.hip).
#pragma once

#define MMSA_MAX_WINDOWS 64
struct WindowTable { int n; int b[MMSA_MAX_WINDOWS], y0[MMSA_MAX_WINDOWS], x0[MMSA_MAX_WINDOWS]; };
__device__ __forceinline__ int win_n(const WindowTable& wt) { return wt.n; }
__device__ __forceinline__ int win_b(const WindowTable& wt, int k) { return wt.b[k]; }
__device__ __forceinline__ int win_y0(const WindowTable& wt, int k) { return wt.y0[k]; }
__device__ __forceinline__ int win_x0(const WindowTable& wt, int k) { return wt.x0[k]; }

struct DevWindows { const int* t; int n; };      // t = the first of the n rows (image, y0, x0)
__device__ __forceinline__ int win_n(const DevWindows& wt) { return wt.n; }
__device__ __forceinline__ int win_b(const DevWindows& wt, int k) { return wt.t[3 * k]; }
__device__ __forceinline__ int win_y0(const DevWindows& wt, int k) { return wt.t[3 * k + 1]; }
__device__ __forceinline__ int win_x0(const DevWindows& wt, int k) { return wt.t[3 * k + 2]; }

// Registers: four taps with the eight slots of slide_pixel.inc would need 4 x 56 (the first form did: 372 registers, one wave per SIMD).  Here a tap
// keeps RESIZED_SLOTS = 4 windows, each packed to four registers (offset of the top-left logit, window index | "has a row below" << 8 | "has a column
// to the right" << 9, the two weights); a pixel with a tap under 5 .. 8 windows (strides below half the crop) takes the scanning form instead, which walks
// the window table again for every class and keeps nothing.  Same terms, same order, same bits either way.
#define RESIZED_SLOTS 4
struct TapSlots { int nk; int o[RESIZED_SLOTS], kf[RESIZED_SLOTS]; float lh[RESIZED_SLOTS], lw[RESIZED_SLOTS]; };

// window k of image b over canvas pixel (ty, tx)?  -> its 4-tap coordinates in the window's logits, as slide_pixel.inc computes them
template <class WT>
__device__ __forceinline__ bool tap_coords(const WT& wt, int k, int b, int ty, int tx, int hc, int wc, int hs, int ws, float rh, float rw,
                                           int& o, int& kf, float& lh, float& lw) {
  if (win_b(wt, k) != b) return false;
  const int i = ty - win_y0(wt, k), j = tx - win_x0(wt, k);
  if (i < 0 || i >= hc || j < 0 || j >= wc) return false;
  float sh = ((float)i + 0.5f) * rh - 0.5f, sw = ((float)j + 0.5f) * rw - 0.5f;
  sh = sh < 0.f ? 0.f : sh;
  sw = sw < 0.f ? 0.f : sw;
  const int h0 = min((int)sh, hs - 1), w0 = min((int)sw, ws - 1);
  o = h0 * ws + w0;
  kf = k | (h0 < hs - 1 ? 256 : 0) | (w0 < ws - 1 ? 512 : 0);
  lh = sh - (float)h0;
  lw = sw - (float)w0;
  return true;
}

// one window's term of a canvas pixel: the interpolation of bilinear_accum_kernel / slide_pixel.inc
__device__ __forceinline__ float tap_term(const float* __restrict__ logits, int C, int c, int hs, int ws, int o, int kf, float lh, float lw) {
  const int dh = (kf >> 8) & 1 ? ws : 0, dw = (kf >> 9) & 1;
  const float* sp = logits + ((long)(kf & 255) * C + c) * hs * ws + o;
  return (1.f - lh) * ((1.f - lw) * sp[0] + lw * sp[dw]) + lh * ((1.f - lw) * sp[dh] + lw * sp[dh + dw]);
}

__device__ __forceinline__ float tap_value(const TapSlots& t, const float* __restrict__ logits, int C, int c, int hs, int ws) {
  float acc = 0.f;
#pragma unroll
  for (int q = 0; q < RESIZED_SLOTS; ++q) {
    if (q < t.nk) {
      const float v = tap_term(logits, C, c, hs, ws, t.o[q], t.kf[q], t.lh[q], t.lw[q]);
      acc = q == 0 ? v : acc + v;     // window order: the first window WRITES (0 + v == v), later ones add
    }
  }
  return acc / (float)t.nk;
}

template <class WT>
__device__ __forceinline__ float tap_value_scan(const WT& wt, int b, int ty, int tx, int nk, const float* __restrict__ logits, int C, int c,
                                                int hs, int ws, int hc, int wc, float rh, float rw) {
  float acc = 0.f;
  bool first = true;
  for (int k = 0; k < win_n(wt); ++k) {
    int o, kf;
    float lh, lw;
    if (!tap_coords(wt, k, b, ty, tx, hc, wc, hs, ws, rh, rw, o, kf, lh, lw)) continue;
    const float v = tap_term(logits, C, c, hs, ws, o, kf, lh, lw);
    acc = first ? v : acc + v;
    first = false;
  }
  return acc / (float)nk;
}
