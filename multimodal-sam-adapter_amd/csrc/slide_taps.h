// The tap arithmetic of the rescaled class map, shared by csrc/segment.hip (mmsa_slide_argmax_resized) and csrc/augment.hip (mmsa_aug_argmax): which windows
// cover a canvas pixel, one window's interpolated term, a canvas pixel's averaged value in window order, and the two-stage pixel built of four such canvas
// pixels (TwoStagePixel: its set-up and its value for one class -- the ONE copy of that text; the kernels of both files only loop over the classes).  The
// functions are templates on the window table, which says where a window's (image, y0, x0) comes from:
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

// host: window k (image wb, y0, x0; hc x wc) lies inside the [B, H, W] input, or the call fails in `name`'s name (view >= 0: a view of an augmented frame)
static inline int check_window(const char* name, int view, int k, int wb, int y0, int x0, int hc, int wc, int B, int H, int W) {
  if (wb >= 0 && wb < B && y0 >= 0 && x0 >= 0 && y0 + hc <= H && x0 + wc <= W) return MMSA_OK;
  char of_view[24] = "";
  if (view >= 0) snprintf(of_view, sizeof of_view, "view %d ", view);
  mmsa_set_error("%s: %swindow %d (image %d, y0 %d, x0 %d, %dx%d) outside the [%d, %d, %d] input", name, of_view, k, wb, y0, x0, hc, wc, B, H, W);
  return MMSA_ERR_ARG;
}

// Registers: four taps with the eight slots of slide_pixel.h would need 4 x 56 (the first form did: 372 registers, one wave per SIMD).  Here a tap
// keeps RESIZED_SLOTS = 4 windows, each packed to four registers (offset of the top-left logit, window index | "has a row below" << 8 | "has a column
// to the right" << 9, the two weights); a pixel with a tap under 5 .. 8 windows (strides below half the crop) takes the scanning form instead, which walks
// the window table again for every class and keeps nothing.  Same terms, same order, same bits either way.
#define RESIZED_SLOTS 4
struct TapSlots { int nk; int o[RESIZED_SLOTS], kf[RESIZED_SLOTS]; float lh[RESIZED_SLOTS], lw[RESIZED_SLOTS]; };

// window k of image b over canvas pixel (ty, tx)?  -> its 4-tap coordinates in the window's logits, as slide_pixel.h computes them
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

// one window's term of a canvas pixel: the interpolation of bilinear_accum_kernel / slide_pixel.h
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

// ---- the two-stage pixel: output pixel (Y, X) of the second bilinear resize (align_corners=False) of the averaged H x W canvas.  Each of its four taps
// (tap t: row y0 / y1 = t >> 1, column x0 / x1 = t & 1) is a canvas pixel with its own covering windows and its own count.
struct TwoStagePixel { TapSlots tp[4]; int y0, y1, x0, x1; float lh2, lw2; int nmin, nmax; };

// nmin == 0: a tap without a window; nmax > 8: a tap under more than 8 -- the callers refuse both.  nmax <= RESIZED_SLOTS: the slots hold every window.
template <class WT>
__device__ __forceinline__ void two_stage_setup(TwoStagePixel& px, const WT& wt, int b, int Y, int X, int H, int W, int hc, int wc, int hs, int ws,
                                                float rh, float rw, float rh2, float rw2) {
  // second stage: the taps of output pixel (Y, X) in the H x W canvas (bilinear_accum_kernel with src = the canvas)
  float sh2 = ((float)Y + 0.5f) * rh2 - 0.5f, sw2 = ((float)X + 0.5f) * rw2 - 0.5f;
  sh2 = sh2 < 0.f ? 0.f : sh2;
  sw2 = sw2 < 0.f ? 0.f : sw2;
  const int y0 = min((int)sh2, H - 1), x0 = min((int)sw2, W - 1);
  const int y1 = y0 + (y0 < H - 1 ? 1 : 0), x1 = x0 + (x0 < W - 1 ? 1 : 0);
  px.y0 = y0; px.y1 = y1; px.x0 = x0; px.x1 = x1;
  px.lh2 = sh2 - (float)y0; px.lw2 = sw2 - (float)x0;
  // first stage: the covering windows of each tap.  Slot arrays only ever indexed by unrolled constants.
  TapSlots (&tp)[4] = px.tp;
#pragma unroll
  for (int t = 0; t < 4; ++t) {
    tp[t].nk = 0;
#pragma unroll
    for (int q = 0; q < RESIZED_SLOTS; ++q) { tp[t].o[q] = tp[t].kf[q] = 0; tp[t].lh[q] = tp[t].lw[q] = 0.f; }
  }
  for (int k = 0; k < win_n(wt); ++k) {
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      int o, kf;
      float lh, lw;
      if (!tap_coords(wt, k, b, t >> 1 ? y1 : y0, t & 1 ? x1 : x0, hc, wc, hs, ws, rh, rw, o, kf, lh, lw)) continue;
#pragma unroll
      for (int q = 0; q < RESIZED_SLOTS; ++q)
        if (q == tp[t].nk) { tp[t].o[q] = o; tp[t].kf[q] = kf; tp[t].lh[q] = lh; tp[t].lw[q] = lw; }
      ++tp[t].nk;
    }
  }
  px.nmin = min(min(tp[0].nk, tp[1].nk), min(tp[2].nk, tp[3].nk));
  px.nmax = max(max(tp[0].nk, tp[1].nk), max(tp[2].nk, tp[3].nk));
}

// The pixel's value for class c.  SCAN false: from the slots (tap_value; needs nmax <= RESIZED_SLOTS); true: the scanning form (tap_value_scan).  The caller
// makes that choice once, outside its loop over c.
template <bool SCAN, class WT>
__device__ __forceinline__ float two_stage_value(const TwoStagePixel& px, const WT& wt, int b, const float* __restrict__ logits, int C, int c, int hs, int ws,
                                                 int hc, int wc, float rh, float rw) {
  float p00, p01, p10, p11;
  if constexpr (SCAN) {
    p00 = tap_value_scan(wt, b, px.y0, px.x0, px.tp[0].nk, logits, C, c, hs, ws, hc, wc, rh, rw);
    p01 = tap_value_scan(wt, b, px.y0, px.x1, px.tp[1].nk, logits, C, c, hs, ws, hc, wc, rh, rw);
    p10 = tap_value_scan(wt, b, px.y1, px.x0, px.tp[2].nk, logits, C, c, hs, ws, hc, wc, rh, rw);
    p11 = tap_value_scan(wt, b, px.y1, px.x1, px.tp[3].nk, logits, C, c, hs, ws, hc, wc, rh, rw);
  } else {
    p00 = tap_value(px.tp[0], logits, C, c, hs, ws); p01 = tap_value(px.tp[1], logits, C, c, hs, ws);
    p10 = tap_value(px.tp[2], logits, C, c, hs, ws); p11 = tap_value(px.tp[3], logits, C, c, hs, ws);
  }
  const float lh2 = px.lh2, lw2 = px.lw2;
  return (1.f - lh2) * ((1.f - lw2) * p00 + lw2 * p01) + lh2 * ((1.f - lw2) * p10 + lw2 * p11);
}
