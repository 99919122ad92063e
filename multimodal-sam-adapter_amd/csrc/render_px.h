// One picture pixel, shared by csrc/render.hip (show_result) and csrc/render_diag.hip (the diagnostic pictures): ONE statement of the blend and of the
// de-normalisation, so that every picture rounds the way show_result does.
#pragma once

// The blend is numpy's: two float64 products and one float64 sum, each rounded, then truncation.  A fused multiply-add gives another picture (with
// opacity 0.3, 5284 of the 65536 (image, colour) pairs have an integer exact result that the three roundings land just below).  The de-normalisation
// is the float32 sequence n * std + mean (cv2.multiply, cv2.add), one rounding per step.  Neither may be contracted.
#pragma clang fp contract(off)

enum { RENDER_NONE = 0, RENDER_RAW = 1, RENDER_TENSOR = 2 };

struct RenderDenorm { float mean[3], std[3]; int swap, mul255; };    // per tensor PLANE; swap = to_rgb (planes 2, 1, 0 are the picture's channels 0, 1, 2)

__device__ __forceinline__ unsigned render_blend(unsigned img, unsigned col, double om, double op) {
  const double a = (double)img * om;
  const double c = (double)col * op;
  const double s = a + c;
  return (unsigned)(int)s;                 // 0 <= s < 256: both weights lie in [0, 1] and their sum is 1 up to one rounding
}

// one picture pixel, packed c0 | c1 << 8 | c2 << 16: the source pixel (packed the same way) under the palette colour
__device__ __forceinline__ unsigned render_pixel(unsigned src, unsigned col, double om, double op) {
  return render_blend(src & 255u, col & 255u, om, op) | (render_blend((src >> 8) & 255u, (col >> 8) & 255u, om, op) << 8) |
         (render_blend((src >> 16) & 255u, (col >> 16) & 255u, om, op) << 16);
}

// float -> uint8 by truncation; out-of-range values saturate (the reference's cast is C's, undefined for them), NaN -> 0
__device__ __forceinline__ unsigned render_u8(float v) { return v >= 255.f ? 255u : (v > 0.f ? (unsigned)(int)v : 0u); }

__device__ __forceinline__ unsigned render_denorm(float n0, float n1, float n2, const RenderDenorm& dn) {
  float d0 = n0 * dn.std[0];
  float d1 = n1 * dn.std[1];
  float d2 = n2 * dn.std[2];
  d0 = d0 + dn.mean[0];
  d1 = d1 + dn.mean[1];
  d2 = d2 + dn.mean[2];
  if (dn.swap) { const float t = d0; d0 = d2; d2 = t; }
  if (dn.mul255) { d0 = d0 * 255.f; d1 = d1 * 255.f; d2 = d2 * 255.f; }
  return render_u8(d0) | (render_u8(d1) << 8) | (render_u8(d2) << 16);
}

__device__ __forceinline__ unsigned render_swap02(unsigned v) { return ((v & 255u) << 16) | (v & 0xff00u) | ((v >> 16) & 255u); }
