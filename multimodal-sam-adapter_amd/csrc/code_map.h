// How the passes over stored maps read a code: csrc/distance.hip (the row pass and the count passes), csrc/components.hip, csrc/pairs.hip and
// csrc/segtable.hip.  A CODE MAP is one byte per pixel of a grid [B, H, W], M(y, x) = lut[src[b, ymap[y], xmap[x]]]: a stored class map through the
// LUT, or raw labels through the LUT and the nearest-neighbour tables of the label side.  The kernels compare bytes and know nothing of classes.
#pragma once
#include "common.h"
#include "eval_hist.h"

struct CodeSrc {                    // the source of a code-map launch
  const unsigned char* src;         // [B, Hs, Ws]
  const unsigned char* lut;         // [256] or NULL (identity)
  const int* ymap;                  // [H] / [W] source row / column, or both NULL (Hs == H, Ws == W)
  const int* xmap;
  int Hs, Ws, H, W;
};

// What a launcher checks before it makes a CodeSrc of its arguments; `size_text` is the entry's own word for a source size that is not positive or not
// below 2^31 ("bad map size", "bad source size").
static inline int code_src_check(const char* name, const char* size_text, int Hs, int Ws, const int* ymap, const int* xmap, int H, int W) {
  MMSA_CHECK_ARG(Hs > 0 && Ws > 0 && (long)Hs * Ws < (1l << 31), "%s: %s", name, size_text);
  MMSA_CHECK_ARG((ymap != NULL) == (xmap != NULL), "%s: ymap and xmap come together", name);
  MMSA_CHECK_ARG(ymap || (Hs == H && Ws == W), "%s: size mismatch: the source is %d x %d, the grid %d x %d, and no ymap / xmap tables were given", name, Hs,
                 Ws, H, W);
  return MMSA_OK;
}

// grid index i of one axis -> the source index, clamped into the n source rows / columns: a table from elsewhere cannot send a read outside the map
__device__ __forceinline__ int code_axis(const int* map, int i, int n) { return map ? min(max(map[i], 0), n - 1) : i; }
__device__ __forceinline__ int code_of(const CodeSrc& s, int v) { return s.lut ? (int)s.lut[v] : v; }

// M(y, x) of image b: 0 <= y < H, 0 <= x < W
__device__ __forceinline__ int code_at(const CodeSrc& s, int b, int y, int x) {
  const int ys = code_axis(s.ymap, y, s.Hs), xs = code_axis(s.xmap, x, s.Ws);
  return code_of(s, s.src[((long)b * s.Hs + ys) * s.Ws + xs]);
}

// the same for a pass that walks along a row: the source row resolved once, then x alone
__device__ __forceinline__ const unsigned char* code_row(const CodeSrc& s, int b, int y) { return s.src + ((long)b * s.Hs + code_axis(s.ymap, y, s.Hs)) * s.Ws; }
__device__ __forceinline__ int code_at(const CodeSrc& s, const unsigned char* __restrict__ row, int x) { return code_of(s, row[code_axis(s.xmap, x, s.Ws)]); }

// pixel i of image b: its label code (a class < C, C, or MMSA_EVAL_IGNORE), read through the tables where there are any.  `lut` = ev.lut, or the copy of
// it that a pass keeps in LDS.
__device__ __forceinline__ int label_code(const EvalLabel& ev, const unsigned char* lut, int b, int W, int i) {      // H * W < 2^31
  long at = i;
  if (ev.ymap) {
    const int y = i / W, x = i - y * W;
    at = (long)min(max(ev.ymap[y], 0), ev.Hl - 1) * ev.Wl + min(max(ev.xmap[x], 0), ev.Wl - 1);
  }
  const int l = lut[ev.label[(long)b * ev.Hl * ev.Wl + at]];
  return l == MMSA_EVAL_IGNORE ? l : min(l, ev.C);
}
