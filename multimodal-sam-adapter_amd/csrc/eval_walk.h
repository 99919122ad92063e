// The pixel walk of the passes over a STORED class map: csrc/evaluate.hip (confusion counts), csrc/calibrate.hip (reliability bins) and
// csrc/selective.hip (confusion counts per confidence bin).  A header of its own and not a part of csrc/eval_hist.h: that one is what the fused
// class-map kernel of csrc/segment.hip shares (the histogram, the LUT, the argument check), and its pixel comes from the class-map computation, not
// from a walk over memory.
// One pass over 2 bytes per pixel (pred, label), or 6 with the float32 confidence map, HBM-bound: a workgroup of 256 lanes walks CHUNK pixels --
// whole rows where the label goes through the nearest-neighbour tables (TABLES: the label is read at [ymap[y], xmap[x]], clamped into the label map
// whatever the tables hold), one flat run of image blockIdx.y otherwise.  A span reads pred as dwords, conf as float4 where that span's address is
// 16-byte aligned (four dword loads otherwise), the label as dwords where it shares pred's alignment and no table is in the way; an edge path, one
// pixel per lane, serves the unaligned head and tail.  What happens to the pixels once they are in registers is the pass's POLICY:
//   static constexpr bool CONF     the pass reads the confidence map (false: no conf address is formed, nothing is loaded)
//   bool edge_lanes(int nedge)     the lanes that make the edge path's add (whole waves where the add needs them)
//   Px none()                      the edge path, one pixel per lane: what the pass keeps of a pixel (its bin; calibration: also whether it is correct
//   Px pixel(label_byte, pred_byte, c)     and its fixed-point confidence), none() for a lane without one,
//   void add1(Px)                  and the add
//   void add4(has, lv, pv, cv)     the dword loop, four pixels per lane: the packed label and pred dwords (pixel j in byte j) and their confidences;
//                                  has == false: this lane has none
// add1() and add4() are called by every lane of edge_lanes() / of the workgroup together, so that they may vote across the wave.
#pragma once
#include "eval_hist.h"

struct EvalWalkArgs {            // the maps of a launch
  const unsigned char* pred;     // [B, H, W]
  const float* conf;             // [B, H, W] (CONF passes)
  const unsigned char* label;    // [B, Hl, Wl]
  const unsigned char* lut;      // [256]
  const int* ymap;               // [H] / [W] source row / column of the nearest-neighbour resize, or both NULL (Hl == H, Wl == W)
  const int* xmap;
  unsigned long long* out;       // the pass's int64 result, [n_slots, ...]
  int H, W, Hl, Wl, C, K;        // K: confidence bins (CONF passes)
};

template <bool TABLES>
__device__ __forceinline__ unsigned eval_label_at(const unsigned char* __restrict__ l, const int* __restrict__ xmap, int Wl, int i) {
  if (TABLES) return l[min(max(xmap[i], 0), Wl - 1)];
  return l[i];
}

// n pixels: pred p[0..n) and conf c[0..n) against label l[0..n) (TABLES: l[xmap[0..n)], a label ROW)
template <bool TABLES, class Policy>
__device__ __forceinline__ void eval_walk_span(const unsigned char* __restrict__ p, const float* __restrict__ c, const unsigned char* __restrict__ l,
                                               const int* __restrict__ xmap, int Wl, int n, const Policy& pol) {
  const int head = min(n, (int)((4u - (unsigned)((uintptr_t)p & 3u)) & 3u));     // bytes in front of the first aligned pred dword
  const int ndw = (n - head) >> 2;
  const int tail0 = head + (ndw << 2);
  const int nedge = head + (n - tail0);                                          // edge path: at most 3 + 3 pixels, one lane each
  if (pol.edge_lanes(nedge)) {
    typename Policy::Px px = pol.none();
    if ((int)threadIdx.x < nedge) {
      const int i = (int)threadIdx.x < head ? (int)threadIdx.x : tail0 + ((int)threadIdx.x - head);
      px = pol.pixel(eval_label_at<TABLES>(l, xmap, Wl, i), p[i], Policy::CONF ? c[i] : 0.0f);
    }
    pol.add1(px);
  }
  const unsigned* __restrict__ pw = (const unsigned*)(p + head);
  const float* __restrict__ cw = Policy::CONF ? c + head : nullptr;
  const bool c16 = (((uintptr_t)cw) & 15u) == 0;                                 // this span's confidences start on a 16-byte boundary: float4 loads
  const bool ldw = !TABLES && (((uintptr_t)(l + head)) & 3u) == 0;               // the label shares pred's alignment: dwords too
  for (int i0 = 0; i0 < ndw; i0 += 256) {
    const int i = i0 + (int)threadIdx.x;
    const bool has = i < ndw;
    unsigned pv = 0u, lv = 0u;
    float4 cv = {0.0f, 0.0f, 0.0f, 0.0f};
    if (has) {
      pv = pw[i];
      const int base = head + 4 * i;
      if (ldw)
        lv = ((const unsigned*)(l + head))[i];
      else
        lv = eval_label_at<TABLES>(l, xmap, Wl, base) | (eval_label_at<TABLES>(l, xmap, Wl, base + 1) << 8) |
             (eval_label_at<TABLES>(l, xmap, Wl, base + 2) << 16) | (eval_label_at<TABLES>(l, xmap, Wl, base + 3) << 24);
      if constexpr (Policy::CONF) {
        if (c16) {
          cv = ((const float4*)cw)[i];
        } else {
          cv.x = cw[4 * i];
          cv.y = cw[4 * i + 1];
          cv.z = cw[4 * i + 2];
          cv.w = cw[4 * i + 3];
        }
      }
    }
    pol.add4(has, lv, pv, cv);
  }
}

// The body of a walk kernel between its LDS set-up and its flush: this workgroup's rows (blockIdx.x * rows .., one span per row) or its flat run
// (CHUNK pixels from blockIdx.x * CHUNK) of image b.
template <bool TABLES, int CHUNK, class Policy>
__device__ __forceinline__ void eval_walk(const EvalWalkArgs& a, int b, int rows, const Policy& pol) {
  const int H = a.H, W = a.W;
  if (TABLES) {
    const int y1 = min(H, ((int)blockIdx.x + 1) * rows);
    for (int y = (int)blockIdx.x * rows; y < y1; ++y) {
      const int ys = min(max(a.ymap[y], 0), a.Hl - 1);
      const long at = ((long)b * H + y) * W;
      eval_walk_span<true>(a.pred + at, Policy::CONF ? a.conf + at : nullptr, a.label + ((long)b * a.Hl + ys) * a.Wl, a.xmap, a.Wl, W, pol);
    }
  } else {                                             // same size: image b is one run of H * W pixels
    const long HW = (long)H * W, start = (long)blockIdx.x * CHUNK;
    const int n = (int)min((long)CHUNK, HW - start);
    const long at = b * HW + start;
    eval_walk_span<false>(a.pred + at, Policy::CONF ? a.conf + at : nullptr, a.label + at, nullptr, 0, n, pol);
  }
}

// host: the launch pair of a walk kernel, `tab` = kernel<true> over whole rows, `flat` = kernel<false> over runs of `chunk` pixels; both take
// (args..., rows).  Grid (chunks, B, gz), 256 lanes, `lds` dynamic bytes.
template <class Kernel, class... Args>
static inline void eval_walk_launch(Kernel tab, Kernel flat, bool tables, int chunk, int B, int H, int W, int gz, size_t lds, hipStream_t stream,
                                    Args... args) {
  if (tables) {
    const int rows = max(1, cdiv(chunk, W));
    hipLaunchKernelGGL(tab, dim3(cdiv(H, rows), B, gz), dim3(256), lds, stream, args..., rows);
  } else {
    hipLaunchKernelGGL(flat, dim3(cdiv((long)H * W, (long)chunk), B, gz), dim3(256), lds, stream, args..., 0);
  }
}
