// Segment-level evaluation on device: the connected components of a code map (mmsa_components_u8), their areas (mmsa_component_area), the class map without
// its small blobs (mmsa_suppress_small_u8) and the segment counts of a prediction against the ground truth (mmsa_eval_segments: how many label segments were
// found, how many prediction segments are real, by class, by size and by the share of the segment that is covered).  Integers only: the same bytes run after run.
//
// The quantity.  For a code map M (one byte per pixel after the LUT and the nearest-neighbour tables, read through csrc/code_map.h; the kernels compare
// bytes and know nothing of classes) two pixels of one image are connected iff they are 4- or 8-neighbours and hold the same code; a component is a maximal
// connected set, and root[b, y, x] = the smallest linear index y * W + x of the pixel's component, within its own image: canonical, whatever the schedule.
//
// Three launches over parent = root, int32 [B, H, W], with parent[i] <= i throughout; no workgroup waits for another and no loop spins on a value that
// somebody else must write:
//   tile pass     a WORKGROUP per tile of 64 x 32 codes staged in LDS (a border of COMP_NONE around them: no bounds test per neighbour).  Labels start as
//                 the local index; every trip lowers a pixel's label to the smallest label among its equal neighbours (and hangs its old root under it),
//                 then every label jumps to its root; __syncthreads_or(changed) ends the loop.  Local and global order are both row-major inside a tile,
//                 so the local minimum is the global one: parent[p] = the global index of the tile-local root.
//   merge pass    a lane per pixel on the first column / row behind a tile border, and its (up to three) neighbours across it: union(find(a), find(b)).
//                 parent is lowered by atomicMin only and the larger root is hung under the smaller.  parent is READ with relaxed agent-scope atomic loads
//                 (a plain load may be served stale from another XCD's L2 or this CU's L1); a stale parent is still an ancestor, only a larger one, and the
//                 value atomicMin returns is the only thing a decision rests on.
//   flatten pass  a launch of its own, so that it reads final parents: root[p] = find(p).  A lane writes its own pixel only; whoever reads that pixel on its
//                 way up sees the old parent or the root, both ancestors.
// A map of one tile needs the tile pass only.
// The passes on top are pointwise.  A component of half a frame adds to ONE address: a wave first reduces its lanes per distinct root in registers (the
// lowest pending lane's root is broadcast, a ballot counts its lanes, one lane adds their number: the form of csrc/cal_wave.h, at most 64 rounds).
#include "common.h"
#include "eval_hist.h"
#include "code_map.h"
#include "comp_shared.h"

#define COMP_TW 64
#define COMP_TH 32
#define COMP_TILE (COMP_TW * COMP_TH)
#define COMP_PW (COMP_TW + 2)                 // the staged codes with their border
#define COMP_PH (COMP_TH + 2)
#define COMP_NONE 0xffffu                     // no pixel (outside the tile or the image): equal to no code
#define COMP_MAX_BINS 64
#define COMP_RLX_AGENT __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT

// grid.x = tiles_x * tiles_y * B, x fastest.  Lane t owns the local pixels t, t + 256, ...: a wave on one tile row.
__global__ __launch_bounds__(256) void components_tile_kernel(CodeSrc s, int tiles_x, int tiles_y, int conn8, int* __restrict__ parent) {
  __shared__ unsigned short code[COMP_PH * COMP_PW];
  __shared__ int lab[COMP_TILE];
  const long t = blockIdx.x;
  const int tx = (int)(t % tiles_x);
  const long rest = t / tiles_x;
  const int ty = (int)(rest % tiles_y), b = (int)(rest / tiles_y);
  const int x0 = tx * COMP_TW, y0 = ty * COMP_TH, H = s.H, W = s.W;
  for (int i = threadIdx.x; i < COMP_PH * COMP_PW; i += 256) code[i] = (unsigned short)COMP_NONE;
  __syncthreads();
#pragma unroll
  for (int k = 0; k < COMP_TILE / 256; ++k) {
    const int li = k * 256 + (int)threadIdx.x, ly = li / COMP_TW, lx = li % COMP_TW;
    if (y0 + ly < H && x0 + lx < W) code[(ly + 1) * COMP_PW + lx + 1] = (unsigned short)code_at(s, b, y0 + ly, x0 + lx);
    lab[li] = li;
  }
  __syncthreads();
  // Natural exit: a trip that lowers no label.  Bound: labels only fall, and a pixel at d steps from its component's smallest pixel holds that pixel's
  // index after trip d (its neighbour at d - 1 steps held it before), d < COMP_TILE.  The cap is that bound: a mistake shows as a wrong map, not a hang.
  for (int trip = 0; trip <= COMP_TILE; ++trip) {
    int changed = 0;
#pragma unroll
    for (int k = 0; k < COMP_TILE / 256; ++k) {
      const int li = k * 256 + (int)threadIdx.x, ci = (li / COMP_TW + 1) * COMP_PW + li % COMP_TW + 1;
      const unsigned c = code[ci];
      if (c == COMP_NONE) continue;
      const int own = lab[li];
      int m = own;
      if (code[ci - 1] == c) m = min(m, lab[li - 1]);                        // a neighbour outside the tile holds COMP_NONE: its label is never read
      if (code[ci + 1] == c) m = min(m, lab[li + 1]);
      if (code[ci - COMP_PW] == c) m = min(m, lab[li - COMP_TW]);
      if (code[ci + COMP_PW] == c) m = min(m, lab[li + COMP_TW]);
      if (conn8) {
        if (code[ci - COMP_PW - 1] == c) m = min(m, lab[li - COMP_TW - 1]);
        if (code[ci - COMP_PW + 1] == c) m = min(m, lab[li - COMP_TW + 1]);
        if (code[ci + COMP_PW - 1] == c) m = min(m, lab[li + COMP_TW - 1]);
        if (code[ci + COMP_PW + 1] == c) m = min(m, lab[li + COMP_TW + 1]);
      }
      if (m < own) {                                                         // labels are lowered by atomicMin only in this half
        atomicMin(&lab[own], m);                                             // the old root (or an ancestor) goes along
        atomicMin(&lab[li], m);
        changed = 1;
      }
    }
    if (!__syncthreads_or(changed)) break;
#pragma unroll
    for (int k = 0; k < COMP_TILE / 256; ++k) {                              // pointer jumping: nobody lowers by atomicMin in this half
      const int li = k * 256 + (int)threadIdx.x;
      int r = lab[li];
      for (int n = 0; n < COMP_TILE; ++n) {                                  // strictly falling indices: bounded by the tile's pixel count
        const int up = lab[r];
        if (up >= r) break;
        r = up;
      }
      lab[li] = r;                                                           // this lane's own cell; r <= what it held
    }
    __syncthreads();
  }
  int* __restrict__ img = parent + (long)b * H * W;
#pragma unroll
  for (int k = 0; k < COMP_TILE / 256; ++k) {
    const int li = k * 256 + (int)threadIdx.x, ly = li / COMP_TW, lx = li % COMP_TW;
    if (y0 + ly < H && x0 + lx < W) {
      const int r = lab[li];
      img[(y0 + ly) * W + x0 + lx] = (y0 + r / COMP_TW) * W + x0 + r % COMP_TW;      // H * W < 2^31
    }
  }
}

// The root above pixel i as far as this lane can see it.  Strictly falling indices: bounded by i, capped at `cap` = H * W hops.
__device__ __forceinline__ int comp_find(const int* img, int i, int cap) {
  for (int n = 0; n < cap; ++n) {
    const int up = __hip_atomic_load(img + i, COMP_RLX_AGENT);
    if (up >= i) break;                                                      // up == i: a root (up > i never happens: parent[i] <= i)
    i = up;
  }
  return i;
}

// The sets of a and b become one.  hi > lo; atomicMin(parent[hi], lo) returned hi: hi was a root and now hangs under lo -- done.  It returned less: hi had a
// parent `old` already, parent[hi] = min(old, lo) now, and the sets of old and lo are still to be joined: go on from there.  max(old, lo) < hi, so every
// retry starts below the last: bounded by the index, capped at `cap`.
__device__ __forceinline__ void comp_union(int* img, int a, int b, int cap) {
  a = comp_find(img, a, cap);
  b = comp_find(img, b, cap);
  for (int n = 0; n < cap && a != b; ++n) {
    const int hi = max(a, b), lo = min(a, b);
    const int old = atomicMin(img + hi, lo);
    if (old == hi) break;
    a = comp_find(img, old, cap);
    b = lo;
  }
}

// grid (cdiv(nv + nh, 256), B): nv = (tiles_x - 1) * H lanes on the first column behind a vertical tile border, nh = (tiles_y - 1) * W on the first row
// behind a horizontal one.  A pair across a corner is seen from both sides, which does no harm.
__global__ __launch_bounds__(256) void components_merge_kernel(CodeSrc s, int tiles_x, int tiles_y, int conn8, int* parent) {
  const int H = s.H, W = s.W, b = blockIdx.y;
  const long nv = (long)(tiles_x - 1) * H, nh = (long)(tiles_y - 1) * W;
  long j = (long)blockIdx.x * 256 + threadIdx.x;
  if (j >= nv + nh) return;
  int* img = parent + (long)b * H * W;
  const int cap = H * W;
  int y, x, ny[3], nx[3];
  if (j < nv) {                                                              // (y, x) against (y, x - 1), and the two diagonals at 8
    x = ((int)(j / H) + 1) * COMP_TW;
    y = (int)(j % H);
    ny[0] = y, ny[1] = y - 1, ny[2] = y + 1;
    nx[0] = nx[1] = nx[2] = x - 1;
  } else {                                                                   // (y, x) against (y - 1, x), and the two diagonals at 8
    j -= nv;
    y = ((int)(j / W) + 1) * COMP_TH;
    x = (int)(j % W);
    ny[0] = ny[1] = ny[2] = y - 1;
    nx[0] = x, nx[1] = x - 1, nx[2] = x + 1;
  }
  const int c = code_at(s, b, y, x), n = conn8 ? 3 : 1;
  for (int k = 0; k < n; ++k) {
    if (ny[k] < 0 || ny[k] >= H || nx[k] < 0 || nx[k] >= W) continue;
    if (code_at(s, b, ny[k], nx[k]) == c) comp_union(img, y * W + x, ny[k] * W + nx[k], cap);
  }
}

// grid (cdiv(H * W, 256), B), in place: reads the parents the merge launch left, writes its own pixel only
__global__ __launch_bounds__(256) void components_flatten_kernel(int H, int W, int* root) {
  const long HW = (long)H * W, i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= HW) return;
  int* img = root + blockIdx.y * HW;
  int r = img[i];
  for (int n = 0; n < (int)HW; ++n) {                                        // strictly falling indices: bounded by i, capped at H * W hops
    const int up = img[r];
    if (up >= r) break;
    r = up;
  }
  img[i] = r;
}

extern "C" int mmsa_components_u8(const unsigned char* src, int B, int Hs, int Ws, const unsigned char* lut, const int* ymap, const int* xmap, int H, int W,
                                  int connectivity, int* root, hipStream_t stream) {
  const char* name = "components_u8";
  MMSA_CHECK_ARG(src && root, "%s: src and root are required", name);
  int rc = comp_check_size(name, B, H, W);
  if (rc) return rc;
  rc = code_src_check(name, "bad source size", Hs, Ws, ymap, xmap, H, W);
  if (rc) return rc;
  MMSA_CHECK_ARG(connectivity == 4 || connectivity == 8, "%s: connectivity = %d; 4 or 8 is expected", name, connectivity);
  const int tiles_x = cdiv(W, COMP_TW), tiles_y = cdiv(H, COMP_TH), conn8 = connectivity == 8;
  const long tiles = (long)tiles_x * tiles_y * B;                            // <= B * H * W < 2^31
  const CodeSrc s = {src, lut, ymap, xmap, Hs, Ws, H, W};
  hipLaunchKernelGGL(components_tile_kernel, dim3((unsigned)tiles), dim3(256), 0, stream, s, tiles_x, tiles_y, conn8, root);
  if (tiles_x * tiles_y > 1) {
    const long pairs = (long)(tiles_x - 1) * H + (long)(tiles_y - 1) * W;
    hipLaunchKernelGGL(components_merge_kernel, dim3((unsigned)cdiv(pairs, 256l), B), dim3(256), 0, stream, s, tiles_x, tiles_y, conn8, root);
    hipLaunchKernelGGL(components_flatten_kernel, dim3((unsigned)cdiv((long)H * W, 256l), B), dim3(256), 0, stream, H, W, root);
  }
  MMSA_CHECK_LAUNCH("components_u8");
  return MMSA_OK;
}

// ---- the pointwise passes over root maps (comp_wave_add, seg_count_add and the size bucket: csrc/comp_shared.h, shared with csrc/pairs.hip)
// grid (cdiv(H * W, 256), B): a wave lies inside one image
__global__ __launch_bounds__(256) void component_area_kernel(const int* __restrict__ root, int H, int W, int* area) {
  const long HW = (long)H * W, i = (long)blockIdx.x * 256 + threadIdx.x, base = blockIdx.y * HW;
  const bool has = i < HW;
  int r = has ? root[base + i] : 0;
  r = min(max(r, 0), (int)HW - 1);                                           // a root map from elsewhere cannot send the add outside the plane
  comp_wave_add(area + base, nullptr, has, r, false);
}

extern "C" int mmsa_component_area(const int* root, int B, int H, int W, int* area, hipStream_t stream) {
  const char* name = "component_area";
  MMSA_CHECK_ARG(root && area && root != area, "%s: root and area are required, and two planes", name);
  int rc = comp_check_size(name, B, H, W);
  if (rc) return rc;
  rc = comp_zero(name, area, (size_t)B * H * W * sizeof(int), stream);
  if (rc) return rc;
  hipLaunchKernelGGL(component_area_kernel, dim3((unsigned)cdiv((long)H * W, 256l), B), dim3(256), 0, stream, root, H, W, area);
  MMSA_CHECK_LAUNCH("component_area");
  return MMSA_OK;
}

// n = B * H * W pixels, HW per image; out may be pred
__global__ __launch_bounds__(256) void suppress_small_kernel(const unsigned char* pred, const int* __restrict__ root, const int* __restrict__ area, long n, int HW,
                                                             int min_area, int fill, unsigned char* out) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const long base = i / HW * HW;
  const int r = min(max(root[i], 0), HW - 1);
  out[i] = area[base + r] < min_area ? (unsigned char)fill : pred[i];
}

extern "C" int mmsa_suppress_small_u8(const unsigned char* pred, const int* root, const int* area, int B, int H, int W, int min_area, int fill,
                                      unsigned char* out, hipStream_t stream) {
  const char* name = "suppress_small_u8";
  MMSA_CHECK_ARG(pred && root && area && out, "%s: pred, root, area and out are required", name);
  int rc = comp_check_size(name, B, H, W);
  if (rc) return rc;
  MMSA_CHECK_ARG(min_area >= 1, "%s: min_area = %d; at least 1 (the identity) is expected", name, min_area);
  MMSA_CHECK_ARG(fill >= 0 && fill <= 255, "%s: fill = %d; a byte is expected", name, fill);
  const long n = (long)B * H * W;
  hipLaunchKernelGGL(suppress_small_kernel, dim3((unsigned)cdiv(n, 256l)), dim3(256), 0, stream, pred, root, area, n, H * W, min_area, fill, out);
  MMSA_CHECK_LAUNCH("suppress_small_u8");
  return MMSA_OK;
}

struct SegMaps {
  const unsigned char* pred;        // [B, H, W]
  const int* root_pred;             // [B, H, W]
  const int* root_label;
  int* planes;                      // [4, B, H, W]: area and hits of the label segments, area and hits of the prediction segments, at the root pixels
  int H, W, B;
};

// grid (cdiv(H * W, 256), B): every pixel whose label is not ignored adds itself to its label segment and to its prediction segment
__global__ __launch_bounds__(256) void eval_segments_area_kernel(SegMaps m, EvalLabel ev) {
  const long HW = (long)m.H * m.W, i = (long)blockIdx.x * 256 + threadIdx.x, base = blockIdx.y * HW, plane = (long)m.B * HW;
  bool has = i < HW, hit = false;
  int rl = 0, rp = 0;
  if (has) {
    const int l = label_code(ev, ev.lut, blockIdx.y, m.W, (int)i);
    has = l != MMSA_EVAL_IGNORE;
    hit = l < ev.C && min((int)m.pred[base + i], ev.C) == l;
    rl = min(max(m.root_label[base + i], 0), (int)HW - 1);
    rp = min(max(m.root_pred[base + i], 0), (int)HW - 1);
  }
  comp_wave_add(m.planes + base, m.planes + plane + base, has, rl, hit);
  comp_wave_add(m.planes + 2 * plane + base, m.planes + 3 * plane + base, has, rp, hit);
}

// the cell of a segment inside [C, 24, bins + 1] (at most 254 * 24 * 65 cells), or -1: area > 0, code c < C
__device__ __forceinline__ int seg_cell(int c, int C, int area, int hit, int bins) {
  if (area <= 0 || c >= C) return -1;
  const int s = comp_size_bucket(area);
  const int k = (int)((long)bins * hit / area);                              // hit <= area: k <= bins, k == bins iff hit == area
  return (c * COMP_SIZE_BUCKETS + s) * (bins + 1) + k;
}

// grid (cdiv(H * W, 256), B): every root pixel of either side adds its segment; counts int64 [n_slots, 2, C, 24, bins + 1]
__global__ __launch_bounds__(256) void eval_segments_count_kernel(SegMaps m, EvalLabel ev, EvalSlots es, int bins) {
  const long HW = (long)m.H * m.W, i = (long)blockIdx.x * 256 + threadIdx.x, base = blockIdx.y * HW, plane = (long)m.B * HW;
  const int C = ev.C, b = blockIdx.y;
  const long side = (long)C * COMP_SIZE_BUCKETS * (bins + 1);
  unsigned long long* slot = ev.counts + (long)es.s[b] * 2 * side;
  int c0 = -1, c1 = -1;
  if (i < HW) {
    if (m.root_label[base + i] == (int)i) {
      const int a = m.planes[base + i];
      if (a > 0) c0 = seg_cell(label_code(ev, ev.lut, b, m.W, (int)i), C, a, m.planes[plane + base + i], bins);
    }
    if (m.root_pred[base + i] == (int)i) {
      const int a = m.planes[2 * plane + base + i];
      if (a > 0) c1 = seg_cell(min((int)m.pred[base + i], C), C, a, m.planes[3 * plane + base + i], bins);
    }
  }
  seg_count_add(slot, c0);
  seg_count_add(slot + side, c1);
}

extern "C" int mmsa_eval_segments(const unsigned char* pred, const unsigned char* label, int B, int H, int W, int Hl, int Wl, const unsigned char* lut, int C,
                                  const int* ymap, const int* xmap, const int* slots /* HOST [B] */, int n_slots, const int* root_pred, const int* root_label,
                                  int bins, int* scratch, int64_t* counts, hipStream_t stream) {
  const char* name = "eval_segments";
  MMSA_CHECK_ARG(pred && root_pred && root_label && scratch, "%s: pred, root_pred, root_label and scratch are required", name);
  EvalSlots es;
  int rc = eval_check(name, label, B, H, W, Hl, Wl, lut, C, ymap, xmap, slots, n_slots, counts, es, 254, "a uint8 class map");
  if (rc) return rc;
  MMSA_CHECK_ARG(bins >= 1 && bins <= COMP_MAX_BINS, "%s: bins = %d; 1..%d coverage bins are supported", name, bins, COMP_MAX_BINS);
  rc = comp_zero(name, scratch, (size_t)4 * B * H * W * sizeof(int), stream);
  if (rc) return rc;
  const SegMaps m = {pred, root_pred, root_label, scratch, H, W, B};
  const EvalLabel ev = {label, lut, ymap, xmap, (unsigned long long*)counts, Hl, Wl, C};
  const dim3 grid((unsigned)cdiv((long)H * W, 256l), B);
  hipLaunchKernelGGL(eval_segments_area_kernel, grid, dim3(256), 0, stream, m, ev);
  hipLaunchKernelGGL(eval_segments_count_kernel, grid, dim3(256), 0, stream, m, ev, es, bins);
  MMSA_CHECK_LAUNCH("eval_segments");
  return MMSA_OK;
}
