// Euclidean boundary evaluation on device: the exact squared distance of every pixel of a code map to the nearest pixel OF THE IMAGE that holds another code
// (mmsa_boundary_distance_u8), the confusion counts split by "within a Euclidean radius of a label / prediction boundary" (mmsa_eval_boundary_d2: the four
// zones of csrc/boundary.hip with a threshold on two such maps in the place of its window test) and the displacement histogram of the two contours
// (mmsa_eval_boundary_displacement: what the boundary F-score at every tolerance and the Hausdorff percentiles are formed from, in float64 on the host).
// Integers only: the same bytes run after run.
//
// The quantity.  For a code map M (one byte per pixel after the LUT and the nearest-neighbour tables; the kernel compares bytes and knows nothing of classes):
//   D2(p) = min over pixels q of the image with M(q) != M(p) of (qy - py)^2 + (qx - px)^2           (>= 1; no such q: FAR)
//   border = 1: additionally D2(p) <= db^2, db = min(y, x, H - 1 - y, W - 1 - x) + 1, the distance to the first pixel outside the image
//   d2[p] = D2(p) where D2(p) <= cap^2, else 65535 (DIST_FAR), uint16; cap <= 255, so cap^2 <= 65025 fits.
// It is separable.  With r(x, y) the distance along row y from x to the nearest pixel of that row whose code differs from M(x, y):
//   D2(p) = min over rows y' of (y' - py)^2 + g^2,  g = r(px, y') if M(px, y') == M(p) else 0
// (a pixel of another code in row y' nearest to column px is either (px, y') itself or the end of the run of M(p) that holds (px, y')).
//
// Two launches, no dependence between workgroups inside either, every loop bounded by the row length, by cap or by the image height:
//   row pass     the row pass of csrc/row_scan.h with a code change as the marked index: a lane finds the first and the last change of its piece, row_scan
//                gives it the last change before and the first change after the piece, and the lane walks its piece again run by run and writes, per
//                pixel, the code and r - 1 saturated at 255 (r >= 256 can matter at no cap) as ONE uint16 into the scratch plane [B, H, W].
//   column pass  a lane per pixel, a wave on 64 consecutive x: from the pixel's own row outward, dy = 1, 2, ... while dy <= cap and dy^2 < best, both rows at
//                distance dy: one coalesced 128-byte read of the scratch plane per wave and row.  Pixels next to a contour stop after a step or two; a pixel
//                deep inside a region pays up to 2 cap reads.
// The count passes are pointwise: a lane per pixel reads pred, the label byte (LUT, tables and slots as in mmsa_eval_confusion_u8) and the two uint16 distances,
// and adds into the workgroup's private LDS histogram of csrc/eval_hist.h.  (The walk of csrc/eval_walk.h hands its policy the packed bytes of four pixels
// but not their position, which a pass that reads two more planes needs: these passes walk by themselves.)
#include "common.h"
#include "eval_hist.h"
#include "code_map.h"
#include "row_scan.h"

#define DIST_FAR 65535
#define DIST_MAX_CAP 255
#define DIST_RUN_SAT 255          // stored run byte: r - 1, or 255 for r >= 256
#define DIST_BIG (1 << 20)        // above every cap^2, small enough that two of them add without overflow
#define DIST_LDS_BYTES 65536
#define DIST_CHUNK 8192           // pixels per workgroup of the count passes: 32 per lane, as EVAL_CHUNK

// The largest C of the zone counts: ONE zone's (C + 1)^2 uint32 histogram and the LUT in 64 KiB of LDS; the zones are split over gridDim.z into 2 or 4 groups
// where four do not fit (as csrc/boundary.hip and csrc/selective.hip split theirs).
#define DIST_MAX_CLASSES MMSA_EVAL_MAX_CLASSES
// The displacement histogram [2 sides, C + 1, cap + 2] uint32 of a workgroup: both sides where they fit, else one side per gridDim.z; one side must fit.
//   25 classes at cap 255: 2 * 26 * 257 * 4 = 53 456 B, one group;  82 classes at cap 64: 2 * 83 * 66 * 4 = 43 824 B, one group.
#define DIST_MAX_SIDE_CELLS ((DIST_LDS_BYTES - 256) / 4)
static_assert(2 * 26 * 257 * 4 + 256 <= DIST_LDS_BYTES && 2 * 83 * 66 * 4 + 256 <= DIST_LDS_BYTES, "the required sizes of the displacement histogram");

// rows = B * H; the workgroup blockIdx.x owns one row
__global__ __launch_bounds__(256) void distance_rows_kernel(CodeSrc s, unsigned short* __restrict__ plane) {
  __shared__ int wave_last[4], wave_first[4];
  const long row = blockIdx.x;
  const int W = s.W;
  const int b = (int)(row / s.H), y = (int)(row - (long)b * s.H);
  const unsigned char* __restrict__ srow = code_row(s, b, y);
  unsigned short* __restrict__ prow = plane + row * W;
  int x0, x1, before, after;
  row_piece(W, x0, x1);

  // 1. the first and the last change of this lane's piece; a change at x: code(x) != code(x - 1), x >= 1
  int fc = ROW_NONE, lc = -1;
  const int left = (x0 > 0 && x0 < x1) ? code_at(s, srow, x0 - 1) : -1;
  {
    int prev = left;
    for (int x = x0; x < x1; ++x) {
      const int c = code_at(s, srow, x);
      if (prev >= 0 && c != prev) {
        fc = min(fc, x);
        lc = x;
      }
      prev = c;
    }
  }
  // 2. the last change in front of the piece, the first change behind it (every lane of the workgroup is here: a row is a workgroup's)
  row_scan(fc, lc, wave_last, wave_first, before, after);
  if (x0 >= x1) return;

  // 3. run by run: the run [a, x) of code `prev` starts behind the change `st` (-1: it reaches the row's left end) and ends at the change `en`
  int a = x0, prev = code_at(s, srow, x0);
  int st = (left >= 0 && left != prev) ? x0 : before;
  for (int x = x0 + 1; x <= x1; ++x) {
    int c = -1, en = ROW_NONE;
    if (x < x1) {
      c = code_at(s, srow, x);
      if (c == prev) continue;
      en = x;
    } else {
      en = after;
    }
    for (int q = a; q < x; ++q) {                                            // every pixel of the piece is written once
      int r = ROW_NONE;
      if (st >= 0) r = q - st + 1;                                           // the pixel st - 1 holds another code
      if (en != ROW_NONE) r = min(r, en - q);                                    // and so does the pixel en
      const int rb = r > DIST_RUN_SAT ? DIST_RUN_SAT : r - 1;
      prow[q] = (unsigned short)(prev | (rb << 8));
    }
    st = x;
    a = x;
    prev = c;
  }
}

__device__ __forceinline__ int dist_run2(int v) {      // g^2 of a scratch word's run byte
  const int rb = v >> 8;
  return rb == DIST_RUN_SAT ? DIST_BIG : (rb + 1) * (rb + 1);
}

// the grid of col_tile (csrc/row_scan.h)
__global__ __launch_bounds__(256) void distance_cols_kernel(const unsigned short* __restrict__ plane, int H, int W, int tiles_x, int groups_y, int cap,
                                                            int border, unsigned short* __restrict__ d2) {
  int b, y, x;
  if (!col_tile(H, W, tiles_x, groups_y, b, y, x)) return;
  const unsigned short* __restrict__ col = plane + (long)b * H * W + x;
  const int own = col[(long)y * W], c = own & 255, limit = cap * cap;
  int best = min(limit + 1, dist_run2(own));
  if (border) {
    const int db = min(min(min(y, x), min(H - 1 - y, W - 1 - x)) + 1, DIST_MAX_CAP + 1);
    best = min(best, db * db);
  }
  const int reach = min(cap, max(y, H - 1 - y));                            // no row of the image lies further
  for (int dy = 1; dy <= reach && dy * dy < best; ++dy) {
    const int d = dy * dy;
    if (y - dy >= 0) {
      const int v = col[(long)(y - dy) * W];
      best = min(best, (v & 255) == c ? d + dist_run2(v) : d);
    }
    if (y + dy < H) {
      const int v = col[(long)(y + dy) * W];
      best = min(best, (v & 255) == c ? d + dist_run2(v) : d);
    }
  }
  d2[((long)b * H + y) * W + x] = (unsigned short)(best <= limit ? best : DIST_FAR);
}

extern "C" int mmsa_boundary_distance_u8(const unsigned char* src, int B, int Hs, int Ws, const unsigned char* lut, const int* ymap, const int* xmap, int H,
                                         int W, int cap, int border, unsigned short* scratch, unsigned short* d2, hipStream_t stream) {
  const char* name = "boundary_distance_u8";
  MMSA_CHECK_ARG(src && scratch && d2, "%s: src, scratch and d2 are required", name);
  MMSA_CHECK_ARG(scratch != d2, "%s: scratch and d2 are two planes", name);
  MMSA_CHECK_ARG(B > 0 && H > 0 && W > 0 && (long)H * W < (1l << 31), "%s: bad map size", name);
  int rc = code_src_check(name, "bad map size", Hs, Ws, ymap, xmap, H, W);
  if (rc) return rc;
  MMSA_CHECK_ARG(cap >= 1 && cap <= DIST_MAX_CAP, "%s: cap = %d; 1..%d are supported (cap^2 must fit the uint16 map below 65535)", name, cap, DIST_MAX_CAP);
  MMSA_CHECK_ARG(border == 0 || border == 1, "%s: border = %d; 0 (pixels outside the image do not exist) or 1 (the image border is a boundary)", name, border);
  RowColGrid g;
  rc = row_col_grid(name, B, H, W, g);
  if (rc) return rc;
  const CodeSrc s = {src, lut, ymap, xmap, Hs, Ws, H, W};
  hipLaunchKernelGGL(distance_rows_kernel, dim3((unsigned)g.rows), dim3(256), 0, stream, s, scratch);
  hipLaunchKernelGGL(distance_cols_kernel, dim3((unsigned)g.blocks), dim3(256), 0, stream, scratch, H, W, g.tiles_x, g.groups_y, cap, border, d2);
  MMSA_CHECK_LAUNCH("boundary_distance_u8");
  return MMSA_OK;
}

// ---- the pointwise count passes over (pred, label, d2_pred, d2_label)
struct DistMaps {
  const unsigned char* pred;        // [B, H, W]
  const unsigned short* d2p;        // [B, H, W]
  const unsigned short* d2l;
  int H, W;
};

// grid (chunks of DIST_CHUNK pixels, B, zone groups): zone = 2 * (d2_label <= t) + (d2_pred <= t)
__global__ __launch_bounds__(256) void eval_boundary_d2_kernel(DistMaps m, EvalLabel ev, EvalSlots es, int t, int zn) {
  extern __shared__ unsigned dist_lds[];
  const int C = ev.C, nb = (C + 1) * (C + 1);
  unsigned* hist = dist_lds;
  unsigned char* lut_s = (unsigned char*)(hist + zn * nb);
  eval_hist_init(hist, lut_s, ev.lut, zn * nb);
  const int b = blockIdx.y, z0 = (int)blockIdx.z * zn;
  const long HW = (long)m.H * m.W, start = (long)blockIdx.x * DIST_CHUNK, base = b * HW;
  for (int k = 0; k < DIST_CHUNK; k += 256) {                                // every lane makes every trip (eval_hist_add votes across the wave)
    const long i = start + k + threadIdx.x;
    int bin = -1;
    if (i < HW) {
      const int l = label_code(ev, lut_s, b, m.W, (int)i);
      if (l != MMSA_EVAL_IGNORE) {
        const int z = 2 * (int)((int)m.d2l[base + i] <= t) + (int)((int)m.d2p[base + i] <= t) - z0;
        if ((unsigned)z < (unsigned)zn) bin = z * nb + l * (C + 1) + min((int)m.pred[base + i], C);
      }
    }
    eval_hist_add(hist, bin, 1u);
  }
  eval_hist_flush(hist, ev.counts + ((long)es.s[b] * 4 + z0) * nb, zn * nb);
}

static inline int dist_check_maps(const char* name, const unsigned char* pred, const unsigned short* d2_pred, const unsigned short* d2_label) {
  MMSA_CHECK_ARG(pred && d2_pred && d2_label, "%s: pred, d2_pred and d2_label are required", name);
  return MMSA_OK;
}

extern "C" int mmsa_eval_boundary_d2(const unsigned char* pred, const unsigned char* label, int B, int H, int W, int Hl, int Wl, const unsigned char* lut, int C,
                                     const int* ymap, const int* xmap, const int* slots /* HOST [B] */, int n_slots, const unsigned short* d2_pred,
                                     const unsigned short* d2_label, int t, int64_t* counts, hipStream_t stream) {
  const char* name = "eval_boundary_d2";
  int rc = dist_check_maps(name, pred, d2_pred, d2_label);
  if (rc) return rc;
  EvalSlots es;
  rc = eval_check(name, label, B, H, W, Hl, Wl, lut, C, ymap, xmap, slots, n_slots, counts, es, DIST_MAX_CLASSES,
                  "one zone's (C + 1)^2 uint32 histogram must fit 64 KiB of LDS");
  if (rc) return rc;
  MMSA_CHECK_ARG(t >= 1 && t <= DIST_MAX_CAP * DIST_MAX_CAP, "%s: t = %d; a squared radius in 1..%d is expected", name, t, DIST_MAX_CAP * DIST_MAX_CAP);
  const int nb = (C + 1) * (C + 1);
  int groups = 1;
  while (groups < 4 && (size_t)(4 / groups) * nb * 4 + 256 > DIST_LDS_BYTES) groups *= 2;      // C <= DIST_MAX_CLASSES: four groups always fit
  const int zn = 4 / groups;
  const DistMaps m = {pred, d2_pred, d2_label, H, W};
  const EvalLabel ev = {label, lut, ymap, xmap, (unsigned long long*)counts, Hl, Wl, C};
  hipLaunchKernelGGL(eval_boundary_d2_kernel, dim3((unsigned)cdiv((long)H * W, (long)DIST_CHUNK), B, groups), dim3(256), (size_t)zn * nb * 4 + 256, stream, m,
                     ev, es, t, zn);
  MMSA_CHECK_LAUNCH("eval_boundary_d2");
  return MMSA_OK;
}

// the smallest k >= 1 with k^2 >= d2 (1 <= d2 <= 65025), cap + 1 for DIST_FAR: a float square root corrected by integer compares
__device__ __forceinline__ int dist_bin(int d2, int cap) {
  if (d2 == DIST_FAR) return cap + 1;
  int k = (int)sqrtf((float)d2);
  k += (int)(k * k < d2);
  k += (int)(k * k < d2);
  k -= (int)(k > 1 && (k - 1) * (k - 1) >= d2);
  return min(max(k, 1), cap + 1);
}

// grid (chunks, B, side groups); hist_out int64 [n_slots, 2, C + 1, cap + 2]; side 0: label-boundary pixels by their distance to the prediction's contour,
// side 1: prediction-boundary pixels by their distance to the label's
__global__ __launch_bounds__(256) void eval_boundary_displacement_kernel(DistMaps m, EvalLabel ev, EvalSlots es, int cap, int sn) {
  extern __shared__ unsigned dist_lds[];
  const int C = ev.C, nk = cap + 2, ns = (C + 1) * nk;
  unsigned* hist = dist_lds;
  unsigned char* lut_s = (unsigned char*)(hist + sn * ns);
  eval_hist_init(hist, lut_s, ev.lut, sn * ns);
  const int b = blockIdx.y, s0 = (int)blockIdx.z * sn;
  const long HW = (long)m.H * m.W, start = (long)blockIdx.x * DIST_CHUNK, base = b * HW;
  for (int k = 0; k < DIST_CHUNK; k += 256) {
    const long i = start + k + threadIdx.x;
    if (i >= HW) continue;
    const int dl = m.d2l[base + i], dp = m.d2p[base + i];
    if (dl > 2 && dp > 2) continue;                                          // most of a frame: on neither contour
    const int l = label_code(ev, lut_s, b, m.W, (int)i);
    if (l == MMSA_EVAL_IGNORE) continue;
    if (dl <= 2 && s0 == 0) atomicAdd(&hist[l * nk + dist_bin(dp, cap)], 1u);
    if (dp <= 2 && s0 + sn == 2) atomicAdd(&hist[(1 - s0) * ns + min((int)m.pred[base + i], C) * nk + dist_bin(dl, cap)], 1u);
  }
  eval_hist_flush(hist, ev.counts + ((long)es.s[b] * 2 + s0) * ns, sn * ns);
}

extern "C" int mmsa_eval_boundary_displacement(const unsigned char* pred, const unsigned char* label, int B, int H, int W, int Hl, int Wl,
                                               const unsigned char* lut, int C, const int* ymap, const int* xmap, const int* slots /* HOST [B] */, int n_slots,
                                               const unsigned short* d2_pred, const unsigned short* d2_label, int cap, int64_t* hist, hipStream_t stream) {
  const char* name = "eval_boundary_displacement";
  int rc = dist_check_maps(name, pred, d2_pred, d2_label);
  if (rc) return rc;
  EvalSlots es;
  rc = eval_check(name, label, B, H, W, Hl, Wl, lut, C, ymap, xmap, slots, n_slots, hist, es, 254, "a uint8 class map");
  if (rc) return rc;
  MMSA_CHECK_ARG(cap >= 1 && cap <= DIST_MAX_CAP, "%s: cap = %d; 1..%d are supported", name, cap, DIST_MAX_CAP);
  const int ns = (C + 1) * (cap + 2);
  MMSA_CHECK_ARG(ns <= DIST_MAX_SIDE_CELLS,
                 "%s: %d classes at cap %d: (C + 1) * (cap + 2) = %d cells per side; at most %d are supported (one side's uint32 histogram must fit 64 KiB of LDS)",
                 name, C, cap, ns, DIST_MAX_SIDE_CELLS);
  const int groups = (size_t)2 * ns * 4 + 256 <= DIST_LDS_BYTES ? 1 : 2, sn = 2 / groups;
  const DistMaps m = {pred, d2_pred, d2_label, H, W};
  const EvalLabel ev = {label, lut, ymap, xmap, (unsigned long long*)hist, Hl, Wl, C};
  hipLaunchKernelGGL(eval_boundary_displacement_kernel, dim3((unsigned)cdiv((long)H * W, (long)DIST_CHUNK), B, groups), dim3(256), (size_t)sn * ns * 4 + 256,
                     stream, m, ev, es, cap, sn);
  MMSA_CHECK_LAUNCH("eval_boundary_displacement");
  return MMSA_OK;
}
