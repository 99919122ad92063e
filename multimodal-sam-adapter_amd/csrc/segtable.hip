// The segment table on device: dense segment ids and one record per segment (mmsa_segment_table), and the class map with chosen segments painted over
// (mmsa_select_segments_u8).  Integers only: the same bytes run after run.
//
// The quantities.  Code map and roots are csrc/components.hip's.  A component of image b is LISTED iff its area >= min_area and its code
// is below `void_from` (C: the classes only; 256: every code).  The listed segments of an image are numbered 0 .. n_b - 1 in ascending order of their root
// index -- the raster order of their first pixel -- so the numbering is canonical.  count[b] = n_b; ids[b, y, x] = the number of the pixel's segment, -1 where
// it is not listed; records[b, k] = ROOT, CLASS, AREA, X0, Y0, X1, Y1, SUM_X, SUM_Y, SUM_Q for k < min(n_b, capacity), zero from there on.
//
// The launches.  The listed roots are numbered by the stream compaction of csrc/compact.h (count, scan, rank: three launches, blocks of SEGTAB_BLOCK pixels)
// with flag(i) = root[i] == i && listed.
//   id pass      the rank launch: it writes ids at the root pixels (-1 at a root that is not listed), the row's ROOT, CLASS, X0 = X1 = x, Y0 = Y1 = y for
//                id < capacity, and the last block of an image writes count[b].
//   accumulate   a lane per pixel: id = ids[root] (the root clamped into the plane), written to ids[i]; for 0 <= id < capacity the row takes 1, x, y, q and the
//                min / max of x and the max of y by 64-bit atomics.  A road of half a frame is ONE row: a wave first reduces its lanes per distinct id in
//                registers (the form of comp_wave_add), SEGTAB_WAVE_ROUNDS = 8 rounds at the most; what is pending after them goes lane by lane.  A wave holds
//                64 CONSECUTIVE pixels, so a round needs two register reductions only: one packed sum (the lanes, their lane numbers, their rows below the
//                wave's first row: from these n, SUM_Y and -- through the sum of the linear indices -- SUM_X) and the sum of q; Y1 is the row of the last
//                member lane, and X0 / X1 are the columns of the first / last member lane where the members lie in one row (two more reductions otherwise).
//                What binds the pass is the NUMBER of atomic instructions a wave issues, not their addresses, so round r parks its seven terms in lanes
//                8 r .. 8 r + 6 and after the rounds the wave issues ONE add, one min and one max instruction for all of them.  Before that the first id
//                of every wave is merged across the four waves of the workgroup through LDS (one __syncthreads; every wave makes round 0, with or without
//                a pixel, so the barrier is met by all): the lowest wave that holds an id adds for the others.  The lane-by-lane remainder reads X0, X1
//                and Y1 first (an agent-scope relaxed load: they only ever move one way, so a stale value is further from the end, never past it) and
//                issues a min / max only where it would move the value.  The forms, round counts and block sizes that were timed: profiles/segment_table.txt.
// Y0 is the root's row: the root is the component's smallest linear index.  The rows are zeroed with hipMemsetAsync before the id pass.
#include "common.h"
#include "cal_wave.h"       // cal_wave_sum: a wave's sum by data-parallel-primitive moves
#include "code_map.h"
#include "comp_shared.h"
#include "compact.h"
#include "conf_bin.h"

#ifndef SEGTAB_BLOCK
#define SEGTAB_BLOCK 2048                     // pixels per workgroup of the count and id passes (mmsa/evaluate.py SEGTAB_BLOCK); a multiple of 256
#endif
#ifndef SEGTAB_WAVE_ROUNDS
#define SEGTAB_WAVE_ROUNDS 8                  // rounds of the in-wave reduction of the accumulate pass (profiles/segment_table.txt)
#endif
#ifndef SEGTAB_WG_MERGE
#define SEGTAB_WG_MERGE 1                     // 1: the waves of a workgroup merge their first id through LDS before the row atomics (0: the A/B build)
#endif
#ifndef SEGTAB_ACC_THREADS
#define SEGTAB_ACC_THREADS 256                // lanes per workgroup of the accumulate pass
#endif
#define SEGTAB_PER_LANE (SEGTAB_BLOCK / 256)
#define SEGTAB_FIELDS 10
#define SEGTAB_RLX_AGENT __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT
enum { ST_ROOT, ST_CLASS, ST_AREA, ST_X0, ST_Y0, ST_X1, ST_Y1, ST_SUM_X, ST_SUM_Y, ST_SUM_Q };

static_assert(SEGTAB_WAVE_ROUNDS >= 1 && SEGTAB_WAVE_ROUNDS <= 8, "a round's terms take eight lanes of the wave");
static_assert(ST_X1 == 5 && ST_Y1 == 6 && ST_SUM_Y == ST_SUM_X + 1 && ST_SUM_Q == ST_SUM_X + 2, "the lane -> field rule of the accumulate pass");
COMPACT_CHECK_BLOCK(SEGTAB_BLOCK);

struct SegTabMaps {
  CodeSrc s;
  const int* root;                  // [B, H, W]
  const int* area;                  // [B, H, W] as mmsa_component_area writes it, or NULL (min_area == 1)
  int min_area, void_from;
};

// the value in 24-bit fixed point, floor(clamp(v) * 2^24): the product of cal_pixel in csrc/calibrate.hip (exact scaling, truncated: 0 .. 2^24), after the
// clamp of csrc/conf_bin.h -- stated once more here, so that the kernels of calibrate.hip stay as they were built
__device__ __forceinline__ unsigned segtab_q24(float v) { return (unsigned)(conf_clamp(v) * 16777216.0f); }

// pixel i < H * W of image b: 1 = the root of a listed component, -1 = a root that is not listed, 0 = no root; `code` is set for the roots
__device__ __forceinline__ int segtab_flag(const SegTabMaps& m, int b, long base, int i, int& code) {
  if (m.root[base + i] != i) return 0;
  const int y = i / m.s.W;
  code = code_at(m.s, b, y, i - y * m.s.W);
  if (code >= m.void_from) return -1;
  return m.area == nullptr || m.area[base + i] >= m.min_area ? 1 : -1;
}

// grid (cdiv(H * W, SEGTAB_BLOCK), B): the count launch of csrc/compact.h
__global__ __launch_bounds__(256) void segtab_count_kernel(SegTabMaps m, int nblk, int* __restrict__ scratch) {
  const long HW = (long)m.s.H * m.s.W, base = blockIdx.y * HW;
  int code;
  compact_block_count<SEGTAB_PER_LANE>([&](int, long i) { return i < HW && segtab_flag(m, blockIdx.y, base, (int)i, code) > 0; }, nblk, scratch);
}

// grid (cdiv(H * W, SEGTAB_BLOCK), B): the rank launch, with the offsets of the scan
__global__ __launch_bounds__(256) void segtab_ids_kernel(SegTabMaps m, int nblk, const int* __restrict__ scratch, int capacity, int* __restrict__ count,
                                                         int* __restrict__ ids, long long* __restrict__ records) {
  const long HW = (long)m.s.H * m.s.W, base = blockIdx.y * HW;
  const int b = blockIdx.y, W = m.s.W;
  int flag[SEGTAB_PER_LANE], code[SEGTAB_PER_LANE], rank[SEGTAB_PER_LANE], total;
  bool listed[SEGTAB_PER_LANE];
#pragma unroll
  for (int k = 0; k < SEGTAB_PER_LANE; ++k) {
    const long i = compact_index<SEGTAB_PER_LANE>(k);
    code[k] = 0;
    flag[k] = i < HW ? segtab_flag(m, b, base, (int)i, code[k]) : 0;
    listed[k] = flag[k] > 0;
  }
  compact_block_rank<SEGTAB_PER_LANE>(listed, rank, total);
  const int off = scratch[(long)b * nblk + blockIdx.x];
#pragma unroll
  for (int k = 0; k < SEGTAB_PER_LANE; ++k) {
    if (flag[k] == 0) continue;
    const long i = compact_index<SEGTAB_PER_LANE>(k);
    const int id = listed[k] ? off + rank[k] : -1;
    ids[base + i] = id;
    if (id >= 0 && id < capacity) {
      long long* row = records + ((long)b * capacity + id) * SEGTAB_FIELDS;
      const int y = (int)i / W, x = (int)i - y * W;
      row[ST_ROOT] = i;
      row[ST_CLASS] = code[k];
      row[ST_X0] = row[ST_X1] = x;
      row[ST_Y0] = row[ST_Y1] = y;
    }
  }
  if ((int)blockIdx.x == nblk - 1 && threadIdx.x == 0) count[b] = off + total;
}

// one (wave, id) or one lane: n pixels with these sums and extremes join the row
__device__ __forceinline__ void segtab_row_add(unsigned long long* row, unsigned long long n, unsigned long long sx, unsigned long long sy, unsigned long long sq,
                                               unsigned long long xmin, unsigned long long xmax, unsigned long long ymax) {
  atomicAdd(&row[ST_AREA], n);
  if (sx) atomicAdd(&row[ST_SUM_X], sx);
  if (sy) atomicAdd(&row[ST_SUM_Y], sy);
  if (sq) atomicAdd(&row[ST_SUM_Q], sq);
  if (xmin < __hip_atomic_load(&row[ST_X0], SEGTAB_RLX_AGENT)) atomicMin(&row[ST_X0], xmin);      // X0 only falls, X1 and Y1 only rise: a stale value is
  if (xmax > __hip_atomic_load(&row[ST_X1], SEGTAB_RLX_AGENT)) atomicMax(&row[ST_X1], xmax);      // further from the end, and then the atomic decides
  if (ymax > __hip_atomic_load(&row[ST_Y1], SEGTAB_RLX_AGENT)) atomicMax(&row[ST_Y1], ymax);
}

// what one round of one wave adds to one row
struct SegTabPart {
  int id;                           // -1: nothing
  int xmin, xmax, ymax;
  unsigned long long n, sx, sy, sq;
};

// grid (cdiv(H * W, SEGTAB_ACC_THREADS), B): a wave holds 64 consecutive pixels of one image
__global__ __launch_bounds__(SEGTAB_ACC_THREADS) void segtab_accumulate_kernel(const int* __restrict__ root, const float* __restrict__ values, int H, int W,
                                                                               int capacity, int* ids, unsigned long long* records) {
#if SEGTAB_WG_MERGE
  __shared__ SegTabPart part[SEGTAB_ACC_THREADS / 64];
#endif
  const long HW = (long)H * W, i = (long)blockIdx.x * SEGTAB_ACC_THREADS + threadIdx.x, base = blockIdx.y * HW;
  const int lane = threadIdx.x & 63;
  const long i0 = i - lane;                                                    // the wave's first pixel
  const bool has = i < HW;
  int id = -1, x = 0, y = 0;
  unsigned q = 0u;
  if (has) {
    const int r = min(max(root[base + i], 0), (int)HW - 1);                    // a root map from elsewhere cannot send the read outside the plane
    id = ids[base + r];                                                        // written by the id pass: a root pixel
    ids[base + i] = id;                                                        // a root pixel writes what it read
    y = (int)(i / W);
    x = (int)(i - (long)y * W);
    if (values) q = segtab_q24(values[base + i]);
  }
  const int y0 = (int)(i0 / W), dy = has ? y - y0 : 0;                         // 0 <= dy <= 63
  unsigned long long* rows = records + (long)blockIdx.y * capacity * SEGTAB_FIELDS;
  bool pending = has && id >= 0 && id < capacity;                              // an id from elsewhere addresses no row outside the table
  unsigned long long live = __ballot(pending), myval = 0ull;
  int myrow = -1;
  for (int r = 0; r < SEGTAB_WAVE_ROUNDS; ++r) {
    const bool any = live != 0ull;
    if (!any && !(SEGTAB_WG_MERGE && r == 0)) break;                           // with the merge every wave makes round 0: it holds the workgroup's barrier
    const int lead = any ? __ffsll((long long)live) - 1 : 0;
    const int lid = any ? __builtin_amdgcn_readlane(id, lead) : -1;
    const bool same = pending && id == lid;
    const unsigned long long ms = __ballot(same);
    // dy sum < 2^12, lane sum < 2^11, lanes <= 64: 30 bits
    const unsigned long long packed = cal_wave_sum(same ? (unsigned)dy | ((unsigned)lane << 12) | (1u << 23) : 0u);
    const unsigned long long sq = values ? cal_wave_sum(same ? q : 0u) : 0ull;                    // a row of 16 lanes: at most 2^28
    const int last = any ? 63 - __clzll((long long)ms) : 0;
    const int dy_first = __builtin_amdgcn_readlane(dy, lead), dy_last = __builtin_amdgcn_readlane(dy, last);      // rows rise with the lane
    int xmin = __builtin_amdgcn_readlane(x, lead), xmax = __builtin_amdgcn_readlane(x, last);
    if (dy_first != dy_last) {                                                 // the members span rows: their columns are in no order
      xmin = same ? x : 0x7fffffff;
      xmax = same ? x : -1;
#pragma unroll
      for (int d = 1; d < 64; d <<= 1) {
        xmin = min(xmin, __shfl_xor(xmin, d));
        xmax = max(xmax, __shfl_xor(xmax, d));
      }
    }
    const unsigned long long n = packed >> 23, sdy = packed & 0xfffull, sl = (packed >> 12) & 0x7ffull;
    const unsigned long long sy = n * (unsigned long long)y0 + sdy, si = n * (unsigned long long)i0 + sl;
    SegTabPart a = {lid, xmin, xmax, y0 + dy_last, n, si - (unsigned long long)W * sy, sy, sq};
#if SEGTAB_WG_MERGE
    if (r == 0) {                                                              // the first id of every wave: the waves of a workgroup that share it add ONCE
      const int w = threadIdx.x >> 6;
      if (lane == lead) part[w] = a;
      __syncthreads();
      bool first = any;
      for (int k = 0; k < w; ++k) first = first && part[k].id != lid;          // a lower wave with this id adds for this one
      if (first) {
        for (int k = w + 1; k < SEGTAB_ACC_THREADS / 64; ++k) {
          const SegTabPart o = part[k];
          if (o.id != lid) continue;
          a.n += o.n, a.sx += o.sx, a.sy += o.sy, a.sq += o.sq;
          a.xmin = min(a.xmin, o.xmin), a.xmax = max(a.xmax, o.xmax), a.ymax = max(a.ymax, o.ymax);
        }
      } else {
        a.id = -1;
      }
    }
#endif
    if (a.id >= 0 && (lane >> 3) == r) {                                       // the round's seven terms go to lanes 8 r .. 8 r + 6, one each
      myrow = a.id;
      const int f = lane & 7;
      myval = f == 0 ? a.n : f == 1 ? a.sx : f == 2 ? a.sy : f == 3 ? a.sq
            : f == 4 ? (unsigned long long)a.xmin : f == 5 ? (unsigned long long)a.xmax : f == 6 ? (unsigned long long)a.ymax : 0ull;
    }
    pending = pending && !same;
    live &= ~ms;
  }
  if (myrow >= 0) {                                                            // every round's terms at once: ONE add, one min and one max instruction per wave
    const int f = lane & 7;
    unsigned long long* p = rows + (long)myrow * SEGTAB_FIELDS + (f == 0 ? ST_AREA : f < 4 ? ST_SUM_X + f - 1 : f == 4 ? ST_X0 : f);      // 5, 6: ST_X1, ST_Y1
    if (f < 4) {
      if (myval) atomicAdd(p, myval);
    } else if (f == 4) {
      atomicMin(p, myval);
    } else if (f < 7) {
      atomicMax(p, myval);
    }
  }
  if (pending)                                                                 // beyond the rounds: lane by lane
    segtab_row_add(rows + (long)id * SEGTAB_FIELDS, 1ull, (unsigned long long)x, (unsigned long long)y, (unsigned long long)q, (unsigned long long)x,
                   (unsigned long long)x, (unsigned long long)y);
}

extern "C" int mmsa_segment_table(const unsigned char* src, int B, int Hs, int Ws, const unsigned char* lut, const int* ymap, const int* xmap, int H, int W,
                                  const int* root, const int* area, const float* values, int min_area, int void_from, int capacity, int* count, int* ids,
                                  int64_t* records, int* scratch, hipStream_t stream) {
  const char* name = "segment_table";
  MMSA_CHECK_ARG(src && root && count && ids && records && scratch, "%s: src, root, count, ids, records and scratch are required", name);
  int rc = comp_check_size(name, B, H, W);
  if (rc) return rc;
  rc = code_src_check(name, "bad source size", Hs, Ws, ymap, xmap, H, W);
  if (rc) return rc;
  MMSA_CHECK_ARG(root != ids && (const void*)root != (const void*)scratch && ids != scratch, "%s: root, ids and scratch are three buffers", name);
  MMSA_CHECK_ARG(min_area >= 1, "%s: min_area = %d; at least 1 (every component) is expected", name, min_area);
  MMSA_CHECK_ARG(min_area == 1 || area, "%s: min_area = %d needs the area plane of mmsa_component_area", name, min_area);
  MMSA_CHECK_ARG(void_from >= 1 && void_from <= 256, "%s: void_from = %d; the class count C (codes from C on are not listed) or 256 (every code is) is expected",
                 name, void_from);
  MMSA_CHECK_ARG(capacity >= 1 && (long)B * capacity < (1l << 31), "%s: capacity = %d rows per image; at least 1, and B * capacity below 2^31, is expected", name,
                 capacity);
  MMSA_CHECK_ARG(((uintptr_t)values & 3u) == 0, "%s: values must be 4-byte aligned", name);
  rc = comp_zero(name, records, (size_t)B * capacity * SEGTAB_FIELDS * sizeof(int64_t), stream);
  if (rc) return rc;
  const long HW = (long)H * W;
  const int nblk = cdiv(HW, (long)SEGTAB_BLOCK);
  const SegTabMaps m = {{src, lut, ymap, xmap, Hs, Ws, H, W}, root, min_area > 1 ? area : nullptr, min_area, void_from};
  hipLaunchKernelGGL(segtab_count_kernel, dim3((unsigned)nblk, B), dim3(256), 0, stream, m, nblk, scratch);
  compact_scan(scratch, B, nblk, stream);
  hipLaunchKernelGGL(segtab_ids_kernel, dim3((unsigned)nblk, B), dim3(256), 0, stream, m, nblk, (const int*)scratch, capacity, count, ids,
                     (long long*)records);
  hipLaunchKernelGGL(segtab_accumulate_kernel, dim3((unsigned)cdiv(HW, (long)SEGTAB_ACC_THREADS), B), dim3(SEGTAB_ACC_THREADS), 0, stream, root, values, H, W, capacity, ids,
                     (unsigned long long*)records);
  MMSA_CHECK_LAUNCH("segment_table");
  return MMSA_OK;
}

// the pixels per scratch word this library was built with: the caller sizes `scratch` by it (mmsa/evaluate.py compares it with its own constant)
extern "C" int mmsa_segment_table_block(void) { return SEGTAB_BLOCK; }

// n = B * H * W pixels, HW per image; out may be pred
__global__ __launch_bounds__(256) void select_segments_kernel(const unsigned char* pred, const int* __restrict__ ids, const unsigned char* __restrict__ keep, long n,
                                                              int HW, int capacity, int fill, unsigned char* out) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const int id = ids[i];
  const bool drop = id >= 0 && id < capacity && keep[i / HW * capacity + id] == 0;
  out[i] = drop ? (unsigned char)fill : pred[i];
}

extern "C" int mmsa_select_segments_u8(const unsigned char* pred, const int* ids, const unsigned char* keep, int B, int H, int W, int capacity, int fill,
                                       unsigned char* out, hipStream_t stream) {
  const char* name = "select_segments_u8";
  MMSA_CHECK_ARG(pred && ids && keep && out, "%s: pred, ids, keep and out are required", name);
  int rc = comp_check_size(name, B, H, W);
  if (rc) return rc;
  MMSA_CHECK_ARG(capacity >= 1 && (long)B * capacity < (1l << 31), "%s: capacity = %d rows per image; at least 1, and B * capacity below 2^31, is expected", name,
                 capacity);
  MMSA_CHECK_ARG(fill >= 0 && fill <= 255, "%s: fill = %d; a byte is expected", name, fill);
  const long n = (long)B * H * W;
  hipLaunchKernelGGL(select_segments_kernel, dim3((unsigned)cdiv(n, 256l)), dim3(256), 0, stream, pred, ids, keep, n, H * W, capacity, fill, out);
  MMSA_CHECK_LAUNCH("select_segments_u8");
  return MMSA_OK;
}
