// Run-length tables on device: the runs of a map in row-major or column-major order (mmsa_run_lengths_u8 / _i32) and their inverse (mmsa_run_decode_i32).
// Integers only: the same bytes run after run.
//
// The quantities.  Of image b of a map m [B, H, W], flat_b = m[b].ravel() (order 0, rows) or m[b].T.ravel() (order 1, columns: COCO's
// mask order).  A HEAD is index 0 and every i > 0 with flat_b[i] != flat_b[i - 1]: runs continue across line ends, and a map of one value is ONE run.
// count[b] = the heads of image b, also where it exceeds capacity; starts[b, j] = the flat index of the j-th head in ascending order, values[b, j] = flat_b
// there, for j < min(count[b], capacity); the rows behind them are NOT written.  Lengths are not stored: length[j] = (starts[j + 1] or H * W) - starts[j].
//
// The launches.  The heads are numbered by the stream compaction of csrc/compact.h (count, scan, rank: three launches); its blocks are the SCAN UNITS of
// RUNS_BLOCK consecutive flat indices.  The rank launch is the write pass: starts / values of head j for j < capacity, and the last unit of an image writes
// count[b].
// Row order: a lane takes its predecessor from the lane below it; lane 0 of a wave reads it from memory -- the pixel before the unit's first included,
//   across the line end.
// Column order: the map is first transposed into the caller's scratch, behind the unit counts (a 64 x 64 tile per workgroup through padded LDS: row reads
//   and row writes), and the row-order launches run on the copy: the flat index of the transposed map IS the column-major index.  A form that walked a
//   staged tile with a lane per column, one (column, row tile) piece per scan unit, was built and timed first: on two 1024 x 1024 maps / the 1080 x 1920
//   frame it took 37 / 52 us where this takes 26 / 26 us and the row order 23 / 23 us -- a frame has 32 times as many such pieces as blocks, and the
//   single-workgroup scan walks them all (profiles/run_length.txt).
// Decode: a lane per pixel finds the last start <= its flat index by a binary search over min(count[b], capacity) starts, 32 steps at the most.
#include "common.h"
#include "comp_shared.h"    // comp_check_size
#include "compact.h"

#ifndef RUNS_BLOCK
#define RUNS_BLOCK 2048                       // pixels per unit (and workgroup) of the row order; a multiple of 256
#endif
#define RUNS_TILE 64                          // rows and columns of a tile of the transpose: a wave is a row of it
#define RUNS_PER_LANE (RUNS_BLOCK / 256)

COMPACT_CHECK_BLOCK(RUNS_BLOCK);
static_assert(RUNS_TILE == 64, "a wave is one row of a tile");

// ---- row order.  grid (cdiv(H * W, RUNS_BLOCK), B)

// pixel i of the image at `img` (every lane of the wave calls it together): whether it is a head, and its value
template <typename T>
__device__ __forceinline__ bool runs_row_head(const T* __restrict__ img, long HW, long i, int lane, int& v) {
  v = i < HW ? (int)img[i] : 0;
  int prev = __shfl_up(v, 1);
  if (lane == 0 && i > 0 && i < HW) prev = (int)img[i - 1];                    // the pixel before the wave's first, from memory
  return i < HW && (i == 0 || v != prev);
}

template <typename T>
__global__ __launch_bounds__(256) void runs_row_count_kernel(const T* __restrict__ src, long HW, int nunit, int* __restrict__ scratch) {
  const T* img = src + blockIdx.y * HW;
  int v;
  compact_block_count<RUNS_PER_LANE>([&](int, long i) { return runs_row_head(img, HW, i, threadIdx.x & 63, v); }, nunit, scratch);
}

template <typename T>
__global__ __launch_bounds__(256) void runs_row_write_kernel(const T* __restrict__ src, long HW, int nunit, const int* __restrict__ scratch, int capacity,
                                                             int* __restrict__ count, int* __restrict__ starts, int* __restrict__ values) {
  const T* img = src + blockIdx.y * HW;
  const int lane = threadIdx.x & 63, b = blockIdx.y;
  int v[RUNS_PER_LANE], rank[RUNS_PER_LANE], total;
  bool head[RUNS_PER_LANE];
#pragma unroll
  for (int k = 0; k < RUNS_PER_LANE; ++k) head[k] = runs_row_head(img, HW, compact_index<RUNS_PER_LANE>(k), lane, v[k]);
  compact_block_rank<RUNS_PER_LANE>(head, rank, total);
  const int off = scratch[(long)b * nunit + blockIdx.x];
#pragma unroll
  for (int k = 0; k < RUNS_PER_LANE; ++k) {
    const int j = off + rank[k];
    if (head[k] && j < capacity) {
      starts[(long)b * capacity + j] = (int)compact_index<RUNS_PER_LANE>(k);
      values[(long)b * capacity + j] = v[k];
    }
  }
  if ((int)blockIdx.x == nunit - 1 && threadIdx.x == 0) count[b] = off + total;
}

// ---- column order: the map transposed, then the row order.  grid (tiles across * tiles down, B), 256 lanes: lane (c = t & 63, q = t >> 6)

// dst [B, W, H] = src [B, H, W] transposed, a tile of RUNS_TILE x RUNS_TILE pixels per workgroup through LDS: a wave reads 64 consecutive pixels of a source
// row and writes 64 consecutive pixels of a destination row.  The write phase reads a COLUMN of the tile, so a tile row is padded by one word: lane c reads
// word c * 65 + r, 32 lanes on 32 banks.
template <typename T>
__global__ __launch_bounds__(256) void runs_transpose_kernel(const T* __restrict__ src, int H, int W, int nty, T* __restrict__ dst) {
  __shared__ int tile[RUNS_TILE][RUNS_TILE + 1];
  const int tx = blockIdx.x / nty, ty = blockIdx.x - tx * nty, x0 = tx * RUNS_TILE, y0 = ty * RUNS_TILE;
  const int c = threadIdx.x & 63, q = threadIdx.x >> 6;
  const long base = (long)blockIdx.y * H * W;
  for (int r = q; r < RUNS_TILE; r += 4)
    if (y0 + r < H && x0 + c < W) tile[r][c] = (int)src[base + (long)(y0 + r) * W + x0 + c];
  __syncthreads();
  for (int r = q; r < RUNS_TILE; r += 4)                                       // destination row x0 + r, columns y0 + c: the pixels the first loop stored
    if (x0 + r < W && y0 + c < H) dst[base + (long)(x0 + r) * H + y0 + c] = (T)tile[c][r];
}

template <typename T>
static int runs_launch(const char* name, const T* src, int B, int H, int W, int order, int capacity, int* count, int* starts, int* values, int* scratch,
                       hipStream_t stream) {
  MMSA_CHECK_ARG(src && count && starts && values && scratch, "%s: src, count, starts, values and scratch are required", name);
  const int rc = comp_check_size(name, B, H, W);
  if (rc) return rc;
  MMSA_CHECK_ARG(order == 0 || order == 1, "%s: order = %d; 0 (row-major runs) or 1 (column-major runs) is expected", name, order);
  MMSA_CHECK_ARG(capacity >= 1 && (long)B * capacity < (1l << 31), "%s: capacity = %d runs per image; at least 1, and B * capacity below 2^31, is expected", name,
                 capacity);
  MMSA_CHECK_ARG((const void*)src != (const void*)scratch && starts != scratch && values != scratch && count != scratch && starts != values,
                 "%s: src, starts, values, count and scratch are separate buffers", name);
  const long HW = (long)H * W;
  const int nunit = cdiv(HW, (long)RUNS_BLOCK);
  if (order == 1) {                                                            // the transposed map lies behind the unit counts
    T* flipped = (T*)(scratch + (long)B * nunit);
    const int nty = cdiv(H, RUNS_TILE), ntx = cdiv(W, RUNS_TILE);              // ntx * nty <= H * W
    hipLaunchKernelGGL(runs_transpose_kernel<T>, dim3((unsigned)ntx * nty, B), dim3(256), 0, stream, src, H, W, nty, flipped);
    src = flipped;
  }
  hipLaunchKernelGGL(runs_row_count_kernel<T>, dim3((unsigned)nunit, B), dim3(256), 0, stream, src, HW, nunit, scratch);
  compact_scan(scratch, B, nunit, stream);
  hipLaunchKernelGGL(runs_row_write_kernel<T>, dim3((unsigned)nunit, B), dim3(256), 0, stream, src, HW, nunit, (const int*)scratch, capacity, count, starts,
                     values);
  MMSA_CHECK_LAUNCH(name);
  return MMSA_OK;
}

extern "C" int mmsa_run_lengths_u8(const unsigned char* src, int B, int H, int W, int order, int capacity, int* count, int* starts, int* values, int* scratch,
                                   hipStream_t stream) {
  return runs_launch("run_lengths_u8", src, B, H, W, order, capacity, count, starts, values, scratch, stream);
}

extern "C" int mmsa_run_lengths_i32(const int* src, int B, int H, int W, int order, int capacity, int* count, int* starts, int* values, int* scratch,
                                    hipStream_t stream) {
  MMSA_CHECK_ARG(src != starts && src != values && src != count, "run_lengths_i32: src, starts, values and count are separate buffers");
  return runs_launch("run_lengths_i32", src, B, H, W, order, capacity, count, starts, values, scratch, stream);
}

// the constants this library was built with, for the caller's scratch (mmsa/evaluate.py compares them with its own): 0 = the pixels per scan unit, 1 = the
// tile edge of the column order's transpose, 2 = the lanes of the scan workgroup, 3 = the unit counts one trip of the scan takes; -1 otherwise
extern "C" int mmsa_run_lengths_block(int what) {
  return what == 0 ? RUNS_BLOCK : what == 1 ? RUNS_TILE : what == 2 ? COMPACT_SCAN_LANES : what == 3 ? COMPACT_SCAN_TRIP : -1;
}

// n = B * H * W pixels, a lane each
__global__ __launch_bounds__(256) void runs_decode_kernel(const int* __restrict__ count, const int* __restrict__ starts, const int* __restrict__ values, long n,
                                                          int H, int W, int order, int capacity, int fill, int* __restrict__ out) {
  const long p = (long)blockIdx.x * 256 + threadIdx.x;
  if (p >= n) return;
  const int HW = H * W, b = (int)(p / HW), i = (int)(p - (long)b * HW);
  int f = i;
  if (order) {
    const int y = i / W, x = i - y * W;
    f = x * H + y;
  }
  const int total = count[b], kept = min(max(total, 0), capacity);
  const int* s = starts + (long)b * capacity;
  int lo = 0, hi = kept;                                                       // the first row with starts > f lies in [lo, hi]
  for (int step = 0; step < 32 && lo < hi; ++step) {                           // kept < 2^31: 31 halvings empty the interval
    const int mid = lo + ((hi - lo) >> 1);
    if (s[mid] <= f) lo = mid + 1; else hi = mid;
  }
  const int j = lo - 1;                                                        // the last row with starts <= f; -1: none
  // of an overflowed table the last kept run has no row behind it to end it: its head pixel is known, and from there on the image is `fill`
  const bool known = j >= 0 && (j < kept - 1 || total <= capacity || s[j] == f);
  out[p] = known ? values[(long)b * capacity + j] : fill;
}

extern "C" int mmsa_run_decode_i32(const int* count, const int* starts, const int* values, int B, int H, int W, int order, int capacity, int fill, int* out,
                                   hipStream_t stream) {
  const char* name = "run_decode_i32";
  MMSA_CHECK_ARG(count && starts && values && out, "%s: count, starts, values and out are required", name);
  const int rc = comp_check_size(name, B, H, W);
  if (rc) return rc;
  MMSA_CHECK_ARG(order == 0 || order == 1, "%s: order = %d; 0 (row-major runs) or 1 (column-major runs) is expected", name, order);
  MMSA_CHECK_ARG(capacity >= 1 && (long)B * capacity < (1l << 31), "%s: capacity = %d runs per image; at least 1, and B * capacity below 2^31, is expected", name,
                 capacity);
  MMSA_CHECK_ARG(out != starts && out != values && out != count, "%s: out is a buffer of its own", name);
  const long n = (long)B * H * W;
  hipLaunchKernelGGL(runs_decode_kernel, dim3((unsigned)cdiv(n, 256l)), dim3(256), 0, stream, count, starts, values, n, H, W, order, capacity, fill, out);
  MMSA_CHECK_LAUNCH(name);
  return MMSA_OK;
}
