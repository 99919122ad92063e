// The frame of the two-launch passes that are separable along rows and columns: csrc/distance.hip (nearest pixel of another code) and csrc/fill.hip
// (nearest source pixel).  Each pass says what MARKS an index of a row (a code change, a source pixel) and keeps its own walks.
//   row pass     a WORKGROUP of 256 lanes per row of an image.  Lane t owns the piece [x0, x1) of ceil(W / 256) consecutive pixels (row_piece), finds
//                the first and the last marked index of it, row_scan hands it the last marked index in front of the piece and the first one behind it,
//                and the lane walks its piece again and writes one uint16 per pixel into a scratch plane [B, H, W].
//   column pass  a lane per pixel, a wave on 64 consecutive x, 4 rows per workgroup (col_tile): the lane walks up and down its column of the plane.
#pragma once
#include "common.h"

#define ROW_NONE 0x7fffffff         // no marked index behind

// the piece [x0, x1) of this lane in a row of W pixels
__device__ __forceinline__ void row_piece(int W, int& x0, int& x1) {
  const int ch = (W + 255) >> 8;
  x0 = min(W, (int)threadIdx.x * ch);
  x1 = min(W, x0 + ch);
}

// first / last = the first and the last marked index of this lane's piece (ROW_NONE / -1: none) -> before = the last marked index in front of the piece
// (-1: none), after = the first one behind it (ROW_NONE: none).  An exclusive prefix maximum / suffix minimum over the lanes: a shuffle scan inside each
// wave, the four waves' own ends through LDS.  Holds the __syncthreads(): every lane of the workgroup calls it, also one with an empty piece (a row is
// a workgroup's).
__device__ __forceinline__ void row_scan(int first, int last, int* wave_last, int* wave_first, int& before, int& after) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  int pm = last, sm = first;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const int up = __shfl_up(pm, o, 64), dn = __shfl_down(sm, o, 64);
    if (lane >= o) pm = max(pm, up);
    if (lane + o < 64) sm = min(sm, dn);
  }
  if (lane == 63) wave_last[wave] = pm;                                      // the wave's last marked index
  if (lane == 0) wave_first[wave] = sm;                                      // and its first
  before = __shfl_up(pm, 1, 64), after = __shfl_down(sm, 1, 64);
  if (lane == 0) before = -1;
  if (lane == 63) after = ROW_NONE;
  __syncthreads();
#pragma unroll
  for (int w = 0; w < 4; ++w) {
    if (w < wave) before = max(before, wave_last[w]);
    if (w > wave) after = min(after, wave_first[w]);
  }
}

// grid.x of a column pass = tiles of 64 columns x groups of 4 rows x B, x fastest; a wave per (row, 64 columns).  -> whether (y, x) lies inside the map
__device__ __forceinline__ bool col_tile(int H, int W, int tiles_x, int groups_y, int& b, int& y, int& x) {
  const long t = blockIdx.x;
  const int tx = (int)(t % tiles_x);
  const long rest = t / tiles_x;
  const int gy = (int)(rest % groups_y);
  b = (int)(rest / groups_y);
  x = tx * 64 + (threadIdx.x & 63), y = gy * 4 + (threadIdx.x >> 6);
  return x < W && y < H;
}

struct RowColGrid { int tiles_x, groups_y; long rows, blocks; };      // rows, blocks: the workgroups of the row pass and of the column pass
static inline int row_col_grid(const char* name, int B, int H, int W, RowColGrid& g) {      // B, H, W > 0, H * W < 2^31
  g.rows = (long)B * H;
  g.tiles_x = cdiv(W, 64), g.groups_y = cdiv(H, 4);
  g.blocks = (long)g.tiles_x * g.groups_y * B;
  MMSA_CHECK_ARG(g.rows < (1l << 31) && g.blocks < (1l << 31), "%s: %d maps of %d x %d are more workgroups than a launch holds", name, B, H, W);
  return MMSA_OK;
}
