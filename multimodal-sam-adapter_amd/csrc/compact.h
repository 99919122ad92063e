// Stream compaction of the flagged pixels of a map, once: csrc/segtable.hip (the listed roots) and csrc/runs.hip (the run heads) number them with it.
// The contract.  A BLOCK is PER_LANE * 256 consecutive flat indices of one image, a workgroup of 256 lanes each, grid (blocks, B).
// Lane t owns compact_index<PER_LANE>(k) = block * PER_LANE * 256 + k * 256 + t: pixel order is (k, wave, lane).  Reduce-then-scan, three launches -- no
// workgroup waits for another and no loop spins on a value somebody else must write:
//   count   compact_block_count: the flags of a block -> scratch[b, block], one int32 word per block and image.
//   scan    compact_scan: ONE workgroup per image turns scratch[b, :] into its exclusive prefix sums, COMPACT_SCAN_TRIP counts per trip with a carry.
//   rank    the flags again: compact_block_rank gives a flagged pixel its rank in the block; scratch[b, block] + rank numbers it within the image, and the
//           last block's scratch word + its total is the image's count.
// Every helper is called by ALL 256 lanes of the workgroup together (ballots, barriers), once per kernel (one LDS table each).
#pragma once
#include "common.h"

#define COMPACT_SCAN_LANES 256                // lanes of the scan workgroup
#define COMPACT_SCAN_PER_LANE 4               // consecutive block counts a lane takes per trip
#define COMPACT_SCAN_TRIP (COMPACT_SCAN_LANES * COMPACT_SCAN_PER_LANE)

// scratch[b, :] (n words each, B images) -> its exclusive prefix sums, in place: one launch (csrc/compact.hip)
void compact_scan(int* scratch, int B, int n, hipStream_t stream);

#define COMPACT_CHECK_BLOCK(block) \
  static_assert((block) % 256 == 0 && (block) >= 256 && (block) <= 64 * 256, "a block is 1..64 pixels per lane of 256 lanes: at most 256 (k, wave) counts")

template <int PER_LANE>
__device__ __forceinline__ long compact_index(int k) { return (long)blockIdx.x * (PER_LANE * 256) + k * 256 + threadIdx.x; }

// an inclusive prefix sum over the 64 lanes of a wave
__device__ __forceinline__ int compact_wave_scan(int v, int lane) {
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const int up = __shfl_up(v, d);
    if (lane >= d) v += up;
  }
  return v;
}

// flag(k, i) -> bool for pixel i = compact_index(k).  It is evaluated by every lane for every k, pixels past the image's end too, and there is no early exit:
// a predicate may shuffle across the wave (runs_row_head), so all 64 lanes call it together -- it tests the range itself.
template <int PER_LANE, typename F>
__device__ __forceinline__ void compact_block_count(F flag, int nblk, int* __restrict__ scratch) {
  __shared__ int ws[4];
  int n = 0;
#pragma unroll
  for (int k = 0; k < PER_LANE; ++k) n += (int)__popcll(__ballot(flag(k, compact_index<PER_LANE>(k))));      // the wave's flags of this k, in every lane
  if ((threadIdx.x & 63u) == 0) ws[threadIdx.x >> 6] = n;
  __syncthreads();
  if (threadIdx.x == 0) scratch[(long)blockIdx.y * nblk + blockIdx.x] = ws[0] + ws[1] + ws[2] + ws[3];
}

// flags[k] of this lane's pixels, already evaluated -> rank[k] = the flagged pixels of the block before pixel k of this lane, in pixel order (of use where
// flags[k]), and total = the block's flags.  The counts per (k, wave) go through one LDS table, which wave 0 scans in trips of 64 with a carry (PER_LANE <= 16,
// so the shipped 2048-pixel block: one trip).
template <int PER_LANE>
__device__ __forceinline__ void compact_block_rank(const bool (&flags)[PER_LANE], int (&rank)[PER_LANE], int& total) {
  constexpr int N = PER_LANE * 4;
  __shared__ int cnt[N + 1];                                                   // the flags per (k, wave), then their exclusive prefix sums and the total
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
#pragma unroll
  for (int k = 0; k < PER_LANE; ++k) {
    const unsigned long long ms = __ballot(flags[k]);
    rank[k] = (int)__popcll(ms & ((1ull << lane) - 1ull));                     // the flagged lanes of this wave and k below this one
    if (lane == 0) cnt[k * 4 + w] = (int)__popcll(ms);
  }
  __syncthreads();
  if (w == 0) {
    int carry = 0;
#pragma unroll
    for (int c = 0; c < N; c += 64) {
      const int j = c + lane, v = j < N ? cnt[j] : 0, inc = compact_wave_scan(v, lane);
      if (j < N) cnt[j] = carry + inc - v;
      carry += __builtin_amdgcn_readlane(inc, 63);
    }
    if (lane == 0) cnt[N] = carry;
  }
  __syncthreads();
#pragma unroll
  for (int k = 0; k < PER_LANE; ++k) rank[k] += cnt[k * 4 + w];
  total = cnt[N];
}
