// The scan launch of the stream compaction (csrc/compact.h): the library's one copy of the kernel, for every user.
#include "compact.h"

// grid B: scratch[b, :] (n words) -> its exclusive prefix sums, in place
__global__ __launch_bounds__(COMPACT_SCAN_LANES) void compact_scan_kernel(int n, int* scratch) {
  __shared__ int ws[COMPACT_SCAN_LANES / 64];
  int* s = scratch + (long)blockIdx.x * n;
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  int carry = 0;
  for (long c = 0; c < n; c += COMPACT_SCAN_TRIP) {                            // bounded by the block count
    const long j0 = c + (long)threadIdx.x * COMPACT_SCAN_PER_LANE;
    int v[COMPACT_SCAN_PER_LANE], sum = 0;
#pragma unroll
    for (int k = 0; k < COMPACT_SCAN_PER_LANE; ++k) {
      v[k] = j0 + k < n ? s[j0 + k] : 0;
      sum += v[k];
    }
    const int inc = compact_wave_scan(sum, lane);
    if (lane == 63) ws[w] = inc;
    __syncthreads();
    int before = 0, total = 0;
#pragma unroll
    for (int k = 0; k < COMPACT_SCAN_LANES / 64; ++k) {
      before += k < w ? ws[k] : 0;
      total += ws[k];
    }
    int run = carry + before + inc - sum;
#pragma unroll
    for (int k = 0; k < COMPACT_SCAN_PER_LANE; ++k) {
      if (j0 + k < n) s[j0 + k] = run;
      run += v[k];
    }
    carry += total;
    __syncthreads();                                                           // ws is written again in the next trip
  }
}

void compact_scan(int* scratch, int B, int n, hipStream_t stream) {
  hipLaunchKernelGGL(compact_scan_kernel, dim3(B), dim3(COMPACT_SCAN_LANES), 0, stream, n, scratch);
}
