// What the passes over root maps share: csrc/components.hip (areas, suppression, segment counts) and csrc/pairs.hip (the pair table, panoptic matching).
// Root maps are int32 [B, H, W] as mmsa_components_u8 writes them, B * H * W < 2^31; every pass clamps a root before it addresses anything with it.
// These passes keep no LDS: they read a label code with label_code(ev, ev.lut, ...) of csrc/code_map.h, the LUT in global memory.
#pragma once
#include "common.h"
#include "eval_hist.h"

#define COMP_SIZE_BUCKETS 24                  // s = min(23, floor(log2 area))

static inline int comp_check_size(const char* name, int B, int H, int W) {
  MMSA_CHECK_ARG(B > 0 && B <= 65535 && H > 0 && W > 0 && (long)B * H * W < (1l << 31),
                 "%s: bad map size %d x %d x %d (B * H * W must be positive and below 2^31, B at most 65535)", name, B, H, W);
  return MMSA_OK;
}

static inline int comp_zero(const char* name, void* p, size_t bytes, hipStream_t stream) {
  const hipError_t e = hipMemsetAsync(p, 0, bytes, stream);
  MMSA_CHECK_ARG(e == hipSuccess, "%s: zeroing the planes failed: %s", name, hipGetErrorString(e));
  return MMSA_OK;
}

// dst[key] += the number of lanes that hold `key` (and dst2[key] += those of them with `flag`, where dst2 is given), ONE atomicAdd per (wave, key).  Called by
// every lane of a wave together; `has` = false: a lane without a pixel.  At most 64 distinct keys in a wave: 64 rounds.
__device__ __forceinline__ void comp_wave_add(int* dst, int* dst2, bool has, int key, bool flag) {
  bool pending = has;
  unsigned long long m = __ballot(pending);
  for (int r = 0; r < 64 && m != 0ull; ++r) {
    const int lead = __ffsll((long long)m) - 1;
    const int lk = __builtin_amdgcn_readlane(key, lead);
    const bool same = pending && key == lk;
    const unsigned long long ms = __ballot(same), mf = __ballot(same && flag);
    if ((int)(threadIdx.x & 63u) == lead) {
      atomicAdd(&dst[lk], (int)__popcll(ms));
      if (dst2 && mf) atomicAdd(&dst2[lk], (int)__popcll(mf));
    }
    pending = pending && !same;
    m &= ~ms;
  }
}

// counts[bin] += 1 for every lane with bin >= 0: two rounds of the merge above first (a frame's root pixels of one class and size mostly share a cell), the
// rest lane by lane.  Called by every lane of a wave together.
__device__ __forceinline__ void seg_count_add(unsigned long long* counts, int bin) {
  bool pending = bin >= 0;
#pragma unroll
  for (int r = 0; r < 2; ++r) {
    const unsigned long long m = __ballot(pending);
    if (m == 0ull) return;
    const int lead = __ffsll((long long)m) - 1;
    const int lb = __builtin_amdgcn_readlane(bin, lead);
    const bool same = pending && bin == lb;
    const unsigned long long ms = __ballot(same);
    if ((int)(threadIdx.x & 63u) == lead) atomicAdd(&counts[lb], (unsigned long long)__popcll(ms));
    pending = pending && !same;
  }
  if (pending) atomicAdd(&counts[bin], 1ull);
}

// the size bucket of a segment of `area` > 0 pixels
__device__ __forceinline__ int comp_size_bucket(int area) { return min(COMP_SIZE_BUCKETS - 1, 31 - __clz(area)); }
