// The wave-level bin-by-bin reduction of the passes that add per-pixel terms to a handful of confidence bins in LDS: csrc/calibrate.hip (reliability
// bins) and csrc/temperature.hip (the same bins and the NLL, once per temperature).  Why rounds and not lane-by-lane adds: the header of calibrate.hip.
#pragma once

#define CAL_NONE (-1)            // a lane without a participating pixel

// Sum of v over the 64 lanes of a wave, the same in every lane; all lanes must be active.  Inside each row of 16 lanes by data-parallel-primitive moves
// (no LDS crossbar: lane ^ 1, lane ^ 2, then the row rotated by 4 and by 8) in 32 bits -- a row's sum must fit them -- then the four row sums through
// scalar registers, added in 64 bits.
__device__ __forceinline__ unsigned long long cal_wave_sum(unsigned v) {
  v += (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0xB1, 0xf, 0xf, true);      // quad_perm:[1,0,3,2]
  v += (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0x4E, 0xf, 0xf, true);      // quad_perm:[2,3,0,1]: every lane holds its quad's sum
  v += (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0x124, 0xf, 0xf, true);     // row_ror:4: two quads
  v += (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0x128, 0xf, 0xf, true);     // row_ror:8: the row
  return (unsigned long long)(unsigned)__builtin_amdgcn_readlane((int)v, 0) + (unsigned long long)(unsigned)__builtin_amdgcn_readlane((int)v, 16) +
         (unsigned long long)(unsigned)__builtin_amdgcn_readlane((int)v, 32) + (unsigned long long)(unsigned)__builtin_amdgcn_readlane((int)v, 48);
}

// Add one entry per lane to the workgroup's bins (see the header of calibrate.hip): `cnt` = pixels | correct pixels << 16 (up to 4 each), `q` their
// confidence sum (up to 4 * 2^24, so a row of 16 lanes stays below 2^32).  Must be called by all lanes of a wave together (bin = CAL_NONE where a lane
// has none).
__device__ __forceinline__ void cal_wave_add(unsigned long long* tc, unsigned long long* cs, int bin, unsigned cnt, unsigned q) {
  bool pending = bin >= 0;
  unsigned long long m = __ballot(pending);
  while (m != 0ull) {
    const int lead = __ffsll((long long)m) - 1;
    const int lb = __builtin_amdgcn_readlane(bin, lead);
    const bool same = pending && bin == lb;
    const unsigned long long ms = __ballot(same);
    const unsigned long long n = cal_wave_sum(same ? cnt : 0u);          // at most 256 in either half
    const unsigned long long v = cal_wave_sum(same ? q : 0u);
    if ((int)(threadIdx.x & 63u) == lead) {
      atomicAdd(&tc[lb], (n & 0xffffull) | ((n >> 16) << 32));
      atomicAdd(&cs[lb], v);
    }
    pending = pending && !same;
    m &= ~ms;
  }
}
