// Calibration on device: the reliability bins of a uint8 class map and its float32 confidence map against a uint8 label map.  Per count slot and
// confidence bin k of K: total (pixels whose transformed label is a class), correct (of those, pred == label class) and conf_sum (the sum of
// floor(conf * 2^24), the confidence in 24-bit fixed point) -- int64 [n_slots, 3, K].  ECE, MCE, the reliability diagram and accuracy against coverage
// are formed from these integers in float64 on the host (mmsa/evaluate.py).  The label side (LUT, nearest-neighbour tables, clamping) is the one of
// csrc/evaluate.hip.
// The walk over (pred, conf, label) is the one of csrc/eval_walk.h, CAL_CHUNK pixels per workgroup.
//
// Bin updates.  Confidence is not patchy like a class map: there are few bins, most pixels of a trained model fall into the top one, and 64 lanes would
// queue on a handful of LDS addresses.  So a lane first merges those of its four pixels that share a bin (neighbours usually do), and a wave then
// reduces bin by bin: the lowest pending lane's bin is broadcast, the lanes that hold it retire, and their (total | correct << 16) and confidence sums
// are two wave reductions in registers; the leading lane then makes TWO 64-bit LDS adds (total | correct << 32, and conf_sum).  A round costs the
// same whatever the number of lanes it retires, so the usual frame (one to three bins per 256 pixels) pays one to three rounds and the worst case, K
// bins spread evenly, pays 4 * min(K, 64) -- and no LDS address ever sees more than one add per wave and round.  Chosen over per-wave sub-histograms
// with lane-by-lane adds: those still serialise the lanes of a wave on the top bin's address, which is the common case here; the rounds remove exactly
// that queue.  (Timed, profiles/calibration.txt: one round per PIXEL of a lane, with ballot popcounts for the counts, took 25.6 us on two 1024 x 1024
// maps where the confusion pass takes 14.1, the lane merge 23.8, and two workgroups per CU -- CAL_CHUNK below -- 16.2.)
// Integer sums only, in LDS and in the int64 result: the same bytes whatever the order of arrival.
#include "common.h"
#include "cal_wave.h"       // cal_wave_sum / cal_wave_add and CAL_NONE (shared with csrc/temperature.hip)
#include "conf_bin.h"
#include "eval_walk.h"

// Pixels per workgroup.  Timed at 2048 / 4096 / 8192 (profiles/calibration.txt; -DCAL_CHUNK with tools/build_variant.sh): at 8192 (EVAL_CHUNK) a CU
// holds one workgroup, one wave per SIMD, and nothing hides a round's dependent steps or the loads in front of them; at 2048 four times as many
// workgroups queue their final 64-bit atomics on the same few addresses; 4096 is the fastest on the model's confidences at both sizes.
#ifndef CAL_CHUNK
#define CAL_CHUNK 4096           // at most 3 * K 64-bit atomics per workgroup at the end (usually under ten)
#endif
#define CAL_MAX_BINS 64
#define CAL_MAX_CLASSES 254      // the LUT's limit (255 = ignored); there is no (C + 1)^2 histogram here

// one pixel -> its bin (CAL_NONE: takes no part), whether it is correct, and its confidence in 24-bit fixed point
__device__ __forceinline__ int cal_pixel(const unsigned char* lut_s, unsigned label_byte, unsigned pred_byte, float c, int C, int K, float Kf, bool& ok,
                                         unsigned& q) {
  const int l = lut_s[label_byte & 255u];
  c = conf_clamp(c);                                                 // NaN, negatives and -0.0 -> 0; above 1 (and +inf) -> 1
  ok = (int)pred_byte == l;
  q = (unsigned)(c * 16777216.0f);                                   // exact scaling, truncated: 0 .. 2^24
  const int k = conf_bin(c, K, Kf);                                  // ONE float32 product, truncated (csrc/conf_bin.h)
  return l < C ? k : CAL_NONE;
}

struct CalArgs : EvalWalkArgs {};       // out: the bins, [n_slots, 3, K]

struct CalPixel {                // what the bins keep of one pixel
  int bin;                       // CAL_NONE: takes no part
  bool ok;
  unsigned q;
};

struct CalBins {
  static constexpr bool CONF = true;
  using Px = CalPixel;
  unsigned long long *tc, *cs;
  const unsigned char* lut_s;
  int C, K;
  float Kf;

  __device__ __forceinline__ CalPixel none() const { return {CAL_NONE, false, 0u}; }
  __device__ __forceinline__ CalPixel pixel(unsigned label_byte, unsigned pred_byte, float c) const {
    CalPixel px;
    px.bin = cal_pixel(lut_s, label_byte, pred_byte, c, C, K, Kf, px.ok, px.q);
    return px;
  }
  // cal_wave_add needs whole waves: the edge path (at most 6 pixels) runs in the first wave only, all of its lanes
  __device__ __forceinline__ bool edge_lanes(int nedge) const { return nedge > 0 && threadIdx.x < 64u; }
  __device__ __forceinline__ void add1(const CalPixel& px) const { cal_wave_add(tc, cs, px.bin, 1u | ((unsigned)px.ok << 16), px.q); }
  __device__ __forceinline__ void add4(bool has, unsigned lv, unsigned pv, float4 cv) const {
    int b[4] = {CAL_NONE, CAL_NONE, CAL_NONE, CAL_NONE};
    bool ok[4] = {false, false, false, false};
    unsigned q[4] = {0u, 0u, 0u, 0u};
    if (has) {
      b[0] = cal_pixel(lut_s, lv, pv & 255u, cv.x, C, K, Kf, ok[0], q[0]);
      b[1] = cal_pixel(lut_s, lv >> 8, (pv >> 8) & 255u, cv.y, C, K, Kf, ok[1], q[1]);
      b[2] = cal_pixel(lut_s, lv >> 16, (pv >> 16) & 255u, cv.z, C, K, Kf, ok[2], q[2]);
      b[3] = cal_pixel(lut_s, lv >> 24, pv >> 24, cv.w, C, K, Kf, ok[3], q[3]);
    }
    unsigned cn[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) cn[j] = 1u | ((unsigned)ok[j] << 16);
#pragma unroll
    for (int j = 1; j < 4; ++j) {                                                // a later pixel of an earlier one's bin joins it
#pragma unroll
      for (int i = 0; i < j; ++i) {
        if (b[j] >= 0 && b[j] == b[i]) {
          cn[i] += cn[j];
          q[i] += q[j];
          b[j] = CAL_NONE;
        }
      }
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) cal_wave_add(tc, cs, b[j], cn[j], q[j]);
  }
};

template <bool TABLES>
__global__ __launch_bounds__(256) void eval_calibration_kernel(CalArgs a, EvalSlots es, int rows) {
  __shared__ unsigned long long tc[CAL_MAX_BINS];      // total | correct << 32: a workgroup sees at most CAL_CHUNK pixels, no carry between the halves
  __shared__ unsigned long long cs[CAL_MAX_BINS];      // sum of floor(conf * 2^24): up to CAL_CHUNK * 2^24 = 2^37
  __shared__ unsigned char lut_s[256];
  const int K = a.K;
  if ((int)threadIdx.x < CAL_MAX_BINS) {
    tc[threadIdx.x] = 0ull;
    cs[threadIdx.x] = 0ull;
  }
  lut_s[threadIdx.x] = a.lut[threadIdx.x];             // 256 threads, 256 bytes
  __syncthreads();
  const int b = blockIdx.y;
  eval_walk<TABLES, CAL_CHUNK>(a, b, rows, CalBins{tc, cs, lut_s, a.C, K, (float)K});
  __syncthreads();
  if ((int)threadIdx.x < K) {
    unsigned long long* dst = a.out + (long)es.s[b] * 3 * K;
    const unsigned long long t = tc[threadIdx.x], s = cs[threadIdx.x];
    if (t) {                                           // conf_sum and correct are zero wherever total is
      atomicAdd(&dst[threadIdx.x], t & 0xffffffffull);
      if (t >> 32) atomicAdd(&dst[K + threadIdx.x], t >> 32);
      if (s) atomicAdd(&dst[2 * K + threadIdx.x], s);
    }
  }
}

extern "C" int mmsa_eval_calibration(const unsigned char* pred, const float* conf, const unsigned char* label, int B, int H, int W, int Hl, int Wl,
                                     const unsigned char* lut, int C, const int* ymap, const int* xmap, const int* slots /* HOST [B] */, int n_slots,
                                     int bins, int64_t* cal, hipStream_t stream) {
  const char* name = "eval_calibration";
  MMSA_CHECK_ARG(pred && conf && label && lut && slots && cal, "%s: pred, conf, label, lut, slots and cal are required", name);
  MMSA_CHECK_ARG(((uintptr_t)conf & 3u) == 0, "%s: conf must be 4-byte aligned", name);
  MMSA_CHECK_ARG(bins >= 1 && bins <= CAL_MAX_BINS, "%s: %d bins; 1..%d are supported", name, bins, CAL_MAX_BINS);
  EvalSlots es;
  int rc = eval_check(name, label, B, H, W, Hl, Wl, lut, C, ymap, xmap, slots, n_slots, cal, es, CAL_MAX_CLASSES, "a uint8 label LUT; 255 means ignored");
  if (rc) return rc;
  const CalArgs a = {{pred, conf, label, lut, ymap, xmap, (unsigned long long*)cal, H, W, Hl, Wl, C, bins}};
  eval_walk_launch(eval_calibration_kernel<true>, eval_calibration_kernel<false>, ymap != NULL, CAL_CHUNK, B, H, W, 1, 0, stream, a, es);
  MMSA_CHECK_LAUNCH("eval_calibration");
  return MMSA_OK;
}
