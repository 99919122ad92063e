// Temperature scaling on device, the FIT side: one pass over a logits canvas [B, C, H, W] evaluates, for a whole grid of temperatures T_j at once, the
// reliability bins of max_c softmax(x / T_j)_c and the negative log-likelihood of the label's class -- everything a one-parameter fit of T on a validation
// split needs (minimise the NLL, or the ECE, over the grid; refine by a second, narrower grid).  The APPLY side is the `_t` siblings of the confidence kernels
// (csrc/segment.hip, csrc/augment.hip); both sides are made of the pieces of csrc/softmax_px.h and round alike.
//   sweep = int64 [n_slots, J, 4, K]: per temperature j and confidence bin k, total / correct / conf_sum (the three rows of mmsa_eval_calibration, of the
//   canvas path's class map and its confidence at T_j) and nll_sum (the sum of floor(nll * 2^20), the NLL in 20-bit fixed point, capped at 1024 per pixel).
// The label side (LUT in LDS, nearest-neighbour tables, clamping, slots) is the one of csrc/evaluate.hip; a pixel takes part iff its label is a class,
// Calibration's rule.
//
// One lane per pixel, lanes along x: the reads of a class plane are coalesced.  A first pass over the classes gives the maximum m, the first argmax p and the
// label's logit x_l; a second pass re-reads the pixel's logits (they are in the caches: a workgroup touches C runs of SWEEP_CHUNK floats) and forms the J
// sums of exponentials in registers -- a constant-bound unrolled loop with predicates, as the slot arrays of slide_pixel.h.  Then, temperature by
// temperature, the wave reduces bin by bin as calibrate.hip does (most pixels share a bin at every temperature) into uint64 LDS cells [J][K], which one
// flush per workgroup adds to the result with 64-bit atomics.  Integer sums only, in LDS and in the int64 result: the same bytes whatever the order of arrival.
#include "common.h"

// No fused multiply-add contraction: (x - m) * it and logf(s) - (x_l - m) * it are stated as separate roundings (softmax_px.h; DESIGN section 2 bounds them).
#pragma clang fp contract(off)
#include "cal_wave.h"
#include "conf_bin.h"
#include "eval_walk.h"       // eval_label_at; eval_hist.h: EvalLabel, EvalSlots, eval_check
#include "softmax_px.h"

#define SWEEP_MAX_TEMPS 16
#define SWEEP_MAX_BINS 64
#define SWEEP_MAX_CLASSES 254    // the LUT's limit (255 = ignored)
#define SWEEP_CHUNK 2048         // pixels per workgroup: 8 trips of 256 lanes; at most 4 * J * K 64-bit atomics per workgroup at the end.  Not tuned by measurement.
#define SWEEP_NLL_CAP 1024.0f    // a pixel's NLL is capped here (and NaN becomes the cap): n < 2^30 + 1
#define SWEEP_NLL_ONE 1048576.0f // 2^20, the fixed-point unit of nll_sum

struct SweepTemps { float it[SWEEP_MAX_TEMPS]; };      // the inverse temperatures, by value in the launch arguments: indexed by unrolled constants only

// cal_wave_add with the NLL term: `n` < 2^30 + 1 per lane, and sixteen of those do not fit the 32 bits a row of cal_wave_sum adds in, so it is reduced in two
// 16-bit halves.  `cnt` = 1 | correct << 16, `q` <= 2^24.  Must be called by all lanes of a wave together (bin = CAL_NONE where a lane has no pixel).
__device__ __forceinline__ void sweep_wave_add(unsigned long long* tc, unsigned long long* cs, unsigned long long* ns, int bin, unsigned cnt, unsigned q,
                                               unsigned n) {
  bool pending = bin >= 0;
  unsigned long long m = __ballot(pending);
  while (m != 0ull) {
    const int lead = __ffsll((long long)m) - 1;
    const int lb = __builtin_amdgcn_readlane(bin, lead);
    const bool same = pending && bin == lb;
    const unsigned long long ms = __ballot(same);
    const unsigned long long c = cal_wave_sum(same ? cnt : 0u);          // at most 64 in either half
    const unsigned long long v = cal_wave_sum(same ? q : 0u);
    const unsigned long long nlo = cal_wave_sum(same ? (n & 0xffffu) : 0u), nhi = cal_wave_sum(same ? (n >> 16) : 0u);
    if ((int)(threadIdx.x & 63u) == lead) {
      atomicAdd(&tc[lb], (c & 0xffffull) | ((c >> 16) << 32));
      atomicAdd(&cs[lb], v);
      atomicAdd(&ns[lb], nlo + (nhi << 16));
    }
    pending = pending && !same;
    m &= ~ms;
  }
}

// JMAX: the compile-time bound of the loops over the temperatures (1, 4, 8 or 16; the launch takes the smallest that holds J): the predicates of the unrolled
// loops are scalar branches, and sixteen of them per class cost a single temperature more than its exponentials do (472 us against 178 on two 1024 x 1024 maps, profiles/temperature.txt).  Same statements, same bits, whatever JMAX.
template <bool TABLES, int JMAX>
__global__ __launch_bounds__(256) void temperature_sweep_kernel(const float* __restrict__ logits, EvalLabel ev, EvalSlots es, SweepTemps ts, int H, int W, int J,
                                                                int K) {
  __shared__ unsigned long long tc[SWEEP_MAX_TEMPS * SWEEP_MAX_BINS];      // total | correct << 32: a workgroup sees at most SWEEP_CHUNK pixels, no carry between the halves
  __shared__ unsigned long long cs[SWEEP_MAX_TEMPS * SWEEP_MAX_BINS];      // sum of floor(conf * 2^24): up to SWEEP_CHUNK * 2^24
  __shared__ unsigned long long ns[SWEEP_MAX_TEMPS * SWEEP_MAX_BINS];      // sum of floor(nll * 2^20): up to SWEEP_CHUNK * 2^30
  __shared__ unsigned char lut_s[256];
  const int JK = J * K;                                                    // cell (j, k) at j * K + k
  for (int i = threadIdx.x; i < JK; i += 256) tc[i] = cs[i] = ns[i] = 0ull;
  lut_s[threadIdx.x] = ev.lut[threadIdx.x];                                // 256 threads, 256 bytes
  __syncthreads();
  const int b = blockIdx.y, C = ev.C;
  const int HW = H * W;                                                    // < 2^31 (eval_check)
  const long start = (long)blockIdx.x * SWEEP_CHUNK;
  const int end = (int)min((long)HW, start + SWEEP_CHUNK);
  const float Kf = (float)K;
  for (long i0 = start; i0 < end; i0 += 256) {                             // uniform: every lane of the workgroup makes every trip
    const long i_ = i0 + (long)threadIdx.x;
    const int i = (int)min(i_, (long)end);                                 // a lane past the end holds no pixel (l stays ignored)
    int l = MMSA_EVAL_IGNORE;
    if (i_ < end) {
      unsigned lb;
      if (TABLES) {
        const int y = i / W, x = i - y * W;
        const int ys = min(max(ev.ymap[y], 0), ev.Hl - 1);
        lb = eval_label_at<true>(ev.label + ((long)b * ev.Hl + ys) * ev.Wl, ev.xmap, ev.Wl, x);
      } else {
        lb = ev.label[(long)b * HW + i];
      }
      l = lut_s[lb & 255u];
    }
    const bool part = l < C;                                               // Calibration's rule: the transformed label is a class
    float m = 0.f, xl = 0.f, s[JMAX];
    int p = 0;
#pragma unroll
    for (int j = 0; j < JMAX; ++j) s[j] = 1.f;
    if (part) {
      const float* __restrict__ xp = logits + (long)b * C * HW + i;
      float best = 0.f;
      for (int c = 0; c < C; ++c) {
        const float x = xp[(long)c * HW];
        m = c == 0 ? x : softmax_px_max(m, x);
        if (c == 0 || x > best) { best = x; p = c; }                       // first maximum wins (argmax_nchw_kernel)
        if (c == l) xl = x;
      }
      for (int c = 0; c < C; ++c) {
        const float x = xp[(long)c * HW];
#pragma unroll
        for (int j = 0; j < JMAX; ++j)
          if (JMAX == 1 || j < J) s[j] = softmax_px_sum(s[j], softmax_px_exp_t(x, m, ts.it[j]), c == 0);
      }
    }
    const unsigned cnt = 1u | ((unsigned)(p == l) << 16);
#pragma unroll
    for (int j = 0; j < JMAX; ++j) {
      if (JMAX == 1 || j < J) {                                            // uniform
        const float it = ts.it[j];
        const float cf = conf_clamp(softmax_px_prob(softmax_px_exp_t(m, m, it), s[j]));      // P at the first maximum: the largest probability
        const float nll = logf(s[j]) - (xl - m) * it;                      // -log softmax(x * it)[l]
        const float t = !(nll < SWEEP_NLL_CAP) ? SWEEP_NLL_CAP : (nll > 0.f ? nll : 0.f);   // clamp to [0, cap]; NaN -> cap
        sweep_wave_add(tc + j * K, cs + j * K, ns + j * K, part ? conf_bin(cf, K, Kf) : CAL_NONE, cnt, (unsigned)(cf * 16777216.0f),
                       (unsigned)(t * SWEEP_NLL_ONE));
      }
    }
  }
  __syncthreads();
  unsigned long long* dst = ev.counts + (long)es.s[b] * 4 * JK;
  for (int i = threadIdx.x; i < JK; i += 256) {
    const unsigned long long t = tc[i], c = cs[i], n = ns[i];
    if (t) {                                                               // correct, conf_sum and nll_sum are zero wherever total is
      const int j = i / K, k = i - j * K;
      unsigned long long* d = dst + (long)j * 4 * K + k;
      atomicAdd(&d[0], t & 0xffffffffull);
      if (t >> 32) atomicAdd(&d[K], t >> 32);
      if (c) atomicAdd(&d[2 * K], c);
      if (n) atomicAdd(&d[3 * K], n);
    }
  }
}

template <int JMAX>
static inline void sweep_launch(bool tables, dim3 grid, hipStream_t stream, const float* logits, const EvalLabel& ev, const EvalSlots& es, const SweepTemps& ts, int H,
                                int W, int J, int K) {
  if (tables) hipLaunchKernelGGL((temperature_sweep_kernel<true, JMAX>), grid, dim3(256), 0, stream, logits, ev, es, ts, H, W, J, K);
  else hipLaunchKernelGGL((temperature_sweep_kernel<false, JMAX>), grid, dim3(256), 0, stream, logits, ev, es, ts, H, W, J, K);
}

extern "C" int mmsa_temperature_sweep_nchw(const float* logits, const unsigned char* label, int B, int C, int H, int W, int Hl, int Wl, const unsigned char* lut,
                                           const int* ymap, const int* xmap, const int* slots /* HOST [B] */, int n_slots,
                                           const float* inv_temperatures /* HOST [J] */, int J, int bins, int64_t* sweep, hipStream_t stream) {
  const char* name = "temperature_sweep_nchw";
  MMSA_CHECK_ARG(logits && label && lut && slots && inv_temperatures && sweep, "%s: logits, label, lut, slots, inv_temperatures and sweep are required", name);
  MMSA_CHECK_ARG(((uintptr_t)logits & 3u) == 0, "%s: logits must be 4-byte aligned", name);
  MMSA_CHECK_ARG(J >= 1 && J <= SWEEP_MAX_TEMPS, "%s: %d temperatures; 1..%d per call are supported (their sums live in registers)", name, J, SWEEP_MAX_TEMPS);
  MMSA_CHECK_ARG(bins >= 1 && bins <= SWEEP_MAX_BINS, "%s: %d bins; 1..%d are supported", name, bins, SWEEP_MAX_BINS);
  SweepTemps ts;
  for (int j = 0; j < SWEEP_MAX_TEMPS; ++j) ts.it[j] = 1.f;
  for (int j = 0; j < J; ++j) {
    MMSA_CHECK_INV_TEMPERATURE(name, inv_temperatures[j]);
    ts.it[j] = inv_temperatures[j];
  }
  EvalSlots es;
  int rc = eval_check(name, label, B, H, W, Hl, Wl, lut, C, ymap, xmap, slots, n_slots, sweep, es, SWEEP_MAX_CLASSES, "a uint8 label LUT; 255 means ignored");
  if (rc) return rc;
  const EvalLabel ev = {label, lut, ymap, xmap, (unsigned long long*)sweep, Hl, Wl, C};
  const dim3 grid(cdiv((long)H * W, (long)SWEEP_CHUNK), B);
  if (J == 1) sweep_launch<1>(ymap != NULL, grid, stream, logits, ev, es, ts, H, W, J, bins);
  else if (J <= 4) sweep_launch<4>(ymap != NULL, grid, stream, logits, ev, es, ts, H, W, J, bins);
  else if (J <= 8) sweep_launch<8>(ymap != NULL, grid, stream, logits, ev, es, ts, H, W, J, bins);
  else sweep_launch<SWEEP_MAX_TEMPS>(ymap != NULL, grid, stream, logits, ev, es, ts, H, W, J, bins);
  MMSA_CHECK_LAUNCH(name);
  return MMSA_OK;
}
