// Selective evaluation on device: one confusion matrix per confidence bin.  For a uint8 class map, its float32 confidence map and a uint8 label map,
//   counts[slot][k][row][col] += 1, int64 [n_slots, K, C + 1, C + 1],
// for every pixel whose label is not ignored: row / col are the cell of csrc/eval_hist.h (eval_bin: min(l, C), min(pred, C)) and k is the bin of
// csrc/conf_bin.h (the clamp and the ONE float32 product of csrc/calibrate.hip).  The sum over k is Evaluator's matrix; the rows < C of bin k sum to
// Calibration's total[k] and the trace of its [:C, :C] block is correct[k]; the suffix sums over k are the confusion counts of the map with the pixels
// below a confidence threshold taken out -- mIoU against coverage, formed in float64 on the host (mmsa/evaluate.py).  mmsa_abstain_u8 below writes
// that thresholded map from the same clamp and bin.
// The walk over (pred, conf, label) is the one of csrc/eval_walk.h, SEL_CHUNK pixels per workgroup.
//
// LDS budget and bin groups.  A workgroup keeps a private uint32 histogram of the bins it is responsible for: (C + 1)^2 * 4 bytes per bin, 40 560 B for
// the model's 25 classes and 15 bins.  The launch stays within the 64 KiB a launch may ask for without a function attribute (as evaluate.hip does):
// G = (65536 - 256) / ((C + 1)^2 * 4) bins are resident (the 256 bytes are the LUT), gridDim.z = ceil(K / G) bin groups each walk the pixels and count
// only those whose bin falls in their group, and the last group may be partial.  C <= 126 gives G >= 1; at C = 25, K <= 24 there is one group and one
// read of the data.
//
// Same-cell merging.  Class maps are patchy and most pixels of a trained model sit in the top confidence bin, so the lanes of a wave often hold the SAME
// cell.  SEL_MERGE chooses the form (timed: profiles/selective.txt):
//   0  every pixel through eval_hist_add's two broadcast rounds on the combined key k * (C + 1)^2 + row * (C + 1) + col;
//   1  evaluate.hip's form: a lane whose four pixels share a key makes one add of 4 through the broadcast rounds, any other lane four plain LDS atomics;
//   2  as 1, but the pixels of a mixed lane go through the broadcast rounds as well (merged among the mixed lanes).
// Form 1 is the fastest on every leg: on the model's confidences form 0 takes 1.3 us more (16.9 against 15.6) and form 2 2.5 - 2.9 us more, on uniform
// confidences 3.4 - 5.0 us more.
// Integer sums only, in LDS and in the int64 result: the same bytes whatever the order of arrival.  Plain C++ and HIP atomics; no inline assembly.
#include "common.h"
#include "conf_bin.h"
#include "eval_walk.h"

// Pixels per workgroup.  A workgroup zeroes and scans its whole histogram (K * (C + 1)^2 words: 40 per lane at 25 classes and 15 bins) whatever it
// walked, so the chunk is evaluate.hip's 8192 rather than calibrate.hip's 4096: 32 pixels per lane against those 80 LDS accesses, and two 1024 x 1024
// maps are 256 workgroups, one per CU of the chip.  Timed (profiles/selective.txt): 4096 is 0.4 - 0.6 us faster on the model's confidences with one bin
// group (15.15 against 15.56 us, 14.94 against 15.54: within that leg's own p90 - p10), 2 - 6 us slower on uniform confidences and 9 - 11 us slower with
// six bin groups, where every group zeroes and scans twice as often.
#ifndef SEL_CHUNK
#define SEL_CHUNK 8192
#endif
#ifndef SEL_MERGE
#define SEL_MERGE 1
#endif
#define SEL_MAX_BINS 64
#define SEL_LDS_BYTES (65536 - 256)       // the histogram's share of the 64 KiB; the LUT takes the rest

struct SelArgs : EvalWalkArgs {  // out: the counts, [n_slots, K, C + 1, C + 1]
  int G;                         // bins per group
};

struct SelGroup {                // what a workgroup's bin group needs per pixel
  const unsigned char* lut_s;
  int C, nb, K, k0, kn;          // nb = (C + 1)^2; the group holds the bins k0 .. k0 + kn - 1
  float Kf;
};

// one pixel -> its cell in the group's histogram, or -1: ignored label, or a bin of another group
__device__ __forceinline__ int sel_key(const SelGroup& g, unsigned label_byte, unsigned pred_byte, float c) {
  const int cell = eval_bin(g.lut_s, label_byte, pred_byte, g.C);
  const int k = conf_bin(conf_clamp(c), g.K, g.Kf) - g.k0;
  return (cell >= 0 && (unsigned)k < (unsigned)g.kn) ? k * g.nb + cell : -1;
}

struct SelCounts {
  static constexpr bool CONF = true;
  using Px = int;                                                                // the pixel's key, or -1
  unsigned* hist;
  const SelGroup& g;

  __device__ __forceinline__ int none() const { return -1; }
  __device__ __forceinline__ int pixel(unsigned label_byte, unsigned pred_byte, float c) const { return sel_key(g, label_byte, pred_byte, c); }
  __device__ __forceinline__ bool edge_lanes(int) const { return true; }
  __device__ __forceinline__ void add1(int key) const { eval_hist_add(hist, key, 1u); }
  __device__ __forceinline__ void add4(bool has, unsigned lv, unsigned pv, float4 cv) const {
    int b0 = -1, b1 = -1, b2 = -1, b3 = -1;
    if (has) {
      b0 = sel_key(g, lv, pv & 255u, cv.x);
      b1 = sel_key(g, lv >> 8, (pv >> 8) & 255u, cv.y);
      b2 = sel_key(g, lv >> 16, (pv >> 16) & 255u, cv.z);
      b3 = sel_key(g, lv >> 24, pv >> 24, cv.w);
    }
#if SEL_MERGE == 0
    eval_hist_add(hist, b0, 1u);
    eval_hist_add(hist, b1, 1u);
    eval_hist_add(hist, b2, 1u);
    eval_hist_add(hist, b3, 1u);
#else
    const bool uni = b0 >= 0 && b0 == b1 && b1 == b2 && b2 == b3;                // four pixels of one cell: one add of 4, merged across the wave
    eval_hist_add(hist, uni ? b0 : -1, 4u);
    if (!uni) {
#if SEL_MERGE == 1
      if (b0 >= 0) atomicAdd(&hist[b0], 1u);
      if (b1 >= 0) atomicAdd(&hist[b1], 1u);
      if (b2 >= 0) atomicAdd(&hist[b2], 1u);
      if (b3 >= 0) atomicAdd(&hist[b3], 1u);
#else
      eval_hist_add(hist, b0, 1u);                                               // the ballots see the mixed lanes only
      eval_hist_add(hist, b1, 1u);
      eval_hist_add(hist, b2, 1u);
      eval_hist_add(hist, b3, 1u);
#endif
    }
#endif
  }
};

template <bool TABLES>
__global__ __launch_bounds__(256) void eval_selective_kernel(SelArgs a, EvalSlots es, int rows) {
  extern __shared__ unsigned sel_lds[];
  const int C = a.C, K = a.K, nb = (C + 1) * (C + 1);
  const int k0 = (int)blockIdx.z * a.G, kn = min(a.G, K - k0);                   // this group's bins; the launch asked for min(G, K) * nb words
  unsigned* hist = sel_lds;
  unsigned char* lut_s = (unsigned char*)(sel_lds + min(a.G, K) * nb);
  eval_hist_init(hist, lut_s, a.lut, kn * nb);
  const SelGroup g = {lut_s, C, nb, K, k0, kn, (float)K};
  const int b = blockIdx.y;
  eval_walk<TABLES, SEL_CHUNK>(a, b, rows, SelCounts{hist, g});
  eval_hist_flush(hist, a.out + ((long)es.s[b] * K + k0) * nb, kn * nb);
}

extern "C" int mmsa_eval_selective(const unsigned char* pred, const float* conf, const unsigned char* label, int B, int H, int W, int Hl, int Wl,
                                   const unsigned char* lut, int C, const int* ymap, const int* xmap, const int* slots /* HOST [B] */, int n_slots,
                                   int bins, int64_t* counts, hipStream_t stream) {
  const char* name = "eval_selective";
  MMSA_CHECK_ARG(pred && conf, "%s: pred and conf are required", name);
  MMSA_CHECK_ARG(((uintptr_t)conf & 3u) == 0, "%s: conf must be 4-byte aligned", name);
  MMSA_CHECK_ARG(bins >= 1 && bins <= SEL_MAX_BINS, "%s: %d bins; 1..%d are supported", name, bins, SEL_MAX_BINS);
  EvalSlots es;
  int rc = eval_check(name, label, B, H, W, Hl, Wl, lut, C, ymap, xmap, slots, n_slots, counts, es);
  if (rc) return rc;
  const int nb = (C + 1) * (C + 1);
  const int G = SEL_LDS_BYTES / (nb * 4);              // >= 1 for C <= MMSA_EVAL_MAX_CLASSES
  const int groups = cdiv(bins, G);
  const size_t lds = (size_t)min(G, bins) * nb * 4 + 256;
  const SelArgs a = {{pred, conf, label, lut, ymap, xmap, (unsigned long long*)counts, H, W, Hl, Wl, C, bins}, G};
  eval_walk_launch(eval_selective_kernel<true>, eval_selective_kernel<false>, ymap != NULL, SEL_CHUNK, B, H, W, groups, lds, stream, a, es);
  MMSA_CHECK_LAUNCH("eval_selective");
  return MMSA_OK;
}

// ---- the thresholded map: out[i] = pred[i] where bin(conf[i]) >= min_bin, 255 elsewhere (the same clamp and bin as the counts above)

// `head` pixels in front of the first aligned pred dword and the tail behind the last whole one go one pixel per lane (the first workgroup's lanes
// 0 .. 5); the rest as one pred dword and four confidences per lane.  A lane reads its own pixels before it writes them: out may be pred itself
// (any other overlap of the two is the caller's error).
__global__ __launch_bounds__(256) void abstain_u8_kernel(const unsigned char* pred, const float* __restrict__ conf, long n, int K, int min_bin,
                                                         unsigned char* out) {
  const float Kf = (float)K;
  const long lead = (long)((4u - (unsigned)((uintptr_t)pred & 3u)) & 3u);
  const int head = (int)(n < lead ? n : lead);
  const long ndw = (n - head) >> 2;
  const long tail0 = head + (ndw << 2);
  const int nedge = head + (int)(n - tail0);
  if (blockIdx.x == 0 && (int)threadIdx.x < nedge) {
    const long i = (int)threadIdx.x < head ? (long)threadIdx.x : tail0 + ((int)threadIdx.x - head);
    const unsigned char pv = pred[i];
    out[i] = conf_bin(conf_clamp(conf[i]), K, Kf) >= min_bin ? pv : (unsigned char)255;
  }
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= ndw) return;
  const unsigned pv = ((const unsigned*)(pred + head))[i];
  const float* __restrict__ cw = conf + head;
  float4 cv;
  if ((((uintptr_t)cw) & 15u) == 0) {
    cv = ((const float4*)cw)[i];
  } else {
    cv.x = cw[4 * i];
    cv.y = cw[4 * i + 1];
    cv.z = cw[4 * i + 2];
    cv.w = cw[4 * i + 3];
  }
  unsigned ov = pv;
  if (conf_bin(conf_clamp(cv.x), K, Kf) < min_bin) ov |= 0x000000ffu;
  if (conf_bin(conf_clamp(cv.y), K, Kf) < min_bin) ov |= 0x0000ff00u;
  if (conf_bin(conf_clamp(cv.z), K, Kf) < min_bin) ov |= 0x00ff0000u;
  if (conf_bin(conf_clamp(cv.w), K, Kf) < min_bin) ov |= 0xff000000u;
  unsigned char* ow = out + head;
  if ((((uintptr_t)ow) & 3u) == 0) {
    ((unsigned*)ow)[i] = ov;
  } else {                                             // out does not share pred's alignment: bytes
    ow[4 * i] = (unsigned char)ov;
    ow[4 * i + 1] = (unsigned char)(ov >> 8);
    ow[4 * i + 2] = (unsigned char)(ov >> 16);
    ow[4 * i + 3] = (unsigned char)(ov >> 24);
  }
}

extern "C" int mmsa_abstain_u8(const unsigned char* pred, const float* conf, long n, int bins, int min_bin, unsigned char* out, hipStream_t stream) {
  const char* name = "abstain_u8";
  MMSA_CHECK_ARG(pred && conf && out, "%s: pred, conf and out are required", name);
  MMSA_CHECK_ARG(((uintptr_t)conf & 3u) == 0, "%s: conf must be 4-byte aligned", name);
  MMSA_CHECK_ARG(n >= 1 && n < (1l << 40), "%s: %ld pixels; 1..2^40 - 1 are supported", name, n);
  MMSA_CHECK_ARG(bins >= 1 && bins <= SEL_MAX_BINS, "%s: %d bins; 1..%d are supported", name, bins, SEL_MAX_BINS);
  MMSA_CHECK_ARG(min_bin >= 0 && min_bin <= bins, "%s: min_bin %d outside 0..%d (min_bin == bins abstains everywhere)", name, min_bin, bins);
  const long blocks = n < 1024 ? 1 : (n / 4 + 255) / 256;    // every whole dword has a lane whatever the head is; one workgroup at least, for the edge
  hipLaunchKernelGGL(abstain_u8_kernel, dim3((unsigned)blocks), dim3(256), 0, stream, pred, conf, n, bins, min_bin, out);
  MMSA_CHECK_LAUNCH("abstain_u8");
  return MMSA_OK;
}
