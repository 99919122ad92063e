// Confusion counts of a class map against a label map, shared by csrc/evaluate.hip (the standalone pass) and csrc/segment.hip (the pass fused
// into the class-map kernel).  What the reference computes per image on the host (segmentation/mmseg_custom/apis/evaluation/metrics_micro.py:26-86,
// `intersect_and_union`: three torch.histc calls on the masked maps) is ONE matrix here:
//   counts[slot][l][p], int64 [C + 1, C + 1]: l = transformed label class, p = predicted class; index C = "outside [0, C) and not ignored",
//   the values torch.histc(min=0, max=C-1) drops from ONE of its histograms only.  Ignored pixels are counted nowhere.
// Every workgroup keeps a private uint32 histogram in LDS ((C + 1)^2 * 4 bytes; a workgroup never sees 2^32 pixels), and adds only its non-zero
// bins to the int64 counts with 64-bit vector atomics: integer sums, so the result does not depend on the order of arrival.
#pragma once
#include "common.h"

#define MMSA_EVAL_MAX_CLASSES 126     // (126 + 1)^2 * 4 = 64516 bytes: the largest histogram inside the 64 KiB of LDS a launch may ask for
#define MMSA_EVAL_IGNORE 255          // LUT code "ignored"; 0 .. C - 1 = class, C = kept but out of range (any other code counts as C)
#define MMSA_EVAL_MAX_IMAGES 64

struct EvalSlots { int s[MMSA_EVAL_MAX_IMAGES]; };     // image -> count slot, by value in the launch arguments (like WindowTable)

struct EvalLabel {                    // the label side of a launch
  const unsigned char* label;         // [B, Hl, Wl]
  const unsigned char* lut;           // [256]
  const int* ymap;                    // [H] / [W] source row / column of the nearest-neighbour resize, or both NULL (Hl == H, Wl == W)
  const int* xmap;
  unsigned long long* counts;         // [n_slots, C + 1, C + 1]
  int Hl, Wl, C;
};

__device__ __forceinline__ void eval_hist_init(unsigned* hist, unsigned char* lut_s, const unsigned char* lut, int nbins) {
  for (int i = threadIdx.x; i < nbins; i += blockDim.x) hist[i] = 0u;
  for (int i = threadIdx.x; i < 256; i += blockDim.x) lut_s[i] = lut[i];
  __syncthreads();
}

// bin of one pixel, or -1 when its label is ignored
__device__ __forceinline__ int eval_bin(const unsigned char* lut_s, unsigned label_byte, unsigned pred_byte, int C) {
  const int l = lut_s[label_byte & 255u];
  if (l == MMSA_EVAL_IGNORE) return -1;
  return min(l, C) * (C + 1) + min((int)pred_byte, C);
}

// Add `weight` to hist[bin] for every lane with bin >= 0.  Class maps are made of uniform patches: most lanes of a wave hold the SAME bin, and 64
// LDS atomics on one address are served one after the other.  Two rounds first: the lowest pending lane's bin is broadcast, every lane that holds
// it retires, and one lane adds their number; what is left (edges, noise) goes lane by lane.  `weight` must be the same in all lanes.  The ballots see
// the lanes that are active at the call, so a call inside divergent code merges among those.
__device__ __forceinline__ void eval_hist_add(unsigned* hist, int bin, unsigned weight) {
  bool pending = bin >= 0;
#pragma unroll
  for (int r = 0; r < 2; ++r) {
    const unsigned long long m = __ballot(pending);
    if (m == 0ull) return;
    const int lead = __ffsll((long long)m) - 1;
    const int lb = __shfl(bin, lead, 64);
    const bool same = pending && bin == lb;
    const unsigned long long ms = __ballot(same);
    if ((int)(threadIdx.x & 63u) == lead) atomicAdd(&hist[lb], weight * (unsigned)__popcll(ms));
    pending = pending && !same;
  }
  if (pending) atomicAdd(&hist[bin], weight);
}

__device__ __forceinline__ void eval_hist_flush(const unsigned* hist, unsigned long long* dst, int nbins) {
  __syncthreads();
  for (int i = threadIdx.x; i < nbins; i += blockDim.x) {
    const unsigned v = hist[i];
    if (v) atomicAdd(&dst[i], (unsigned long long)v);
  }
}

// host: the label-side arguments of every entry, checked before anything is launched; `max_classes` and its reason `why` are the entry's own (the
// histogram's LDS for the passes that keep one)
static inline int eval_check(const char* name, const unsigned char* label, int B, int H, int W, int Hl, int Wl, const unsigned char* lut, int C,
                             const int* ymap, const int* xmap, const int* slots, int n_slots, const int64_t* counts, EvalSlots& es,
                             int max_classes = MMSA_EVAL_MAX_CLASSES,
                             const char* why = "the (C + 1)^2 uint32 histogram of a workgroup must fit 64 KiB of LDS") {
  MMSA_CHECK_ARG(label && lut && slots && counts, "%s: label, lut, slots and counts are required", name);
  MMSA_CHECK_ARG(C >= 2 && C <= max_classes, "%s: %d classes; 2..%d are supported (%s)", name, C, max_classes, why);
  MMSA_CHECK_ARG(B > 0 && B <= MMSA_EVAL_MAX_IMAGES, "%s: 1..%d images per call, got %d", name, MMSA_EVAL_MAX_IMAGES, B);
  MMSA_CHECK_ARG(H > 0 && W > 0 && Hl > 0 && Wl > 0 && (long)H * W < (1l << 31) && (long)Hl * Wl < (1l << 31), "%s: bad map size", name);
  MMSA_CHECK_ARG((ymap != NULL) == (xmap != NULL), "%s: ymap and xmap come together", name);
  MMSA_CHECK_ARG(ymap || (Hl == H && Wl == W), "%s: size mismatch: the label is %d x %d, the prediction %d x %d, and no ymap / xmap tables were given",
                 name, Hl, Wl, H, W);
  MMSA_CHECK_ARG(n_slots > 0, "%s: n_slots must be positive", name);
  for (int b = 0; b < B; ++b) {
    MMSA_CHECK_ARG(slots[b] >= 0 && slots[b] < n_slots, "%s: slots[%d] = %d outside the %d count slots", name, b, slots[b], n_slots);
    es.s[b] = slots[b];
  }
  return MMSA_OK;
}
