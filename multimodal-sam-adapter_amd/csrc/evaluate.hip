// Evaluation on device: the confusion counts of a uint8 class map against a uint8 label map -- everything the reference's `dataset.pre_eval`
// -> `intersect_and_union` (segmentation/mmseg_custom/datasets/DELIVER.py:219-259, apis/evaluation/metrics_micro.py:26-86) does with a prediction:
//   label_map / reduce_zero_label / ignore_index (metrics_micro.py:66-74) are one 256-byte LUT applied to the raw label byte;
//   the nearest-neighbour label resize of `Resize_multimodal._resize_seg` (datasets/pipelines/transform.py:1169-1188) is a pair of per-axis source
//   index tables (the label is read at [ymap[y], xmap[x]], clamped into the label map whatever the tables hold);
//   the four histograms follow from counts[label class][pred class] (csrc/eval_hist.h).
// The walk over (pred, label) is the one of csrc/eval_walk.h, EVAL_CHUNK pixels per workgroup, into the workgroup's private LDS histogram; its non-zero
// bins are then added to the int64 counts.
#include "common.h"
#include "eval_walk.h"

#ifndef EVAL_CHUNK
#define EVAL_CHUNK 8192      // pixels per workgroup: 32 per lane, so that the flush (at most (C + 1)^2 atomics, usually a few dozen) is amortised
#endif

// Same-bin merging.  Class maps are patchy: a lane whose four pixels share a bin makes one add of 4, merged across the wave by eval_hist_add's
// broadcast rounds; the pixels of any other lane (edges, noise) are plain LDS atomics.
struct EvalConfusion {
  static constexpr bool CONF = false;
  unsigned* hist;
  const unsigned char* lut_s;
  int C;

  using Px = int;                                                                // the pixel's bin, or -1: ignored label / no pixel
  __device__ __forceinline__ int none() const { return -1; }
  __device__ __forceinline__ int pixel(unsigned label_byte, unsigned pred_byte, float) const { return eval_bin(lut_s, label_byte, pred_byte, C); }
  __device__ __forceinline__ bool edge_lanes(int) const { return true; }
  __device__ __forceinline__ void add1(int bin) const { eval_hist_add(hist, bin, 1u); }
  __device__ __forceinline__ void add4(bool has, unsigned lv, unsigned pv, float4) const {
    int b0 = -1, b1 = -1, b2 = -1, b3 = -1;
    if (has) {
      b0 = eval_bin(lut_s, lv, pv & 255u, C);
      b1 = eval_bin(lut_s, lv >> 8, (pv >> 8) & 255u, C);
      b2 = eval_bin(lut_s, lv >> 16, (pv >> 16) & 255u, C);
      b3 = eval_bin(lut_s, lv >> 24, pv >> 24, C);
    }
    const bool uni = b0 >= 0 && b0 == b1 && b1 == b2 && b2 == b3;                // four pixels of one patch: one add of 4, merged across the wave
    eval_hist_add(hist, uni ? b0 : -1, 4u);
    if (!uni) {
      if (b0 >= 0) atomicAdd(&hist[b0], 1u);
      if (b1 >= 0) atomicAdd(&hist[b1], 1u);
      if (b2 >= 0) atomicAdd(&hist[b2], 1u);
      if (b3 >= 0) atomicAdd(&hist[b3], 1u);
    }
  }
};

template <bool TABLES>
__global__ __launch_bounds__(256) void eval_confusion_kernel(const unsigned char* __restrict__ pred, int H, int W, EvalLabel ev, EvalSlots es, int rows) {
  extern __shared__ unsigned eval_lds[];
  const int C = ev.C, nbins = (C + 1) * (C + 1);
  unsigned* hist = eval_lds;
  unsigned char* lut_s = (unsigned char*)(eval_lds + nbins);
  eval_hist_init(hist, lut_s, ev.lut, nbins);
  const EvalWalkArgs a = {pred, nullptr, ev.label, ev.lut, ev.ymap, ev.xmap, ev.counts, H, W, ev.Hl, ev.Wl, C, 0};
  const int b = blockIdx.y;
  eval_walk<TABLES, EVAL_CHUNK>(a, b, rows, EvalConfusion{hist, lut_s, C});
  eval_hist_flush(hist, ev.counts + (long)es.s[b] * nbins, nbins);
}

extern "C" int mmsa_eval_confusion_u8(const unsigned char* pred, const unsigned char* label, int B, int H, int W, int Hl, int Wl, const unsigned char* lut,
                                      int C, const int* ymap, const int* xmap, const int* slots /* HOST [B] */, int n_slots, int64_t* counts,
                                      hipStream_t stream) {
  MMSA_CHECK_ARG(pred, "eval_confusion_u8: pred is required");
  EvalSlots es;
  int rc = eval_check("eval_confusion_u8", label, B, H, W, Hl, Wl, lut, C, ymap, xmap, slots, n_slots, counts, es);
  if (rc) return rc;
  const EvalLabel ev = {label, lut, ymap, xmap, (unsigned long long*)counts, Hl, Wl, C};
  const size_t lds = (size_t)(C + 1) * (C + 1) * 4 + 256;
  eval_walk_launch(eval_confusion_kernel<true>, eval_confusion_kernel<false>, ymap != NULL, EVAL_CHUNK, B, H, W, 1, lds, stream, pred, H, W, ev, es);
  MMSA_CHECK_LAUNCH("eval_confusion_u8");
  return MMSA_OK;
}
