// Evaluation on device: the confusion counts of a uint8 class map against a uint8 label map -- everything the reference's `dataset.pre_eval`
// -> `intersect_and_union` (segmentation/mmseg_custom/datasets/DELIVER.py:219-259, apis/evaluation/metrics_micro.py:26-86) does with a prediction:
//   label_map / reduce_zero_label / ignore_index (metrics_micro.py:66-74) are one 256-byte LUT applied to the raw label byte;
//   the nearest-neighbour label resize of `Resize_multimodal._resize_seg` (datasets/pipelines/transform.py:1169-1188) is a pair of per-axis source
//   index tables (the label is read at [ymap[y], xmap[x]], clamped into the label map whatever the tables hold);
//   the four histograms follow from counts[label class][pred class] (csrc/eval_hist.h).
// One pass over 2 bytes per pixel, HBM-bound: a workgroup walks EVAL_CHUNK pixels (several rows), pred -- and the label where no table is in the way
// and its alignment matches -- read as dwords, into its private LDS histogram, then adds its non-zero bins to the int64 counts.
#include "common.h"
#include "eval_hist.h"

#define EVAL_CHUNK 8192      // pixels per workgroup: 32 per lane, so that the flush (at most (C + 1)^2 atomics, usually a few dozen) is amortised

template <bool TABLES>
__device__ __forceinline__ unsigned eval_label_at(const unsigned char* __restrict__ l, const int* __restrict__ xmap, int Wl, int i) {
  if (TABLES) return l[min(max(xmap[i], 0), Wl - 1)];
  return l[i];
}

// n pixels: pred p[0..n) against label l[0..n) (TABLES: l[xmap[0..n)], a label ROW)
template <bool TABLES>
__device__ __forceinline__ void eval_span(const unsigned char* __restrict__ p, const unsigned char* __restrict__ l, const int* __restrict__ xmap, int Wl,
                                          int n, unsigned* hist, const unsigned char* lut_s, int C) {
  const int head = min(n, (int)((4u - (unsigned)((uintptr_t)p & 3u)) & 3u));     // bytes in front of the first aligned pred dword
  const int ndw = (n - head) >> 2;
  const int tail0 = head + (ndw << 2);
  const int nedge = head + (n - tail0);                                          // edge path: at most 3 + 3 pixels, one lane each
  {
    int bin = -1;
    if ((int)threadIdx.x < nedge) {
      const int i = (int)threadIdx.x < head ? (int)threadIdx.x : tail0 + ((int)threadIdx.x - head);
      bin = eval_bin(lut_s, eval_label_at<TABLES>(l, xmap, Wl, i), p[i], C);
    }
    eval_hist_add(hist, bin, 1u);
  }
  const unsigned* __restrict__ pw = (const unsigned*)(p + head);
  const bool ldw = !TABLES && (((uintptr_t)(l + head)) & 3u) == 0;               // the label shares pred's alignment: dwords too
  for (int i0 = 0; i0 < ndw; i0 += 256) {
    const int i = i0 + (int)threadIdx.x;
    int b0 = -1, b1 = -1, b2 = -1, b3 = -1;
    if (i < ndw) {
      const unsigned pv = pw[i];
      const int base = head + 4 * i;
      unsigned lv;
      if (ldw)
        lv = ((const unsigned*)(l + head))[i];
      else
        lv = eval_label_at<TABLES>(l, xmap, Wl, base) | (eval_label_at<TABLES>(l, xmap, Wl, base + 1) << 8) |
             (eval_label_at<TABLES>(l, xmap, Wl, base + 2) << 16) | (eval_label_at<TABLES>(l, xmap, Wl, base + 3) << 24);
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
}

template <bool TABLES>
__global__ __launch_bounds__(256) void eval_confusion_kernel(const unsigned char* __restrict__ pred, int H, int W, EvalLabel ev, EvalSlots es, int rows) {
  extern __shared__ unsigned eval_lds[];
  const int C = ev.C, nbins = (C + 1) * (C + 1);
  unsigned* hist = eval_lds;
  unsigned char* lut_s = (unsigned char*)(eval_lds + nbins);
  eval_hist_init(hist, lut_s, ev.lut, nbins);
  const int b = blockIdx.y;
  if (TABLES) {
    const int y1 = min(H, ((int)blockIdx.x + 1) * rows);
    for (int y = (int)blockIdx.x * rows; y < y1; ++y) {
      const int ys = min(max(ev.ymap[y], 0), ev.Hl - 1);
      eval_span<true>(pred + ((long)b * H + y) * W, ev.label + ((long)b * ev.Hl + ys) * ev.Wl, ev.xmap, ev.Wl, W, hist, lut_s, C);
    }
  } else {                                          // same size: image b is one run of H * W byte pairs
    const long HW = (long)H * W, start = (long)blockIdx.x * EVAL_CHUNK;
    const int n = (int)min((long)EVAL_CHUNK, HW - start);
    eval_span<false>(pred + b * HW + start, ev.label + b * HW + start, nullptr, 0, n, hist, lut_s, C);
  }
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
  if (ymap) {
    const int rows = max(1, cdiv(EVAL_CHUNK, W));
    hipLaunchKernelGGL(HIP_KERNEL_NAME(eval_confusion_kernel<true>), dim3(cdiv(H, rows), B), dim3(256), lds, stream, pred, H, W, ev, es, rows);
  } else {
    hipLaunchKernelGGL(HIP_KERNEL_NAME(eval_confusion_kernel<false>), dim3(cdiv((long)H * W, (long)EVAL_CHUNK), B), dim3(256), lds, stream, pred, H, W, ev, es, 0);
  }
  MMSA_CHECK_LAUNCH("eval_confusion_u8");
  return MMSA_OK;
}
