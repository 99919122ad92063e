// Top-k evaluation on device: at which rank of a top-k class map (csrc/segment.hip: classes uint8 [K, B, H, W], rank-major) the label's class stands.
//   counts[slot][l][r], int64 [n_slots, C, K + 1]: l = the transformed label class, r = the first rank whose class byte equals l, K = none of the K does.
// The label side is mmsa_eval_confusion_u8's, verbatim (csrc/eval_hist.h, csrc/evaluate.hip): the 256-byte LUT, the nearest-neighbour source tables clamped into
// the label map, the slot table.  A pixel takes part iff l is a class (l < C): ignored labels and kept labels outside [0, C) are counted nowhere, so row l sums
// to row l of the confusion matrix of plane 0, and column r is the diagonal of the confusion matrix of plane r.  The cumulative column sums over the
// participating pixels are the top-1 .. top-K pixel accuracies.
// A workgroup walks a flat run of TOPK_EVAL_CHUNK pixels of one image into its private uint32 LDS histogram [C, K + 1] (a cell holds at most the chunk: no
// overflow) and adds the non-zero cells to the int64 counts with 64-bit atomics: integer sums, the same bytes run after run.
#include "common.h"
#include "eval_hist.h"

#define TOPK_EVAL_MAX_RANKS 8
#define TOPK_EVAL_MAX_CLASSES 255     // the class byte 255 is "no class at this rank"; 255 * 9 * 4 + 256 bytes of LDS at the most
#ifndef TOPK_EVAL_CHUNK
#define TOPK_EVAL_CHUNK 8192          // pixels per workgroup: 32 per lane, so that the flush (at most C * (K + 1) atomics, usually a few dozen) is amortised
#endif

template <bool TABLES>
__global__ __launch_bounds__(256) void eval_topk_kernel(const unsigned char* __restrict__ classes, int K, long plane, int H, int W, EvalLabel ev, EvalSlots es) {
  extern __shared__ unsigned eval_lds[];
  const int C = ev.C, nbins = C * (K + 1);
  unsigned* hist = eval_lds;
  unsigned char* lut_s = (unsigned char*)(eval_lds + nbins);
  eval_hist_init(hist, lut_s, ev.lut, nbins);
  const int b = blockIdx.y, HW = H * W;
  const int start = blockIdx.x * TOPK_EVAL_CHUNK, n = min(TOPK_EVAL_CHUNK, HW - start);      // H * W < 2^31 (eval_check), start < H * W
  const unsigned char* cp = classes + (long)b * HW;
  const unsigned char* lp = ev.label + (long)b * ev.Hl * ev.Wl;
  for (int o = 0; o < n; o += 256) {      // every lane makes every trip: eval_hist_add merges across the wave
    const int k = o + (int)threadIdx.x, i = start + min(k, n - 1);
    int bin = -1;
    if (k < n) {
      int ls = i;
      if (TABLES) {
        const int y = i / W, x = i - y * W;
        ls = min(max(ev.ymap[y], 0), ev.Hl - 1) * ev.Wl + min(max(ev.xmap[x], 0), ev.Wl - 1);
      }
      const int l = lut_s[lp[ls]];
      if (l < C) {      // MMSA_EVAL_IGNORE = 255 and the "kept but out of range" codes are >= C
        int r = K;
        for (int q = K - 1; q >= 0; --q)
          if (cp[q * plane + i] == l) r = q;
        bin = l * (K + 1) + r;
      }
    }
    eval_hist_add(hist, bin, 1u);
  }
  eval_hist_flush(hist, ev.counts + (long)es.s[b] * nbins, nbins);
}

extern "C" int mmsa_eval_topk_u8(const unsigned char* classes, int K, const unsigned char* label, int B, int H, int W, int Hl, int Wl, const unsigned char* lut,
                                 int C, const int* ymap, const int* xmap, const int* slots /* HOST [B] */, int n_slots, int64_t* counts, hipStream_t stream) {
  MMSA_CHECK_ARG(classes, "eval_topk_u8: classes is required");
  MMSA_CHECK_ARG(K >= 1 && K <= TOPK_EVAL_MAX_RANKS, "eval_topk_u8: K = %d; 1..%d ranks are supported", K, TOPK_EVAL_MAX_RANKS);
  EvalSlots es;
  int rc = eval_check("eval_topk_u8", label, B, H, W, Hl, Wl, lut, C, ymap, xmap, slots, n_slots, counts, es, TOPK_EVAL_MAX_CLASSES,
                      "255 is the byte of a rank without a class");
  if (rc) return rc;
  const EvalLabel ev = {label, lut, ymap, xmap, (unsigned long long*)counts, Hl, Wl, C};
  const size_t lds = (size_t)C * (K + 1) * 4 + 256;
  const long HW = (long)H * W, plane = (long)B * HW;
  const dim3 grid(cdiv(HW, TOPK_EVAL_CHUNK), B);
  if (ymap) hipLaunchKernelGGL(eval_topk_kernel<true>, grid, dim3(256), lds, stream, classes, K, plane, H, W, ev, es);
  else hipLaunchKernelGGL(eval_topk_kernel<false>, grid, dim3(256), lds, stream, classes, K, plane, H, W, ev, es);
  MMSA_CHECK_LAUNCH("eval_topk_u8");
  return MMSA_OK;
}
