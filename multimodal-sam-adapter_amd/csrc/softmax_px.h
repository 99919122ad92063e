// The per-pixel softmax over the class axis and the mean over the views of an augmented frame, stated ONCE: what EncoderDecoder.inference does to the
// logits (F.softmax(seg_logit, dim=1), ED:449,460) and what aug_test does to the probabilities of its views (seg_logit += cur; seg_logit /= len(imgs),
// ED:538-541).  Both kernels of csrc/augment.hip are made of these pieces and nothing else, so the canvas path and the one-pass class map round alike:
//   m   = max_c x_c                               softmax_px_max, in class order from m = x_0
//   e_c = expf(x_c - m)                           softmax_px_exp  (ocml's expf, not the hardware approximation: it is the same instruction sequence wherever it is inlined)
//   e_c = expf((x_c - m) * it)                    softmax_px_exp_t: the softmax of x / T, `it` = float32(1 / float64(T)) made on the host (mmsa.evaluate.inv_temperature);
//                                                 ONE float32 product behind the subtraction, no contraction.  With it == 1.0f the product is exact, so a
//                                                 tempered kernel is bit for bit its untempered sibling; max, sum and division do not change, and the
//                                                 confidence is softmax_px_prob(softmax_px_exp_t(m, m, it), s)
//   s   = e_0; s += e_c for c = 1 .. C-1          softmax_px_sum, in class order
//   p_c = e_c / s                                 softmax_px_prob
//   acc_c = p_c (first view) | acc_c + p_c        softmax_px_accum, in view order
//   acc_c / (float)A  after the last view         softmax_px_mean -- kept although it does not change the argmax of exact values: it can round two distinct
//                                                 sums to the same float, and the first class must then win, as in the reference
// The two uncertainty scores of a pixel beside its confidence p[bi] (bi = the class the map names), stated ONCE as well: both are formed from the float32
// probabilities p_c above (one view: softmax_px_prob(e_c, s); several views: softmax_px_mean), so that the one-pass kernels and the canvas kernel
// (argmax_score_nchw_kernel of csrc/segment.hip, which READS p_c) perform the same operations and agree bit for bit:
//   kind 1, top-2 margin:   p[bi] - p2, p2 = the largest p_c over c != bi in class order with `>`; ONE float32 subtraction; C == 1: p[bi]
//   kind 2, entropy score:  max(0, 1 - H * ilc), H = sum_c (p_c > 0 ? -(p_c * logf(p_c)) : 0) in class order from the first term (ocml's logf, as expf
//                           above), `ilc` = float32(1 / log(float64(C))) made on the host (mmsa.evaluate.inv_log_classes), 0 for C == 1 (score 1)
// Higher = more certain, in [0, 1], as the confidence is.  score_px_class is one class's step (class order), score_px_finish the pixel's score.
// The top-K of a pixel, 1 <= K <= 8, stated ONCE too: the first K classes of the pixel and their float32 probabilities p_c above -- comparisons and moves only,
// no arithmetic, so every path that forms the same p_c names the same classes and writes the same bits:
//   rank 0      = bi, the class the map names, with p[bi] (so plane 0 of the classes IS the map and plane 0 of the probabilities IS the confidence);
//   rank r >= 1 = among the classes not yet ranked the one with the largest p_c, the lowest class index among equal values: classes come in class order and
//                 one moves ahead of a ranked class only with `>`, as score_px_second does (rank 1's probability is its p2);
//   rank r >= C = class 255 with probability 0; a pixel whose map byte is 255 gets 255 / 0 at every rank.
// TopkPx<S> is the rank list, S = 2 / 4 / 8 slots >= K, indexed by unrolled constants only (predicated inserts: it stays in registers); an empty slot is
// class 255 with "probability" -1, which every p_c >= 0 beats.  topk_px_init, then topk_px_class once per class in class order, then topk_px_store.
// Include it AFTER `#pragma clang fp contract(off)`.
#pragma once

__device__ __forceinline__ float softmax_px_max(float m, float x) { return x > m ? x : m; }
__device__ __forceinline__ float softmax_px_exp(float x, float m) { return expf(x - m); }
__device__ __forceinline__ float softmax_px_exp_t(float x, float m, float it) { return expf((x - m) * it); }
__device__ __forceinline__ float softmax_px_sum(float s, float e, bool first) { return first ? e : s + e; }
__device__ __forceinline__ float softmax_px_prob(float e, float s) { return e / s; }
__device__ __forceinline__ float softmax_px_accum(float acc, float p, bool first) { return first ? p : acc + p; }
__device__ __forceinline__ float softmax_px_mean(float acc, int A) { return acc / (float)A; }

#define SCORE_MARGIN 1
#define SCORE_ENTROPY 2
__device__ __forceinline__ float score_px_second(float p2, float p, bool first) { return first || p > p2 ? p : p2; }
__device__ __forceinline__ float score_px_margin(float pb, float p2) { return pb - p2; }
__device__ __forceinline__ float score_px_h_term(float p) { return p > 0.f ? -(p * logf(p)) : 0.f; }
__device__ __forceinline__ float score_px_h_sum(float h, float t, bool first) { return first ? t : h + t; }
__device__ __forceinline__ float score_px_entropy(float h, float ilc) {
  const float v = 1.f - h * ilc;
  return v > 0.f ? v : 0.f;
}
// class c of the pixel, probability p: `a` is p2 (kind 1) or H (kind 2) so far, `pb` becomes p[bi], `none` = no class other than bi seen yet
__device__ __forceinline__ void score_px_class(int kind, int bi, int c, float p, float& a, float& pb, bool& none) {
  if (c == bi) pb = p;
  if (kind == SCORE_MARGIN) {
    if (c != bi) { a = score_px_second(a, p, none); none = false; }
  } else {
    a = score_px_h_sum(a, score_px_h_term(p), c == 0);
  }
}
__device__ __forceinline__ float score_px_finish(int kind, float a, float pb, bool none, float ilc) {
  if (kind == SCORE_MARGIN) return none ? pb : score_px_margin(pb, a);
  return score_px_entropy(a, ilc);
}

#define TOPK_MAX 8
#define TOPK_NONE 255
template <int S>
struct TopkPx {
  float p[S];
  int c[S];
};
template <int S>
__device__ __forceinline__ void topk_px_init(TopkPx<S>& t) {
#pragma unroll
  for (int q = 0; q < S; ++q) { t.p[q] = -1.f; t.c[q] = TOPK_NONE; }
}
// class c of the pixel, probability p: bi takes slot 0 whatever its value; any other class goes in front of the first slot of 1 .. S-1 it beats with `>`, and
// the slots from there on move one down (the last one drops out).  Slot q is rewritten before slot q - 1, so each move reads a value not yet overwritten.
// Written as selects on the values, never as a store under a branch: the compiler merges two such stores into ONE store through a selected address, and a
// rank list addressed at run time goes to scratch.
template <int S>
__device__ __forceinline__ void topk_px_class(TopkPx<S>& t, int bi, int c, float p) {
  const bool is = c == bi;
  t.p[0] = is ? p : t.p[0];
  t.c[0] = is ? c : t.c[0];
#pragma unroll
  for (int q = S - 1; q >= 1; --q) {
    const bool in = !is && p > t.p[q];                             // c stands at slot q or in front of it
    const bool here = q == 1 || !(p > t.p[q - 1]);                 // ... at slot q
    t.p[q] = in ? (here ? p : t.p[q - 1]) : t.p[q];
    t.c[q] = in ? (here ? c : t.c[q - 1]) : t.c[q];
  }
}
// ranks r0 .. K-1 of the classes (r0 = 1 where the map's own store has written plane 0) and 0 .. K-1 of the probabilities go to pixel i of their planes
template <int S>
__device__ __forceinline__ void topk_px_store(const TopkPx<S>& t, unsigned char* classes, float* probs, long plane, long i, int K, int r0) {
#pragma unroll
  for (int q = 0; q < S; ++q)
    if (q < K) {
      if (q >= r0) classes[q * plane + i] = (unsigned char)t.c[q];
      probs[q * plane + i] = t.c[q] == TOPK_NONE ? 0.f : t.p[q];
    }
}
// the pixel without a class (map byte 255): 255 / 0 at ranks r0 .. K-1 / 0 .. K-1
__device__ __forceinline__ void topk_px_store_none(unsigned char* classes, float* probs, long plane, long i, int K, int r0) {
  for (int r = 0; r < K; ++r) {
    if (r >= r0) classes[r * plane + i] = TOPK_NONE;
    probs[r * plane + i] = 0.f;
  }
}
