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
// Include it AFTER `#pragma clang fp contract(off)`.
#pragma once

__device__ __forceinline__ float softmax_px_max(float m, float x) { return x > m ? x : m; }
__device__ __forceinline__ float softmax_px_exp(float x, float m) { return expf(x - m); }
__device__ __forceinline__ float softmax_px_exp_t(float x, float m, float it) { return expf((x - m) * it); }
__device__ __forceinline__ float softmax_px_sum(float s, float e, bool first) { return first ? e : s + e; }
__device__ __forceinline__ float softmax_px_prob(float e, float s) { return e / s; }
__device__ __forceinline__ float softmax_px_accum(float acc, float p, bool first) { return first ? p : acc + p; }
__device__ __forceinline__ float softmax_px_mean(float acc, int A) { return acc / (float)A; }
