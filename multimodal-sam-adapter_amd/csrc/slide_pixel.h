// The pixel of the frame-size class-map kernels of csrc/segment.hip, written once: slide_pixel<WRITE, LDS, TEMP, S, EVAL>.  A kernel is a signature and one call.
//   set-up      the pixel's covering windows (at most 8 slots) and their 4-tap coordinates; a pixel under no window or more than 8 gets 255, is counted in
//               `uncovered`, and leaves;
//   first pass  preds[c] = (sum over the covering windows, in window order, of bilinear(logits_k)[c]) / count, the first maximum `best` at class `bi`,
//               and the map's store;
//   tail        (WRITE other than PX_MAP) the softmax of csrc/softmax_px.h over the same values, whose maximum is `best`: the sum of the exponentials needs
//               `best` first, the probabilities need the sum, so the classes are walked again -- the sum pass for every output, the probability pass
//               behind it for a score or the ranks (the confidence is one probability, e(best) / s).
// WRITE: what the pixel writes beside the map.
//   PX_MAP    nothing.
//   PX_CONF   the probability of the predicted class, softmax_px_prob(e(best), s), to conf float [B, H, W]; TEMP: e = softmax_px_exp_t with the launch's
//             inverse temperature `it` (the confidence of softmax(x / T)), else softmax_px_exp.  0 for a 255 pixel.
//   PX_SCORE  an uncertainty score (`kind`: top-2 margin or entropy score, `ilc` = 1 / log C for the latter) in the confidence's place, from the probabilities
//             p_c = e_c / s through score_px_class / score_px_finish.  TEMP always: the product with it == 1.0f is exact.  0 for a 255 pixel.
//   PX_TOPK   the pixel's first K classes and their probabilities to the rank-major planes out uint8 / conf float [K, B, H, W] (`plane` = B * H * W), through
//             TopkPx<S>, topk_px_class and topk_px_store: the map's own store is plane 0 of the classes.  TEMP always.  255 / 0 at every rank for a 255 pixel.
// LDS: where the tail takes a class's value from.  false: it recomputes acc / cnt from the slots (the same operations on the same inputs, the same bits): no
//   LDS, any C the map allows.  true: the first pass keeps the values in the per-lane column conf_col[c * 256] (private to the lane: no barrier), C * 256 floats
//   of dynamic LDS; with two tail passes the sum pass overwrites x_c with e_c, so the probability pass calls no expf.
// EVAL (with PX_MAP): the pixel's (label class, predicted class) pair also goes into the workgroup's LDS histogram `hist` (csrc/eval_hist.h; `ev` = the label
//   side, `lut_s` = its LUT in LDS), and the map is written only when `out` is given.  The caller still has the histogram to flush behind a barrier, which the
//   lanes with x >= W and the 255 pixels must reach too: leaving the pixel is this function's `return`, never the kernel's.  eval_hist_add votes across the
//   lanes that are active at the call: the lanes of a 255 pixel at the first call, the lanes with a class at the second.
// `y` is the pixel's row; x and the image come from the launch grid (blockIdx.x * 256 + threadIdx.x, blockIdx.z).
// Include it AFTER `#pragma clang fp contract(off)`, slide_taps.h (WindowTable), softmax_px.h and eval_hist.h.
#pragma once

enum { PX_MAP, PX_CONF, PX_SCORE, PX_TOPK };

template <int WRITE, bool LDS = false, bool TEMP = false, int S = 2, bool EVAL = false>
__device__ __forceinline__ void slide_pixel(const float* __restrict__ logits, int C, int hs, int ws, unsigned char* __restrict__ out, float* __restrict__ conf,
                                            int H, int W, int hc, int wc, float rh, float rw, const WindowTable& wt, int* __restrict__ uncovered, int y,
                                            float* conf_col = nullptr, float it = 1.f, int kind = 0, float ilc = 0.f, int K = 0, long plane = 0,
                                            unsigned* hist = nullptr, const unsigned char* lut_s = nullptr, const EvalLabel* ev = nullptr) {
  static_assert(WRITE == PX_MAP || !EVAL, "the fused evaluation launch writes the map alone");
  static_assert(WRITE == PX_MAP ? !LDS && !TEMP : WRITE == PX_CONF || TEMP, "the score and the ranks are always formed with the inverse temperature");
  // Every launcher refuses C <= 0.  Saying so leaves the class loops without a guard of their own, so the compiler forms the 32 tap addresses once, in front
  // of the first pass, for every pass; behind separate guards it formed them again per loop and kept their 64-bit ingredients alive in between: 192
  // registers in the recomputing forms against 118 - 127 (profiles/slide_pixel_template_isa.txt).
  __builtin_assume(C > 0);
  const int x = blockIdx.x * 256 + threadIdx.x, b = blockIdx.z;
  if (x >= W) return;
  const long op = ((long)b * H + y) * W + x;
  int ebin = -1;                                // EVAL: row offset of the pixel's label class in the histogram, -1 = ignored
  if constexpr (EVAL) {
    const int ys = ev->ymap ? min(max(ev->ymap[y], 0), ev->Hl - 1) : y, xs = ev->xmap ? min(max(ev->xmap[x], 0), ev->Wl - 1) : x;
    const int l = lut_s[ev->label[((long)b * ev->Hl + ys) * ev->Wl + xs]];
    if (l != MMSA_EVAL_IGNORE) ebin = min(l, C) * (C + 1);
  }
  // covering windows (at most 8 per pixel) and their 4-tap coordinates (PyTorch upsample_bilinear2d: src = (dst + 0.5) * in/out - 0.5,
  // clamped at 0).  The slot arrays are only ever indexed by unrolled constants (predicated inserts), so they live in registers.
  int nk = 0, kk[8], o00[8], o01[8], o10[8], o11[8];
  float lhs[8], lws[8];
#pragma unroll
  for (int q = 0; q < 8; ++q) { kk[q] = 0; o00[q] = o01[q] = o10[q] = o11[q] = 0; lhs[q] = lws[q] = 0.f; }
  for (int k = 0; k < wt.n; ++k) {
    if (wt.b[k] != b) continue;
    const int i = y - wt.y0[k], j = x - wt.x0[k];
    if (i < 0 || i >= hc || j < 0 || j >= wc) continue;
    float sh = ((float)i + 0.5f) * rh - 0.5f, sw = ((float)j + 0.5f) * rw - 0.5f;
    sh = sh < 0.f ? 0.f : sh;
    sw = sw < 0.f ? 0.f : sw;
    const int h0 = min((int)sh, hs - 1), w0 = min((int)sw, ws - 1);
    const int h1 = h0 + (h0 < hs - 1 ? 1 : 0), w1 = w0 + (w0 < ws - 1 ? 1 : 0);
#pragma unroll
    for (int q = 0; q < 8; ++q)
      if (q == nk) {
        kk[q] = k; lhs[q] = sh - (float)h0; lws[q] = sw - (float)w0;
        o00[q] = h0 * ws + w0; o01[q] = h0 * ws + w1; o10[q] = h1 * ws + w0; o11[q] = h1 * ws + w1;
      }
    ++nk;
  }
  if (nk == 0 || nk > 8) {   // no window, or more than 8 overlapping windows per pixel: not supported -- counted, and the pixel gets 255, never an unwritten byte
    atomicAdd(uncovered, 1);
    if (!EVAL || out) out[op] = 255;
    if constexpr (EVAL) eval_hist_add(hist, ebin < 0 ? -1 : ebin + C, 1u);     // class 255 counts under pred index C
    if constexpr (WRITE == PX_CONF || WRITE == PX_SCORE) conf[op] = 0.f;
    if constexpr (WRITE == PX_TOPK) topk_px_store_none(out, conf, plane, op, K, 1);
    return;
  }
  const float cnt = (float)nk;
  // class c's average over the pixel's covering windows, in window order, of bilinear(logits_k)[c]: the first window WRITES (0 + v == v), later ones add
  auto value = [&](int c) {
    float acc = 0.f;
#pragma unroll
    for (int q = 0; q < 8; ++q) {
      if (q < nk) {
        const float* sp = logits + ((long)kk[q] * C + c) * hs * ws;
        const float lh = lhs[q], lw = lws[q];
        const float v = (1.f - lh) * ((1.f - lw) * sp[o00[q]] + lw * sp[o01[q]]) + lh * ((1.f - lw) * sp[o10[q]] + lw * sp[o11[q]]);
        acc = q == 0 ? v : acc + v;
      }
    }
    return acc / cnt;
  };
  float best = -INFINITY;
  int bi = 0;
  for (int c = 0; c < C; ++c) {
    const float p = value(c);
    if constexpr (LDS) conf_col[c * 256] = p;
    if (c == 0 || p > best) { best = p; bi = c; }      // first maximum wins, like torch.argmax on ties
  }
  if (!EVAL || out) out[op] = (unsigned char)bi;
  if constexpr (EVAL) eval_hist_add(hist, ebin < 0 ? -1 : ebin + bi, 1u);
  if constexpr (WRITE != PX_MAP) {
    auto expo = [&](float v) {
      if constexpr (TEMP) return softmax_px_exp_t(v, best, it);
      else return softmax_px_exp(v, best);
    };
    constexpr bool KEEP = LDS && WRITE != PX_CONF;      // the sum pass leaves e_c in the column for the probability pass
    float s = 0.f;
    for (int c = 0; c < C; ++c) {      // the sum of the exponentials
      const float e = expo(LDS ? conf_col[c * 256] : value(c));
      if constexpr (KEEP) conf_col[c * 256] = e;
      s = softmax_px_sum(s, e, c == 0);
    }
    float sa = 0.f, spb = 0.f;
    bool snone = true;
    TopkPx<S> tk;
    topk_px_init(tk);
    if constexpr (WRITE != PX_CONF)
      for (int c = 0; c < C; ++c) {      // the probabilities, class by class, into the score or the rank list
        const float p = softmax_px_prob(KEEP ? conf_col[c * 256] : expo(value(c)), s);
        if constexpr (WRITE == PX_SCORE) score_px_class(kind, bi, c, p, sa, spb, snone);
        else topk_px_class(tk, bi, c, p);
      }
    if constexpr (WRITE == PX_CONF) conf[op] = softmax_px_prob(expo(best), s);      // e_c / s at the first maximum: the largest probability
    if constexpr (WRITE == PX_SCORE) conf[op] = score_px_finish(kind, sa, spb, snone, ilc);
    if constexpr (WRITE == PX_TOPK) topk_px_store(tk, out, conf, plane, op, K, 1);
  }
}
