// The pixel body of the frame-size class-map kernels of csrc/segment.hip, included once per kernel (like the GEMM epilogues' .inc files):
//   SLIDE_EVAL 0: slide_argmax_kernel, statement for statement what it always was;
//   SLIDE_EVAL 1: slide_argmax_eval_kernel -- the pixel's (label class, predicted class) pair also goes into the workgroup's LDS histogram
//                 `hist` (csrc/eval_hist.h; `ev` = the label side, `lut_s` = its LUT in LDS) and the map is written only when `out` is given.
//   SLIDE_CONF 1: slide_argmax_conf_kernel (with SLIDE_EVAL 0) -- the probability of the predicted class also goes to `conf` float [B, H, W]: the softmax of
//                 csrc/softmax_px.h over the pixel's averaged logits, whose maximum m is `best`, so that its numerator is expf(m - m).  The sum of the
//                 exponentials needs m first, hence a SECOND pass over the classes that recomputes acc / cnt (the same operations on the same inputs, the
//                 same bits): no LDS, no limit on C beyond the map's.  An uncovered pixel (map 255) gets 0.
//   SLIDE_CONF 2: slide_argmax_conf_lds_kernel -- the same, but the first pass keeps the pixel's values in the per-lane LDS column conf_col[c * 256], as
//                 aug_argmax_kernel does, and the second pass reads them back: the faster form (segment.hip has the figures), for C * 256 floats <= 64 KiB.
//   SLIDE_TEMP 1: (with SLIDE_CONF 1 / 2) slide_argmax_conf_t_kernel / slide_argmax_conf_lds_t_kernel -- the confidence of softmax(x / T): the exponentials are
//                 softmax_px_exp_t with the launch's inverse temperature `it`; the map does not depend on it.  SLIDE_TEMP 0: softmax_px_exp, no `it` in scope.
//   SLIDE_SCORE 1 / 2: (with SLIDE_EVAL 0, SLIDE_CONF 0, SLIDE_TEMP 0; not defined = 0) slide_argmax_score_kernel / slide_argmax_score_lds_kernel -- an uncertainty
//                 score of csrc/softmax_px.h (`kind`: top-2 margin or entropy score, `ilc` = 1 / log C for the latter) goes to `conf` in the confidence's place,
//                 formed from the probabilities p_c = e_c / s of softmax(x * it) (`it` always given: the product is exact at 1.0f), which need s first: hence a
//                 THIRD pass over the classes.  1: both later passes recompute acc / cnt, any C the map allows.  2: the per-lane LDS column of SLIDE_CONF 2;
//                 the sum pass overwrites x_c with e_c, so the third pass calls no expf.  An uncovered pixel (map 255) gets 0.
//   SLIDE_TOPK 1 / 2: (with every other switch 0; not defined = 0) slide_argmax_topk_kernel<S> / slide_argmax_topk_lds_kernel<S> -- the pixel's first K classes
//                 and their probabilities (csrc/softmax_px.h, TopkPx<S>) go to the rank-major planes `out` uint8 / `conf` float [K, B, H, W] (`plane` = B * H * W):
//                 the map's own store writes plane 0 of the classes, the rank list the rest.  The three passes of SLIDE_SCORE 1 / 2 with topk_px_class in
//                 score_px_class's place.  An uncovered pixel gets 255 / 0 at every rank.  In scope beside SLIDE_SCORE's: S, K, plane (no kind, no ilc).
// SLIDE_Y is the pixel's row: blockIdx.y in the first kernel, the row variable of the second kernel's loop over its workgroup's rows.
// SLIDE_EXIT leaves the body: `return` in the first kernel, `continue` with the next row in the second, which still has its histogram to flush.
// SLIDE_EXIT MUST NOT be used inside a loop of this body: there `continue` would go on with that loop in the second kernel only, where `return`
// leaves the first (every use below is at the body's top level).  In scope: logits, C, hs, ws, out, H, W, hc, wc, rh, rw, wt, uncovered (and conf; with SLIDE_SCORE also
// kind, it, ilc).
// A kernel defines SLIDE_Y, SLIDE_EXIT and the switches it turns on (one not defined = 0) in front of the #include; the file undefines all of them at its end.
#ifndef SLIDE_EVAL
#define SLIDE_EVAL 0
#endif
#ifndef SLIDE_CONF
#define SLIDE_CONF 0
#endif
#ifndef SLIDE_TEMP
#define SLIDE_TEMP 0
#endif
#ifndef SLIDE_SCORE
#define SLIDE_SCORE 0
#endif
#ifndef SLIDE_TOPK
#define SLIDE_TOPK 0
#endif
#if SLIDE_TEMP
#define SLIDE_EXP(v, m) softmax_px_exp_t(v, m, it)
#else
#define SLIDE_EXP(v, m) softmax_px_exp(v, m)
#endif
// float acc = class c's sum over the pixel's covering windows, in window order, of bilinear(logits_k)[c]: the first window WRITES (0 + v == v), later ones add
#define SLIDE_WINDOW_SUM(acc, c)                                                                                                         \
  float acc = 0.f;                                                                                                                       \
  _Pragma("unroll") for (int q = 0; q < 8; ++q) {                                                                                        \
    if (q < nk) {                                                                                                                        \
      const float* sp = logits + ((long)kk[q] * C + c) * hs * ws;                                                                        \
      const float lh = lhs[q], lw = lws[q];                                                                                              \
      const float v = (1.f - lh) * ((1.f - lw) * sp[o00[q]] + lw * sp[o01[q]]) + lh * ((1.f - lw) * sp[o10[q]] + lw * sp[o11[q]]);       \
      acc = q == 0 ? v : acc + v;                                                                                                        \
    }                                                                                                                                    \
  }
  const int x = blockIdx.x * 256 + threadIdx.x, y = SLIDE_Y, b = blockIdx.z;
  if (x >= W) SLIDE_EXIT;
#if SLIDE_EVAL
  int ebin = -1;                                // row offset of the pixel's label class in the histogram, -1 = ignored
  {
    const int ys = ev.ymap ? min(max(ev.ymap[y], 0), ev.Hl - 1) : y, xs = ev.xmap ? min(max(ev.xmap[x], 0), ev.Wl - 1) : x;
    const int l = lut_s[ev.label[((long)b * ev.Hl + ys) * ev.Wl + xs]];
    if (l != MMSA_EVAL_IGNORE) ebin = min(l, C) * (C + 1);
  }
#endif
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
#if SLIDE_EVAL
    if (out) out[((long)b * H + y) * W + x] = 255;
    eval_hist_add(hist, ebin < 0 ? -1 : ebin + C, 1u);     // class 255 counts under pred index C
#else
    out[((long)b * H + y) * W + x] = 255;
#endif
#if SLIDE_CONF || SLIDE_SCORE
    conf[((long)b * H + y) * W + x] = 0.f;
#endif
#if SLIDE_TOPK
    topk_px_store_none(out, conf, plane, ((long)b * H + y) * W + x, K, 1);
#endif
    SLIDE_EXIT;
  }
  const float cnt = (float)nk;
  float best = -INFINITY;
  int bi = 0;
  for (int c = 0; c < C; ++c) {
    SLIDE_WINDOW_SUM(acc, c)
    const float p = acc / cnt;
#if SLIDE_CONF == 2 || SLIDE_SCORE == 2 || SLIDE_TOPK == 2
    conf_col[c * 256] = p;
#endif
    if (c == 0 || p > best) { best = p; bi = c; }
  }
#if SLIDE_EVAL
  if (out) out[((long)b * H + y) * W + x] = (unsigned char)bi;
  eval_hist_add(hist, ebin < 0 ? -1 : ebin + bi, 1u);
#else
  out[((long)b * H + y) * W + x] = (unsigned char)bi;
#endif
#if SLIDE_CONF == 2
  float s = 0.f;
  for (int c = 0; c < C; ++c) s = softmax_px_sum(s, SLIDE_EXP(conf_col[c * 256], best), c == 0);
  conf[((long)b * H + y) * W + x] = softmax_px_prob(SLIDE_EXP(best, best), s);
#elif SLIDE_CONF
  float s = 0.f;
  for (int c = 0; c < C; ++c) {
    SLIDE_WINDOW_SUM(acc, c)
    s = softmax_px_sum(s, SLIDE_EXP(acc / cnt, best), c == 0);
  }
  conf[((long)b * H + y) * W + x] = softmax_px_prob(SLIDE_EXP(best, best), s);      // e_c / s at the first maximum: the largest probability
#endif
#if SLIDE_SCORE == 2
  float s = 0.f;
  for (int c = 0; c < C; ++c) {
    const float e = softmax_px_exp_t(conf_col[c * 256], best, it);
    conf_col[c * 256] = e;
    s = softmax_px_sum(s, e, c == 0);
  }
  float sa = 0.f, spb = 0.f;
  bool snone = true;
  for (int c = 0; c < C; ++c) score_px_class(kind, bi, c, softmax_px_prob(conf_col[c * 256], s), sa, spb, snone);
  conf[((long)b * H + y) * W + x] = score_px_finish(kind, sa, spb, snone, ilc);
#elif SLIDE_SCORE
  float s = 0.f, sa = 0.f, spb = 0.f;
  bool snone = true;
  for (int pass = 0; pass < 2; ++pass)      // 0: the sum of the exponentials; 1: the probabilities, class by class, into the score
    for (int c = 0; c < C; ++c) {
      SLIDE_WINDOW_SUM(acc, c)
      const float e = softmax_px_exp_t(acc / cnt, best, it);
      if (pass == 0) s = softmax_px_sum(s, e, c == 0);
      else score_px_class(kind, bi, c, softmax_px_prob(e, s), sa, spb, snone);
    }
  conf[((long)b * H + y) * W + x] = score_px_finish(kind, sa, spb, snone, ilc);
#endif
#if SLIDE_TOPK == 2
  float s = 0.f;
  for (int c = 0; c < C; ++c) {
    const float e = softmax_px_exp_t(conf_col[c * 256], best, it);
    conf_col[c * 256] = e;
    s = softmax_px_sum(s, e, c == 0);
  }
  TopkPx<S> tk;
  topk_px_init(tk);
  for (int c = 0; c < C; ++c) topk_px_class(tk, bi, c, softmax_px_prob(conf_col[c * 256], s));
  topk_px_store(tk, out, conf, plane, ((long)b * H + y) * W + x, K, 1);
#elif SLIDE_TOPK
  float s = 0.f;
  TopkPx<S> tk;
  topk_px_init(tk);
  for (int pass = 0; pass < 2; ++pass)      // 0: the sum of the exponentials; 1: the probabilities, class by class, into the rank list
    for (int c = 0; c < C; ++c) {
      SLIDE_WINDOW_SUM(acc, c)
      const float e = softmax_px_exp_t(acc / cnt, best, it);
      if (pass == 0) s = softmax_px_sum(s, e, c == 0);
      else topk_px_class(tk, bi, c, softmax_px_prob(e, s));
    }
  topk_px_store(tk, out, conf, plane, ((long)b * H + y) * W + x, K, 1);
#endif
#undef SLIDE_WINDOW_SUM
#undef SLIDE_EXP
#undef SLIDE_TOPK
#undef SLIDE_EVAL
#undef SLIDE_CONF
#undef SLIDE_TEMP
#undef SLIDE_SCORE
#undef SLIDE_Y
#undef SLIDE_EXIT
