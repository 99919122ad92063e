// The pixel body of the two rescaled class-map kernels of csrc/segment.hip, included once per kernel (as slide_pixel.inc is):
//   RESIZED_CONF 0: slide_argmax_resized_kernel, statement for statement what it always was;
//   RESIZED_CONF 1: slide_argmax_resized_conf_kernel -- the probability of the predicted class also goes to `conf` float [B, Hcut, Wcut] (0 for a 255 pixel),
//                   by a second pass over the classes in the form the first one took (slots or scanning), for the reason slide_pixel.inc gives.
// In scope: logits, C, hs, ws, out, H, W, hc, wc, rh, rw, Hcut, Wcut, rh2, rw2, wt, uncovered (and conf).
  const int X = blockIdx.x * 256 + threadIdx.x, Y = blockIdx.y, b = blockIdx.z;
  if (X >= Wcut) return;
  // second stage: the taps of output pixel (Y, X) in the H x W canvas (bilinear_accum_kernel with src = the canvas)
  float sh2 = ((float)Y + 0.5f) * rh2 - 0.5f, sw2 = ((float)X + 0.5f) * rw2 - 0.5f;
  sh2 = sh2 < 0.f ? 0.f : sh2;
  sw2 = sw2 < 0.f ? 0.f : sw2;
  const int y0 = min((int)sh2, H - 1), x0 = min((int)sw2, W - 1);
  const int y1 = y0 + (y0 < H - 1 ? 1 : 0), x1 = x0 + (x0 < W - 1 ? 1 : 0);
  const float lh2 = sh2 - (float)y0, lw2 = sw2 - (float)x0;
  // first stage: the covering windows of each tap (tap t: row y0 / y1 = t >> 1, column x0 / x1 = t & 1).  Slot arrays only ever indexed by unrolled constants.
  TapSlots tp[4];
#pragma unroll
  for (int t = 0; t < 4; ++t) {
    tp[t].nk = 0;
#pragma unroll
    for (int q = 0; q < RESIZED_SLOTS; ++q) { tp[t].o[q] = tp[t].kf[q] = 0; tp[t].lh[q] = tp[t].lw[q] = 0.f; }
  }
  for (int k = 0; k < wt.n; ++k) {
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      int o, kf;
      float lh, lw;
      if (!tap_coords(wt, k, b, t >> 1 ? y1 : y0, t & 1 ? x1 : x0, hc, wc, hs, ws, rh, rw, o, kf, lh, lw)) continue;
#pragma unroll
      for (int q = 0; q < RESIZED_SLOTS; ++q)
        if (q == tp[t].nk) { tp[t].o[q] = o; tp[t].kf[q] = kf; tp[t].lh[q] = lh; tp[t].lw[q] = lw; }
      ++tp[t].nk;
    }
  }
  const int nmin = min(min(tp[0].nk, tp[1].nk), min(tp[2].nk, tp[3].nk)), nmax = max(max(tp[0].nk, tp[1].nk), max(tp[2].nk, tp[3].nk));
  const long op = ((long)b * Hcut + Y) * Wcut + X;
  if (nmin == 0 || nmax > 8) {      // a tap without a window, or with more than 8: counted once per output pixel, and the pixel gets 255
    atomicAdd(uncovered, 1);
    out[op] = 255;
#if RESIZED_CONF
    conf[op] = 0.f;
#endif
    return;
  }
  float best = -INFINITY;
  int bi = 0;
  if (nmax <= RESIZED_SLOTS) {
    for (int c = 0; c < C; ++c) {
      const float p00 = tap_value(tp[0], logits, C, c, hs, ws), p01 = tap_value(tp[1], logits, C, c, hs, ws);
      const float p10 = tap_value(tp[2], logits, C, c, hs, ws), p11 = tap_value(tp[3], logits, C, c, hs, ws);
      const float p = (1.f - lh2) * ((1.f - lw2) * p00 + lw2 * p01) + lh2 * ((1.f - lw2) * p10 + lw2 * p11);
      if (c == 0 || p > best) { best = p; bi = c; }
    }
  } else {
    for (int c = 0; c < C; ++c) {
      const float p00 = tap_value_scan(wt, b, y0, x0, tp[0].nk, logits, C, c, hs, ws, hc, wc, rh, rw);
      const float p01 = tap_value_scan(wt, b, y0, x1, tp[1].nk, logits, C, c, hs, ws, hc, wc, rh, rw);
      const float p10 = tap_value_scan(wt, b, y1, x0, tp[2].nk, logits, C, c, hs, ws, hc, wc, rh, rw);
      const float p11 = tap_value_scan(wt, b, y1, x1, tp[3].nk, logits, C, c, hs, ws, hc, wc, rh, rw);
      const float p = (1.f - lh2) * ((1.f - lw2) * p00 + lw2 * p01) + lh2 * ((1.f - lw2) * p10 + lw2 * p11);
      if (c == 0 || p > best) { best = p; bi = c; }
    }
  }
  out[op] = (unsigned char)bi;
#if RESIZED_CONF
  // the second pass of slide_pixel.inc at this size: the same values again, now that their maximum `best` is known
  float s = 0.f;
  if (nmax <= RESIZED_SLOTS) {
    for (int c = 0; c < C; ++c) {
      const float p00 = tap_value(tp[0], logits, C, c, hs, ws), p01 = tap_value(tp[1], logits, C, c, hs, ws);
      const float p10 = tap_value(tp[2], logits, C, c, hs, ws), p11 = tap_value(tp[3], logits, C, c, hs, ws);
      const float p = (1.f - lh2) * ((1.f - lw2) * p00 + lw2 * p01) + lh2 * ((1.f - lw2) * p10 + lw2 * p11);
      s = softmax_px_sum(s, softmax_px_exp(p, best), c == 0);
    }
  } else {
    for (int c = 0; c < C; ++c) {
      const float p00 = tap_value_scan(wt, b, y0, x0, tp[0].nk, logits, C, c, hs, ws, hc, wc, rh, rw);
      const float p01 = tap_value_scan(wt, b, y0, x1, tp[1].nk, logits, C, c, hs, ws, hc, wc, rh, rw);
      const float p10 = tap_value_scan(wt, b, y1, x0, tp[2].nk, logits, C, c, hs, ws, hc, wc, rh, rw);
      const float p11 = tap_value_scan(wt, b, y1, x1, tp[3].nk, logits, C, c, hs, ws, hc, wc, rh, rw);
      const float p = (1.f - lh2) * ((1.f - lw2) * p00 + lw2 * p01) + lh2 * ((1.f - lw2) * p10 + lw2 * p11);
      s = softmax_px_sum(s, softmax_px_exp(p, best), c == 0);
    }
  }
  conf[op] = softmax_px_prob(softmax_px_exp(best, best), s);
#endif
