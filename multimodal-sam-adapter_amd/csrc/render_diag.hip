// Diagnostic pictures on device: the ground truth, the wrong pixels, a heat map of any float32 score, the abstained pixels and the boundary band, each
// made the way show_result makes its picture (csrc/render.hip): every pixel gets ONE paint chosen by a rule, then the blend of csrc/render_px.h.
//
// The paint table.  uint32 entries staged in LDS: bits 0..23 the colour in the picture's channel order (c0 | c1 << 8 | c2 << 16), bit 24 PAINT (0 = the
// pixel is the source pixel unchanged, black without a source), bit 25 MARK (the blend uses (mark_opacity, 1 - mark_opacity) in the place of
// (opacity, 1 - opacity)).  The caller packs the table (mmsa/render.py); a kernel computes only an INDEX into it:
//   labels     L < C ? L : C                                                       table [C + 1]         L = the label code of csrc/boundary.hip: a class < C,
//   errors     L == 255 ? 0 : (L < C && pred == L ? 1 + pred : 257 + (wrong_by_label ? L : pred))   [513]      C (kept, out of range) or 255 (ignored)
//   heat       k                                                                   table [bins]          k = conf_bin(conf_clamp(v), bins, (float)bins) of
//   abstained  k >= min_bin ? pred : 256 + k                                       table [256 + bins]        csrc/conf_bin.h, verbatim
//   band       marked ? (mark_by_label ? L : P) : 256 + (inside_by_label ? L : P)  table [512]           P = min(pred, C)
// Two kernels.  The POINTWISE kernel (labels / errors, heat / abstained) walks like render_kernel: a lane owns 4 consecutive pixels of a row -- pred and
// the label as one dword, the values as one float4, the raw frame as three dwords or the tensor as three float4, the 12 output bytes as three dwords --
// where all of them are aligned, and goes pixel by pixel elsewhere (output rows are 3 * w bytes: the alignment changes from row to row unless
// w % 4 == 0); a workgroup covers 1024 pixels of one row.  With label tables the label is read at [ymap[y], xmap[x]], clamped into the label map.
// The STENCIL kernel (band) is eval_boundary_kernel with the histogram replaced by the paint lookup and the 12-byte store: the same tile + halo of codes
// in LDS and the row pass / column pass of csrc/boundary_px.h, so near_pred / near_label are that kernel's, bit for bit.  A missing map (band takes pred,
// labels or both) is staged as code 0 everywhere and its passes are skipped.  Nothing outside any array is read or written.
#include "common.h"
#include "render_px.h"
#include "boundary_px.h"
#include "conf_bin.h"

#define DIAG_PAINT (1u << 24)
#define DIAG_MARK (1u << 25)
#define DIAG_TAB_MAX 513              // the errors table, the largest
#define DIAG_IGNORE 255               // MMSA_EVAL_IGNORE of csrc/eval_hist.h: the LUT code "ignored"
#define DIAG_MAX_CLASSES 254          // a LUT holds a class < C, C or 255
#define DIAG_BAND_MAX_CLASSES 253     // codes <= C must differ from the row pass's "mixed" byte 0xFE
#define DIAG_MAX_BINS 256

enum { DIAG_LABELS = 0, DIAG_ERRORS = 1 };                 // `mode` of the label kind
enum { DIAG_KIND_LABEL = 0, DIAG_KIND_VALUE = 1 };

struct DiagTab { const unsigned* tab; int n; double om, op, mom, mop; };                 // (1 - opacity, opacity) and the MARKED pair
struct DiagSrc { const void* p; int Cs, Hs, Ws, rev; RenderDenorm dn; };                 // the source of the picture: RAW uint8 [B, Hs, Ws, 3] / TENSOR float32 [B, Cs, Hs, Ws]
struct DiagLabel { const unsigned char* label; const unsigned char* lut; const int* ymap; const int* xmap; int Hl, Wl, C; };
struct DiagPoint {                                                                      // the index side of the pointwise kernel
  const unsigned char* pred; long pbs, prs;
  const float* val;
  DiagLabel lb;
  int mode, wrong_by_label, bins, min_bin;
};
struct DiagBand { const unsigned char* pred; long pbs, prs; DiagLabel lb; int H, W, r, border, TH, rows, cols, pdw, tiles_x, where, mark_by_label, inside_by_label; };

struct DiagSrcAt { const unsigned char* sr; const float* st; long plane; };

template <int SRC>
__device__ __forceinline__ DiagSrcAt diag_src_at(const DiagSrc& s, int b, int y, int x) {
  DiagSrcAt a = {nullptr, nullptr, 0};
  if (SRC == RENDER_RAW) a.sr = (const unsigned char*)s.p + (((long)b * s.Hs + y) * s.Ws + x) * 3;
  if (SRC == RENDER_TENSOR) {
    a.plane = (long)s.Hs * s.Ws;
    a.st = (const float*)s.p + (long)b * s.Cs * a.plane + (long)y * s.Ws + x;
  }
  return a;
}

template <int SRC>
__device__ __forceinline__ bool diag_src_aligned(const DiagSrcAt& a) {
  if (SRC == RENDER_RAW) return (((uintptr_t)a.sr) & 3u) == 0;
  if (SRC == RENDER_TENSOR) return ((((uintptr_t)a.st) | ((uintptr_t)(a.plane * 4))) & 15u) == 0;
  return true;
}

// four source pixels from aligned addresses, packed c0 | c1 << 8 | c2 << 16
template <int SRC>
__device__ __forceinline__ void diag_src_load4(const DiagSrcAt& a, const DiagSrc& s, unsigned px[4]) {
  px[0] = px[1] = px[2] = px[3] = 0u;
  if (SRC == RENDER_RAW) {
    const unsigned* wv = (const unsigned*)a.sr;
    const unsigned w0 = wv[0], w1 = wv[1], w2 = wv[2];
    px[0] = w0 & 0xffffffu;
    px[1] = (w0 >> 24) | ((w1 & 0xffffu) << 8);
    px[2] = (w1 >> 16) | ((w2 & 255u) << 16);
    px[3] = w2 >> 8;
    if (s.rev) {
#pragma unroll
      for (int q = 0; q < 4; ++q) px[q] = render_swap02(px[q]);
    }
  }
  if (SRC == RENDER_TENSOR) {
    const float4 u = *(const float4*)a.st, g = *(const float4*)(a.st + a.plane), c = *(const float4*)(a.st + 2 * a.plane);
    px[0] = render_denorm(u.x, g.x, c.x, s.dn);
    px[1] = render_denorm(u.y, g.y, c.y, s.dn);
    px[2] = render_denorm(u.z, g.z, c.z, s.dn);
    px[3] = render_denorm(u.w, g.w, c.w, s.dn);
  }
}

template <int SRC>
__device__ __forceinline__ unsigned diag_src_load1(const DiagSrcAt& a, const DiagSrc& s, int q) {
  unsigned v = 0u;
  if (SRC == RENDER_RAW) {
    v = (unsigned)a.sr[3 * q] | ((unsigned)a.sr[3 * q + 1] << 8) | ((unsigned)a.sr[3 * q + 2] << 16);
    if (s.rev) v = render_swap02(v);
  }
  if (SRC == RENDER_TENSOR) v = render_denorm(a.st[q], a.st[a.plane + q], a.st[2 * a.plane + q], s.dn);
  return v;
}

// the paint rule: a table entry over a source pixel
__device__ __forceinline__ unsigned diag_paint(unsigned src, unsigned e, const DiagTab& t) {
  if (!(e & DIAG_PAINT)) return src;
  const bool m = (e & DIAG_MARK) != 0;
  return render_pixel(src, e, m ? t.mom : t.om, m ? t.mop : t.op);
}

__device__ __forceinline__ void diag_store4(unsigned char* o, unsigned q0, unsigned q1, unsigned q2, unsigned q3) {
  unsigned* ow = (unsigned*)o;
  ow[0] = q0 | (q1 << 24);
  ow[1] = (q1 >> 8) | (q2 << 16);
  ow[2] = (q2 >> 16) | (q3 << 8);
}

__device__ __forceinline__ void diag_store1(unsigned char* o, int q, unsigned v) {
  o[3 * q] = (unsigned char)(v & 255u);
  o[3 * q + 1] = (unsigned char)((v >> 8) & 255u);
  o[3 * q + 2] = (unsigned char)((v >> 16) & 255u);
}

// the label code of a LUT value: a class < C, C, or 255
__device__ __forceinline__ int diag_code(int l, int C) { return l == DIAG_IGNORE ? DIAG_IGNORE : min(l, C); }

__device__ __forceinline__ int diag_label_index(int L, int p, const DiagPoint& a) {
  const int C = a.lb.C;
  if (a.mode == DIAG_LABELS) return L < C ? L : C;
  if (L == DIAG_IGNORE) return 0;
  if (L < C && p == L) return 1 + p;
  return 257 + (a.wrong_by_label ? L : p);
}

__device__ __forceinline__ int diag_value_index(float v, int p, bool has_pred, const DiagPoint& a) {
  const int k = conf_bin(conf_clamp(v), a.bins, (float)a.bins);
  if (!has_pred) return k;
  return k >= a.min_bin ? p : 256 + k;
}

// grid (cdiv(w, 1024), h, B)
template <int KIND, int SRC>
__global__ __launch_bounds__(256) void diag_point_kernel(DiagPoint a, DiagTab t, DiagSrc s, unsigned char* __restrict__ out, int h, int w) {
  __shared__ unsigned tab[DIAG_TAB_MAX];
  __shared__ unsigned char lut_s[256];
  for (int i = threadIdx.x; i < t.n; i += 256) tab[i] = t.tab[i];
  if (KIND == DIAG_KIND_LABEL) lut_s[threadIdx.x] = a.lb.lut[threadIdx.x];
  __syncthreads();
  const int x = ((int)blockIdx.x * 256 + (int)threadIdx.x) * 4;
  if (x >= w) return;
  const int y = blockIdx.y, b = blockIdx.z;
  const int nvalid = min(4, w - x);
  unsigned char* o = out + (((long)b * h + y) * w + x) * 3;
  const DiagSrcAt sa = diag_src_at<SRC>(s, b, y, x);
  const bool has_pred = a.pred != nullptr;
  const unsigned char* p = has_pred ? a.pred + (long)b * a.pbs + (long)y * a.prs + x : nullptr;
  bool vec = nvalid == 4 && (((uintptr_t)o) & 3u) == 0 && diag_src_aligned<SRC>(sa) && (((uintptr_t)p) & 3u) == 0;
  const unsigned char* lrow = nullptr;
  const float* v = nullptr;
  bool tables = false;
  if (KIND == DIAG_KIND_LABEL) {
    tables = a.lb.ymap != nullptr;
    const int ys = tables ? min(max(a.lb.ymap[y], 0), a.lb.Hl - 1) : y;
    lrow = a.lb.label + ((long)b * a.lb.Hl + ys) * a.lb.Wl;
    if (!tables) vec = vec && (((uintptr_t)(lrow + x)) & 3u) == 0;
  } else {
    v = a.val + ((long)b * h + y) * w + x;
    vec = vec && (((uintptr_t)v) & 15u) == 0;
  }
  if (vec) {
    const unsigned pv = has_pred ? *(const unsigned*)p : 0u;
    int idx[4];
    if (KIND == DIAG_KIND_LABEL) {
      unsigned lv;
      if (tables) {
        lv = 0u;
#pragma unroll
        for (int q = 0; q < 4; ++q) lv |= (unsigned)lrow[min(max(a.lb.xmap[x + q], 0), a.lb.Wl - 1)] << (8 * q);
      } else {
        lv = *(const unsigned*)(lrow + x);
      }
#pragma unroll
      for (int q = 0; q < 4; ++q) idx[q] = diag_label_index(diag_code(lut_s[(lv >> (8 * q)) & 255u], a.lb.C), (int)((pv >> (8 * q)) & 255u), a);
    } else {
      const float4 f = *(const float4*)v;
      idx[0] = diag_value_index(f.x, (int)(pv & 255u), has_pred, a);
      idx[1] = diag_value_index(f.y, (int)((pv >> 8) & 255u), has_pred, a);
      idx[2] = diag_value_index(f.z, (int)((pv >> 16) & 255u), has_pred, a);
      idx[3] = diag_value_index(f.w, (int)(pv >> 24), has_pred, a);
    }
    unsigned px[4];
    diag_src_load4<SRC>(sa, s, px);
    diag_store4(o, diag_paint(px[0], tab[idx[0]], t), diag_paint(px[1], tab[idx[1]], t), diag_paint(px[2], tab[idx[2]], t), diag_paint(px[3], tab[idx[3]], t));
  } else {                                                                 // edge path: pixel by pixel
#pragma unroll 1
    for (int q = 0; q < nvalid; ++q) {
      const int pq = has_pred ? (int)p[q] : 0;
      int idx;
      if (KIND == DIAG_KIND_LABEL) {
        const int xs = tables ? min(max(a.lb.xmap[x + q], 0), a.lb.Wl - 1) : x + q;
        idx = diag_label_index(diag_code(lut_s[lrow[xs]], a.lb.C), pq, a);
      } else {
        idx = diag_value_index(v[q], pq, has_pred, a);
      }
      diag_store1(o, q, diag_paint(diag_src_load1<SRC>(sa, s, q), tab[idx], t));
    }
  }
}

static inline size_t diag_band_lds_bytes(int r) {
  return ((size_t)512 + (size_t)2 * (bnd_tile_h(r) + 2 * r) * (bnd_pitch_dw(r) + BND_TILE_W / 4)) * 4 + 256;      // radius 32: 2048 + 37632 + 256 bytes
}

// grid (tiles, B), dynamic LDS: the table [512], the staged codes and the row-pass bytes of both maps (as in eval_boundary_kernel), the LUT
template <int SRC>
__global__ __launch_bounds__(256) void diag_band_kernel(DiagBand g, DiagTab t, DiagSrc s, unsigned char* __restrict__ out) {
  extern __shared__ unsigned diag_lds[];
  const int C = g.lb.C, r = g.r, rows = g.rows, pdw = g.pdw, H = g.H, W = g.W;
  constexpr int RDW = BND_TILE_W / 4;
  unsigned* tab = diag_lds;
  unsigned* stL = tab + 512;                    // staged codes [rows][pdw dwords], label / prediction
  unsigned* stP = stL + rows * pdw;
  unsigned* rpL = stP + rows * pdw;             // row-pass bytes [rows][16 dwords]
  unsigned* rpP = rpL + rows * RDW;
  unsigned char* lut_s = (unsigned char*)(rpP + rows * RDW);
  const bool has_pred = g.pred != nullptr, has_label = g.lb.label != nullptr;
  for (int i = threadIdx.x; i < 512; i += 256) tab[i] = t.tab[i];
  lut_s[threadIdx.x] = has_label ? g.lb.lut[threadIdx.x] : (unsigned char)0;
  __syncthreads();
  const int b = blockIdx.y;
  const int ty = (int)blockIdx.x / g.tiles_x, tx = (int)blockIdx.x - ty * g.tiles_x;
  const int y0 = ty * g.TH, x0 = tx * BND_TILE_W;

  // 1. stage the codes of tile + halo, clamp-to-edge: a wave per staged row, a lane per column (64 + 2 r <= 128: two columns per lane at the most)
  {
    const bool tables = has_label && g.lb.ymap != nullptr;
    const int lx = threadIdx.x & 63, ly = threadIdx.x >> 6, pitch = pdw * 4;
    const unsigned char* pp = has_pred ? g.pred + (long)b * g.pbs : nullptr;
    const unsigned char* lp = has_label ? g.lb.label + (long)b * g.lb.Hl * g.lb.Wl : nullptr;
    unsigned char* bL = (unsigned char*)stL;
    unsigned char* bP = (unsigned char*)stP;
    int xc[2], xs[2];
#pragma unroll
    for (int q = 0; q < 2; ++q) {
      xc[q] = min(max(x0 - r + lx + 64 * q, 0), W - 1);
      xs[q] = tables ? min(max(g.lb.xmap[xc[q]], 0), g.lb.Wl - 1) : xc[q];
    }
    for (int sy = ly; sy < rows; sy += 4) {
      const int yc = min(max(y0 - r + sy, 0), H - 1);
      const int ys = tables ? min(max(g.lb.ymap[yc], 0), g.lb.Hl - 1) : yc;
#pragma unroll
      for (int q = 0; q < 2; ++q) {
        const int sx = lx + 64 * q;
        if (sx < g.cols) {
          bL[sy * pitch + sx] = (unsigned char)(has_label ? diag_code(lut_s[lp[(long)ys * g.lb.Wl + xs[q]]], C) : 0);
          bP[sy * pitch + sx] = (unsigned char)(has_pred ? min((int)pp[(long)yc * g.prs + xc[q]], C) : 0);
        }
      }
    }
  }
  __syncthreads();

  // 2. row pass over every staged row, the maps that exist
  for (int i = threadIdx.x; i < rows * RDW; i += 256) {
    const int sy = i / RDW, gx = i - sy * RDW;
    if (has_label) rpL[i] = bnd_row_pass(stL + sy * pdw + gx, r);
    if (has_pred) rpP[i] = bnd_row_pass(stP + sy * pdw + gx, r);
  }
  __syncthreads();

  // 3. column pass, the paint and the store: four pixels of a tile row per lane
  for (int i = threadIdx.x; i < g.TH * RDW; i += 256) {
    const int y = i / RDW, gx = i - y * RDW;
    const int Y = y0 + y, X = x0 + 4 * gx;
    if (Y >= H || X >= W) continue;
    const unsigned nl = has_label ? bnd_col_pass(rpL + i, r) : 0u, np = has_pred ? bnd_col_pass(rpP + i, r) : 0u;
    const bool edge_y = g.border && (Y < r || Y >= H - r);
    const unsigned char* cl = (const unsigned char*)(stL + (y + r) * pdw) + 4 * gx + r;      // the pixels' own codes
    const unsigned char* cp = (const unsigned char*)(stP + (y + r) * pdw) + 4 * gx + r;
    const int nvalid = min(4, W - X);
    unsigned e[4] = {0u, 0u, 0u, 0u};
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      if (j < nvalid) {
        const int l = cl[j], p = cp[j];
        const bool edge = edge_y || (g.border && (X + j < r || X + j >= W - r));
        const bool nlj = has_label && (((nl >> (8 * j + 7)) & 1u) != 0 || edge), npj = has_pred && (((np >> (8 * j + 7)) & 1u) != 0 || edge);
        const bool marked = (((g.where & 1) && npj) || ((g.where & 2) && nlj)) && !(has_label && l == DIAG_IGNORE);
        e[j] = tab[marked ? (g.mark_by_label ? l : p) : 256 + (g.inside_by_label ? l : p)];
      }
    }
    unsigned char* o = out + (((long)b * H + Y) * W + X) * 3;
    const DiagSrcAt sa = diag_src_at<SRC>(s, b, Y, X);
    if (nvalid == 4 && (((uintptr_t)o) & 3u) == 0 && diag_src_aligned<SRC>(sa)) {
      unsigned px[4];
      diag_src_load4<SRC>(sa, s, px);
      diag_store4(o, diag_paint(px[0], e[0], t), diag_paint(px[1], e[1], t), diag_paint(px[2], e[2], t), diag_paint(px[3], e[3], t));
    } else {
#pragma unroll 1
      for (int q = 0; q < nvalid; ++q) diag_store1(o, q, diag_paint(diag_src_load1<SRC>(sa, s, q), e[q], t));
    }
  }
}

// ---- host ----
static int diag_common_check(const char* name, int B, int h, int w, const unsigned* table, int ntab, int ntab_want, const void* src, int src_form, int Cs,
                             int Hs, int Ws, const float* mean, const float* std, double opacity, double one_minus, double mark_opacity, double one_minus_mark,
                             const unsigned char* out) {
  MMSA_CHECK_ARG(table && out, "%s: null argument (table and out are required)", name);
  MMSA_CHECK_ARG(B > 0 && B <= 65535 && h > 0 && h <= 65535 && w > 0, "%s: bad map shape [%d, %d, %d]", name, B, h, w);
  MMSA_CHECK_ARG(ntab == ntab_want, "%s: the paint table has %d entries, this picture needs %d", name, ntab, ntab_want);
  MMSA_CHECK_ARG(opacity > 0.0 && opacity <= 1.0 && one_minus >= 0.0 && one_minus < 1.0, "%s: opacity %g (1 - opacity %g) must be in (0, 1]", name, opacity,
                 one_minus);
  MMSA_CHECK_ARG(mark_opacity > 0.0 && mark_opacity <= 1.0 && one_minus_mark >= 0.0 && one_minus_mark < 1.0,
                 "%s: mark_opacity %g (1 - mark_opacity %g) must be in (0, 1]", name, mark_opacity, one_minus_mark);
  MMSA_CHECK_ARG(src_form >= RENDER_NONE && src_form <= RENDER_TENSOR, "%s: src_form = %d; 0 (none), 1 (raw uint8 frames) or 2 (normalised float32 tensor)", name,
                 src_form);
  if (src_form != RENDER_NONE) {
    MMSA_CHECK_ARG(src, "%s: src_form = %d needs src", name, src_form);
    MMSA_CHECK_ARG(Hs >= h && Ws >= w, "%s: the %d x %d source is smaller than the %d x %d map", name, Hs, Ws, h, w);
  }
  if (src_form == RENDER_TENSOR) {
    MMSA_CHECK_ARG(mean && std, "%s: null argument (mean and std are required with a float32 source)", name);
    MMSA_CHECK_ARG(Cs >= 3, "%s: the tensor has %d planes, the picture needs the first 3", name, Cs);
  }
  return MMSA_OK;
}

static int diag_pred_check(const char* name, long pbs, long prs, int B, int h, int w) {
  MMSA_CHECK_ARG(prs >= w && (B == 1 || pbs >= (long)(h - 1) * prs + w), "%s: pred strides (image %ld, row %ld) overlap for a [%d, %d, %d] map", name, pbs, prs, B,
                 h, w);
  return MMSA_OK;
}

static int diag_label_check(const char* name, const unsigned char* label, const unsigned char* lut, int h, int w, int Hl, int Wl, const int* ymap,
                            const int* xmap) {
  MMSA_CHECK_ARG(label && lut, "%s: label and lut are required", name);
  MMSA_CHECK_ARG(Hl > 0 && Wl > 0 && (long)Hl * Wl < (1l << 31), "%s: bad label map size %d x %d", name, Hl, Wl);
  MMSA_CHECK_ARG((ymap != NULL) == (xmap != NULL), "%s: ymap and xmap come together", name);
  MMSA_CHECK_ARG(ymap || (Hl == h && Wl == w), "%s: size mismatch: the label is %d x %d, the prediction %d x %d, and no ymap / xmap tables were given", name, Hl,
                 Wl, h, w);
  return MMSA_OK;
}

static DiagSrc diag_src_of(const void* src, int src_form, int Cs, int Hs, int Ws, int src_reverse, const float* mean, const float* std, int to_rgb, int mul255) {
  DiagSrc s = {};
  s.p = src_form == RENDER_NONE ? nullptr : src;
  s.Cs = Cs; s.Hs = Hs; s.Ws = Ws; s.rev = src_form == RENDER_RAW && src_reverse != 0;
  if (src_form == RENDER_TENSOR) {
    for (int c = 0; c < 3; ++c) { s.dn.mean[c] = mean[c]; s.dn.std[c] = std[c]; }
    s.dn.swap = to_rgb != 0;
    s.dn.mul255 = mul255 != 0;
  }
  return s;
}

template <int KIND>
static void diag_point_launch(int src_form, dim3 grid, hipStream_t stream, const DiagPoint& a, const DiagTab& t, const DiagSrc& s, unsigned char* out, int h,
                              int w) {
  if (src_form == RENDER_RAW) hipLaunchKernelGGL(HIP_KERNEL_NAME(diag_point_kernel<KIND, RENDER_RAW>), grid, dim3(256), 0, stream, a, t, s, out, h, w);
  else if (src_form == RENDER_TENSOR) hipLaunchKernelGGL(HIP_KERNEL_NAME(diag_point_kernel<KIND, RENDER_TENSOR>), grid, dim3(256), 0, stream, a, t, s, out, h, w);
  else hipLaunchKernelGGL(HIP_KERNEL_NAME(diag_point_kernel<KIND, RENDER_NONE>), grid, dim3(256), 0, stream, a, t, s, out, h, w);
}

extern "C" int mmsa_render_labels_u8(const unsigned char* pred, long pred_image_stride, long pred_row_stride, const unsigned char* label, int B, int h, int w,
                                     int Hl, int Wl, const unsigned char* lut, int C, const int* ymap, const int* xmap, int mode, int wrong_by_label,
                                     const unsigned* table, int ntab, const void* src, int src_form, int Cs, int Hs, int Ws, int src_reverse, const float* mean,
                                     const float* std, int to_rgb, int mul255, double opacity, double one_minus_opacity, double mark_opacity,
                                     double one_minus_mark_opacity, unsigned char* out, hipStream_t stream) {
  const char* name = "render_labels_u8";
  MMSA_CHECK_ARG(mode == DIAG_LABELS || mode == DIAG_ERRORS, "%s: mode = %d; 0 (the ground-truth picture) or 1 (the wrong-pixel picture)", name, mode);
  MMSA_CHECK_ARG(C >= 1 && C <= DIAG_MAX_CLASSES, "%s: %d classes; 1..%d are supported (a LUT byte is a class, C or 255)", name, C, DIAG_MAX_CLASSES);
  int rc = diag_common_check(name, B, h, w, table, ntab, mode == DIAG_LABELS ? C + 1 : 513, src, src_form, Cs, Hs, Ws, mean, std, opacity, one_minus_opacity,
                             mark_opacity, one_minus_mark_opacity, out);
  if (rc) return rc;
  if ((rc = diag_label_check(name, label, lut, h, w, Hl, Wl, ymap, xmap))) return rc;
  if (mode == DIAG_ERRORS) {
    MMSA_CHECK_ARG(pred, "%s: pred is required for the wrong-pixel picture", name);
    if ((rc = diag_pred_check(name, pred_image_stride, pred_row_stride, B, h, w))) return rc;
  }
  DiagPoint a = {};
  a.pred = mode == DIAG_ERRORS ? pred : nullptr;
  a.pbs = pred_image_stride; a.prs = pred_row_stride;
  a.lb = {label, lut, ymap, xmap, Hl, Wl, C};
  a.mode = mode; a.wrong_by_label = wrong_by_label != 0;
  const DiagTab t = {table, ntab, one_minus_opacity, opacity, one_minus_mark_opacity, mark_opacity};
  diag_point_launch<DIAG_KIND_LABEL>(src_form, dim3(cdiv(w, 1024), h, B), stream, a, t,
                                     diag_src_of(src, src_form, Cs, Hs, Ws, src_reverse, mean, std, to_rgb, mul255), out, h, w);
  MMSA_CHECK_LAUNCH("render_labels_u8");
  return MMSA_OK;
}

extern "C" int mmsa_render_values_f32(const float* values, const unsigned char* pred, long pred_image_stride, long pred_row_stride, int B, int h, int w, int bins,
                                      int min_bin, const unsigned* table, int ntab, const void* src, int src_form, int Cs, int Hs, int Ws, int src_reverse,
                                      const float* mean, const float* std, int to_rgb, int mul255, double opacity, double one_minus_opacity, double mark_opacity,
                                      double one_minus_mark_opacity, unsigned char* out, hipStream_t stream) {
  const char* name = "render_values_f32";
  MMSA_CHECK_ARG(values, "%s: values is required", name);
  MMSA_CHECK_ARG((((uintptr_t)values) & 3u) == 0, "%s: values must be 4-byte aligned", name);
  MMSA_CHECK_ARG(bins >= 1 && bins <= DIAG_MAX_BINS, "%s: bins = %d; 1..%d are supported (one paint per bin)", name, bins, DIAG_MAX_BINS);
  if (pred) MMSA_CHECK_ARG(min_bin >= 0 && min_bin <= bins, "%s: min_bin = %d; 0..%d for %d bins (%d abstains everywhere)", name, min_bin, bins, bins, bins);
  int rc = diag_common_check(name, B, h, w, table, ntab, pred ? 256 + bins : bins, src, src_form, Cs, Hs, Ws, mean, std, opacity, one_minus_opacity, mark_opacity,
                             one_minus_mark_opacity, out);
  if (rc) return rc;
  if (pred && (rc = diag_pred_check(name, pred_image_stride, pred_row_stride, B, h, w))) return rc;
  DiagPoint a = {};
  a.pred = pred; a.pbs = pred_image_stride; a.prs = pred_row_stride;
  a.val = values; a.bins = bins; a.min_bin = min_bin;
  const DiagTab t = {table, ntab, one_minus_opacity, opacity, one_minus_mark_opacity, mark_opacity};
  diag_point_launch<DIAG_KIND_VALUE>(src_form, dim3(cdiv(w, 1024), h, B), stream, a, t,
                                     diag_src_of(src, src_form, Cs, Hs, Ws, src_reverse, mean, std, to_rgb, mul255), out, h, w);
  MMSA_CHECK_LAUNCH("render_values_f32");
  return MMSA_OK;
}

extern "C" int mmsa_render_band_u8(const unsigned char* pred, long pred_image_stride, long pred_row_stride, const unsigned char* label, int B, int H, int W, int Hl,
                                   int Wl, const unsigned char* lut, int C, const int* ymap, const int* xmap, int radius, int border, int where,
                                   int mark_by_label, int inside_by_label, const unsigned* table, int ntab, const void* src, int src_form, int Cs, int Hs,
                                   int Ws, int src_reverse, const float* mean, const float* std, int to_rgb, int mul255, double opacity,
                                   double one_minus_opacity, double mark_opacity, double one_minus_mark_opacity, unsigned char* out, hipStream_t stream) {
  const char* name = "render_band_u8";
  MMSA_CHECK_ARG(pred || label, "%s: pred or label is required (the band of one of them, or of both)", name);
  MMSA_CHECK_ARG(radius >= 1 && radius <= BND_MAX_RADIUS, "%s: radius = %d; 1..%d are supported", name, radius, BND_MAX_RADIUS);
  MMSA_CHECK_ARG(border == 0 || border == 1, "%s: border = %d; 0 (neighbours outside the image do not exist) or 1 (the image border is a boundary)", name,
                 border);
  MMSA_CHECK_ARG(C >= 1 && C <= DIAG_BAND_MAX_CLASSES, "%s: %d classes; 1..%d are supported (the row pass marks a mixed window with the byte 0xFE)", name, C,
                 DIAG_BAND_MAX_CLASSES);
  MMSA_CHECK_ARG(where >= 1 && where <= 3, "%s: where = %d; 1 (the prediction's band), 2 (the label's) or 3 (their union)", name, where);
  MMSA_CHECK_ARG(!(where & 1) || pred, "%s: where = %d marks the prediction's band and needs pred", name, where);
  MMSA_CHECK_ARG(!(where & 2) || label, "%s: where = %d marks the label's band and needs label", name, where);
  MMSA_CHECK_ARG(label || !(mark_by_label || inside_by_label), "%s: a paint by the label's code needs label", name);
  int rc = diag_common_check(name, B, H, W, table, ntab, 512, src, src_form, Cs, Hs, Ws, mean, std, opacity, one_minus_opacity, mark_opacity,
                             one_minus_mark_opacity, out);
  if (rc) return rc;
  MMSA_CHECK_ARG((long)H * W < (1l << 31), "%s: bad map size %d x %d", name, H, W);
  if (pred && (rc = diag_pred_check(name, pred_image_stride, pred_row_stride, B, H, W))) return rc;
  if (label && (rc = diag_label_check(name, label, lut, H, W, Hl, Wl, ymap, xmap))) return rc;
  const int TH = bnd_tile_h(radius), tiles_x = cdiv(W, BND_TILE_W);
  DiagBand g = {};
  g.pred = pred; g.pbs = pred_image_stride; g.prs = pred_row_stride;
  if (label) g.lb = {label, lut, ymap, xmap, Hl, Wl, C};
  g.lb.C = C;
  g.H = H; g.W = W; g.r = radius; g.border = border;
  g.TH = TH; g.rows = TH + 2 * radius; g.cols = BND_TILE_W + 2 * radius; g.pdw = bnd_pitch_dw(radius); g.tiles_x = tiles_x;
  g.where = where; g.mark_by_label = mark_by_label != 0; g.inside_by_label = inside_by_label != 0;
  const DiagTab t = {table, ntab, one_minus_opacity, opacity, one_minus_mark_opacity, mark_opacity};
  const DiagSrc s = diag_src_of(src, src_form, Cs, Hs, Ws, src_reverse, mean, std, to_rgb, mul255);
  const dim3 grid((unsigned)tiles_x * (unsigned)cdiv(H, TH), B);
  const size_t lds = diag_band_lds_bytes(radius);
  if (src_form == RENDER_RAW) hipLaunchKernelGGL(HIP_KERNEL_NAME(diag_band_kernel<RENDER_RAW>), grid, dim3(256), lds, stream, g, t, s, out);
  else if (src_form == RENDER_TENSOR) hipLaunchKernelGGL(HIP_KERNEL_NAME(diag_band_kernel<RENDER_TENSOR>), grid, dim3(256), lds, stream, g, t, s, out);
  else hipLaunchKernelGGL(HIP_KERNEL_NAME(diag_band_kernel<RENDER_NONE>), grid, dim3(256), lds, stream, g, t, s, out);
  MMSA_CHECK_LAUNCH("render_band_u8");
  return MMSA_OK;
}
