// Boundary evaluation on device: the confusion counts of a class map against a label map, split by whether the pixel lies near a boundary of the label map
// and near a boundary of the prediction -- what the trimap accuracy / mIoU (Kohli et al.; the DeepLab plots) and the Boundary IoU (Cheng et al., CVPR 2021)
// are formed from, in float64 on the host (mmsa/evaluate.py).
//
// The quantity.  For a pixel p = (y, x) of the prediction grid [H, W]:
//   L(p) = the label code: l = lut[label[ymap[y], xmap[x]]] normalised as the confusion pass does -- a class < C, C for "kept but out of range" (any LUT
//          value in [C, 254]), 255 for ignored;                         P(p) = min(pred[p], C), the prediction code.
//   near_label(p) iff some pixel q OF THE IMAGE with Chebyshev distance max(|dy|, |dx|) <= d from p has L(q) != L(p); near_pred(p) the same for P.
//          Chebyshev: what d iterations of a 3 x 3 erosion give.  An ignored label is a code like any other as a NEIGHBOUR.
//   border = 0: neighbours outside the image do not exist -- which a window test with clamp-to-edge addressing is exactly (the clamped pixel lies inside
//          the window); border = 1: a pixel with y < d, x < d, y >= H - d or x >= W - d is near a boundary on both sides (the zero-padded erosion).
//   counts[slot][z][min(L, C)][P] += 1, int64 [n_slots, 4, C + 1, C + 1], z = 2 * near_label + near_pred, for every pixel whose own L is not 255.
//   The sum over the four zones is mmsa_eval_confusion_u8's matrix, bit for bit.
//
// The kernel.  ONE launch, grid (tiles, B, zone groups), 256 lanes.  A workgroup owns a tile of BND_TILE_W x TH output pixels (TH = 64 up to radius 16,
// 32 above) and stages the tile plus a halo of `radius` on every side, as CODES, one byte per pixel, for both maps, with clamp-to-edge addressing.  A window
// is uniform iff every one of its rows is uniform and the rows agree in one column, so the test is separable without min / max:
//   row pass     for every staged row and every tile column x: the code at x if the 2 d + 1 codes around it in that row are equal, else BND_MIXED (0xFE, no
//                code: codes are <= C <= 82 or 255).  Four columns per lane, as one dword: the window slides by byte shifts of a dword pair, and a byte of
//                OR_k (shifted_k ^ centre) is non-zero iff some code of that column's window differs.
//   column pass  for every tile pixel: near iff its row-pass byte is BND_MIXED or differs from one of the 2 d + 1 row-pass bytes above and below.  Four
//                columns per lane again, dword reads with no shifts; 64 lanes read 64 consecutive dwords.
// Then the border rule is ORed in and the pixel goes into the private uint32 LDS histogram [zones, C + 1, C + 1] (csrc/eval_hist.h: lanes of a wave that
// hold the same cell merge), which is flushed with 64-bit atomics.  Integers only: the same bytes run after run.
//
// LDS, as a function of radius d and classes C (TW = 64, rows = TH + 2 d staged rows, P = 17 + d / 2 dwords of row pitch: 64 + 2 d bytes and the dword the
// sliding pair reads ahead):
//   bytes = 4 * zones * (C + 1)^2  +  2 maps * rows * (P + 16) * 4  +  256 (the LUT)          zones = 4 / groups
//   d = 1: 2 * 66 * 33 * 4 = 17 424 B of tiles;  d = 8: 2 * 80 * 37 * 4 = 23 680;  d = 16: 2 * 96 * 41 * 4 = 31 488;  d = 32: 2 * 96 * 49 * 4 = 37 632 (the largest).
// The launch asks for at most 64 KiB.  Where four zone histograms do not fit next to the tiles the zones are split over gridDim.z into 2 or 4 groups, as
// csrc/selective.hip splits its bins: every group stages the tile and counts only its zones.  25 classes: 10 816 B of histograms, one group at every radius.
#include "common.h"
#include "eval_hist.h"
#include "boundary_px.h"     // the tile geometry, the row pass and the column pass: shared with csrc/render_diag.hip

#define BOUNDARY_MAX_RADIUS 32
static_assert(BOUNDARY_MAX_RADIUS == BND_MAX_RADIUS, "the radius limit is the shared tile geometry's");
// The largest C for which ONE zone's histogram fits next to the tiles at the maximum radius: 65536 - 256 - 37632 = 27648 bytes = 6912 cells >= (C + 1)^2
// gives C + 1 <= 83 (83^2 = 6889, 84^2 = 7056).
#define BOUNDARY_MAX_CLASSES 82
#define BND_LDS_BYTES 65536

static_assert(256 + 37632 + 83 * 83 * 4 <= BND_LDS_BYTES && 256 + 37632 + 84 * 84 * 4 > BND_LDS_BYTES, "BOUNDARY_MAX_CLASSES");

struct BndGeom {                      // the geometry of a launch, formed once on the host
  int H, W, r, border;
  int TH, rows, cols, pdw;            // tile rows; staged rows TH + 2 r, staged columns 64 + 2 r, dwords of staged row pitch
  int tiles_x, zn;                    // tiles per row of tiles; zones per group
};

static inline size_t bnd_lds_bytes(int r, int C, int zn) {
  return ((size_t)zn * (C + 1) * (C + 1) + (size_t)2 * (bnd_tile_h(r) + 2 * r) * (bnd_pitch_dw(r) + BND_TILE_W / 4)) * 4 + 256;
}

__global__ __launch_bounds__(256) void eval_boundary_kernel(const unsigned char* __restrict__ pred, EvalLabel ev, EvalSlots es, BndGeom g) {
  extern __shared__ unsigned bnd_lds[];
  const int C = ev.C, nb = (C + 1) * (C + 1), r = g.r, rows = g.rows, pdw = g.pdw, H = g.H, W = g.W;
  constexpr int RDW = BND_TILE_W / 4;
  unsigned* hist = bnd_lds;
  unsigned* stL = hist + g.zn * nb;             // staged codes [rows][pdw dwords], label / prediction
  unsigned* stP = stL + rows * pdw;
  unsigned* rpL = stP + rows * pdw;             // row-pass bytes [rows][16 dwords]
  unsigned* rpP = rpL + rows * RDW;
  unsigned char* lut_s = (unsigned char*)(rpP + rows * RDW);
  eval_hist_init(hist, lut_s, ev.lut, g.zn * nb);
  const int b = blockIdx.y;
  const int ty = (int)blockIdx.x / g.tiles_x, tx = (int)blockIdx.x - ty * g.tiles_x;
  const int y0 = ty * g.TH, x0 = tx * BND_TILE_W;

  // 1. stage the codes of tile + halo, clamp-to-edge: a wave per staged row, a lane per column (64 + 2 r <= 128: two columns per lane at the most)
  {
    const bool tables = ev.ymap != nullptr;
    const int lx = threadIdx.x & 63, ly = threadIdx.x >> 6, pitch = pdw * 4;
    const unsigned char* pp = pred + (long)b * H * W;
    const unsigned char* lp = ev.label + (long)b * ev.Hl * ev.Wl;
    unsigned char* bL = (unsigned char*)stL;
    unsigned char* bP = (unsigned char*)stP;
    int xc[2], xs[2];
#pragma unroll
    for (int q = 0; q < 2; ++q) {
      xc[q] = min(max(x0 - r + lx + 64 * q, 0), W - 1);
      xs[q] = tables ? min(max(ev.xmap[xc[q]], 0), ev.Wl - 1) : xc[q];
    }
    for (int sy = ly; sy < rows; sy += 4) {
      const int yc = min(max(y0 - r + sy, 0), H - 1);
      const int ys = tables ? min(max(ev.ymap[yc], 0), ev.Hl - 1) : yc;
      const unsigned char* prow = pp + (long)yc * W;
      const unsigned char* lrow = lp + (long)ys * ev.Wl;
#pragma unroll
      for (int q = 0; q < 2; ++q) {
        const int sx = lx + 64 * q;
        if (sx < g.cols) {
          const int l = lut_s[lrow[xs[q]]];
          bL[sy * pitch + sx] = (unsigned char)(l == MMSA_EVAL_IGNORE ? MMSA_EVAL_IGNORE : min(l, C));
          bP[sy * pitch + sx] = (unsigned char)min((int)prow[xc[q]], C);
        }
      }
    }
  }
  __syncthreads();

  // 2. row pass over every staged row, both maps
  for (int i = threadIdx.x; i < rows * RDW; i += 256) {
    const int sy = i / RDW, gx = i - sy * RDW;
    rpL[i] = bnd_row_pass(stL + sy * pdw + gx, r);
    rpP[i] = bnd_row_pass(stP + sy * pdw + gx, r);
  }
  __syncthreads();

  // 3. column pass and count: TH * 16 is a multiple of 256, so every lane makes every trip (eval_hist_add votes across the wave)
  const int z0 = (int)blockIdx.z * g.zn;
  for (int i = threadIdx.x; i < g.TH * RDW; i += 256) {
    const int y = i / RDW, gx = i - y * RDW;
    const unsigned nl = bnd_col_pass(rpL + i, r), np = bnd_col_pass(rpP + i, r);
    const int Y = y0 + y, X = x0 + 4 * gx;
    const bool edge_y = g.border && (Y < r || Y >= H - r);
    const unsigned char* cl = (const unsigned char*)(stL + (y + r) * pdw) + 4 * gx + r;      // the pixels' own codes
    const unsigned char* cp = (const unsigned char*)(stP + (y + r) * pdw) + 4 * gx + r;
    int bin[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      bin[j] = -1;
      if (Y < H && X + j < W) {
        const int l = cl[j];
        if (l != MMSA_EVAL_IGNORE) {
          const bool edge = edge_y || (g.border && (X + j < r || X + j >= W - r));
          const int nlj = (int)((nl >> (8 * j + 7)) & 1u) | (int)edge, npj = (int)((np >> (8 * j + 7)) & 1u) | (int)edge;
          const int z = 2 * nlj + npj - z0;
          if ((unsigned)z < (unsigned)g.zn) bin[j] = z * nb + l * (C + 1) + (int)cp[j];
        }
      }
    }
    const bool uni = bin[0] >= 0 && bin[0] == bin[1] && bin[1] == bin[2] && bin[2] == bin[3];      // four pixels of one cell: one add of 4, merged across the wave
    eval_hist_add(hist, uni ? bin[0] : -1, 4u);
    if (!uni) {
#pragma unroll
      for (int j = 0; j < 4; ++j)
        if (bin[j] >= 0) atomicAdd(&hist[bin[j]], 1u);
    }
  }
  eval_hist_flush(hist, ev.counts + ((long)es.s[b] * 4 + z0) * nb, g.zn * nb);
}

extern "C" int mmsa_eval_boundary_u8(const unsigned char* pred, const unsigned char* label, int B, int H, int W, int Hl, int Wl, const unsigned char* lut,
                                     int C, const int* ymap, const int* xmap, const int* slots /* HOST [B] */, int n_slots, int radius, int border,
                                     int64_t* counts, hipStream_t stream) {
  const char* name = "eval_boundary_u8";
  MMSA_CHECK_ARG(pred, "%s: pred is required", name);
  EvalSlots es;
  int rc = eval_check(name, label, B, H, W, Hl, Wl, lut, C, ymap, xmap, slots, n_slots, counts, es, BOUNDARY_MAX_CLASSES,
                      "one zone's (C + 1)^2 uint32 histogram must fit 64 KiB of LDS next to the tiles of radius 32");
  if (rc) return rc;
  MMSA_CHECK_ARG(radius >= 1 && radius <= BOUNDARY_MAX_RADIUS, "%s: radius = %d; 1..%d are supported", name, radius, BOUNDARY_MAX_RADIUS);
  MMSA_CHECK_ARG(border == 0 || border == 1, "%s: border = %d; 0 (neighbours outside the image do not exist) or 1 (the image border is a boundary)", name,
                 border);
  int groups = 1;
  while (groups < 4 && bnd_lds_bytes(radius, C, 4 / groups) > BND_LDS_BYTES) groups *= 2;      // C <= BOUNDARY_MAX_CLASSES: four groups always fit
  const int TH = bnd_tile_h(radius), tiles_x = cdiv(W, BND_TILE_W);
  const BndGeom g = {H, W, radius, border, TH, TH + 2 * radius, BND_TILE_W + 2 * radius, bnd_pitch_dw(radius), tiles_x, 4 / groups};
  const EvalLabel ev = {label, lut, ymap, xmap, (unsigned long long*)counts, Hl, Wl, C};
  const dim3 grid((unsigned)tiles_x * (unsigned)cdiv(H, TH), B, groups);
  hipLaunchKernelGGL(eval_boundary_kernel, grid, dim3(256), bnd_lds_bytes(radius, C, g.zn), stream, pred, ev, es, g);
  MMSA_CHECK_LAUNCH("eval_boundary_u8");
  return MMSA_OK;
}
