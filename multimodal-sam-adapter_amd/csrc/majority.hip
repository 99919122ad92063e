// Majority (mode) filter on device (mmsa_majority_filter_u8): every target pixel of a byte map takes the most frequent voter value of its (2 r + 1) x (2 r + 1)
// window, so that salt-and-pepper pixels go, ragged contours straighten and holes close by the vote of everything near.  Integers only: the same bytes run
// after run.
//
// The quantity.  role[256] gives every byte one of three roles: 0 = voter (votes with its value and may be rewritten), 1 = hole (votes nothing and is to be
// rewritten), 2 = inert (votes nothing, is never rewritten, blocks nothing).  For a pixel p of image b, over the pixels q of the SAME image with
// |qy - py| <= r and |qx - px| <= r (the window is clipped at the image border: no padding, a corner's window holds fewer pixels):
//   n_v(p) = the voters of value v in the window;  T(p) = sum_v n_v(p);  n_best(p) = max_v n_v(p).
//   w(p) = p's own value if p is a voter and n_own(p) = n_best(p) (a tie never changes a pixel that is among the tied), else the smallest v with n_v = n_best.
//   targets: every hole, and with all = 1 every voter; never an inert pixel.
//   out[p] = w(p) iff p is a target and T(p) > 0 and (half = 0 or 2 n_best(p) > T(p)); else src[p].  support[p] = n_best(p) at a target, 0 elsewhere.
//
// The kernel.  ONE launch, a workgroup of 256 lanes per tile of MAJ_TILE_W x TH output pixels, no workgroup waits for another, every loop bounded by the tile,
// by the radius or by 256 values.  TH = 16 up to radius 8, 32 up to radius 16, 64 above: about the height of the window.  A low tile holds fewer values and
// gives the chip more waves; a tall one stages less halo per pixel (measured: profiles/majority_filter.txt; a debug-knob build reads MMSA_MAJ_TH).
//   stage     the tile with a halo of r on every side as one uint16 CODE per pixel: value | role << 8; a pixel outside the image is inert (it votes nothing,
//             which is the clipped window).  A wave per staged row, a lane per column.  A voter ORs its value's bit into the 256-bit set of values present,
//             once per change of value down its column.
//   per value v of that set, ascending (uniform over the workgroup):
//     rows    a wave per staged row: the row's mask of "code == v" is two 64-bit ballots (64 + 2 r <= 128 columns), and the horizontal count of output column
//             x is one popcount of the 2 r + 1 bits from bit x on.  One byte per staged row and output column (<= 65), into one of two LDS buffers in turn,
//             so that ONE barrier per value orders the rows of value k + 1 behind the columns of value k - 1.
//     columns a lane owns output column x of a strip of TH / 4 rows and slides the vertical sum of those bytes down it (one add, one subtract per row).  In
//             registers per row: n_best and the value that holds it (a strict > while v ascends keeps the smallest of equals), the count of the own value,
//             and T as the sum of all counts.
//   write     out and support, a wave on 64 consecutive x.
// Work per pixel is O(values present in the staged region), typically 2 .. 6 on a class map; it does not depend on the class count.  A noise map is the
// worst case.  The alternative, a per-lane histogram column in LDS (mmsa_slide_argmax_score's idiom), costs O((2 r + 1)^2) updates per pixel and is not built.
//
// LDS: (TH + 2 r) rows of 128 codes (256 B) and twice 64 count bytes, the role table and the set: r = 1: 7 200 B; r = 8: 12 576 B; r = 16: 24 864 B; r = 32:
// 49 440 B (the largest).
#include "common.h"

#define MAJ_MAX_RADIUS 32
#define MAJ_TILE_W 64
#define MAJ_PITCH 128                // staged codes per row: 64 + 2 r <= 128, the rest inert
#define MAJ_ROLE_VOTER 0
#define MAJ_ROLE_HOLE 1
#define MAJ_ROLE_INERT 2

static inline int maj_tile_h(int r) {
  const int th = MMSA_KNOB("MMSA_MAJ_TH", 0);
  return th == 16 || th == 32 || th == 64 ? th : r <= 8 ? 16 : r <= 16 ? 32 : 64;
}
static inline size_t maj_lds_bytes(int r) { return (size_t)(maj_tile_h(r) + 2 * r) * (MAJ_PITCH * 2 + 2 * MAJ_TILE_W) + 256 + 32; }
static_assert((64 + 2 * MAJ_MAX_RADIUS) * (MAJ_PITCH * 2 + 2 * MAJ_TILE_W) + 288 <= 65536, "the tallest tile at the largest radius fits 64 KiB of LDS");

struct MajGeom {                     // the geometry of a launch, formed once on the host
  int H, W, r, all, half;
  int rows;                          // staged rows TH + 2 r
  int tiles_x, tiles;                // tiles per row of tiles; tiles per image
};

// S = TH / 4: the rows of a lane's strip
template <int S>
__global__ __launch_bounds__(256) void majority_kernel(const unsigned char* __restrict__ src, const unsigned char* __restrict__ role, MajGeom g,
                                                       unsigned char* __restrict__ out, unsigned short* __restrict__ support) {
  extern __shared__ unsigned maj_lds[];
  constexpr int TH = 4 * S;
  const int r = g.r, rows = g.rows, H = g.H, W = g.W;
  unsigned short* st = (unsigned short*)maj_lds;                       // [rows][MAJ_PITCH] codes
  unsigned char* hc = (unsigned char*)(st + rows * MAJ_PITCH);         // [2][rows][64] horizontal counts of the value in hand
  unsigned* present = (unsigned*)(hc + 2 * rows * MAJ_TILE_W);         // [8]: rows * 384 is a multiple of 4
  unsigned char* role_s = (unsigned char*)(present + 8);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int b = (int)(blockIdx.x / (unsigned)g.tiles), t = (int)(blockIdx.x - (unsigned)b * (unsigned)g.tiles);
  const int ty = t / g.tiles_x, tx = t - ty * g.tiles_x;
  const int y0 = ty * TH, x0 = tx * MAJ_TILE_W;
  const unsigned char* __restrict__ img = src + (long)b * H * W;

  role_s[threadIdx.x] = role[threadIdx.x];
  if (threadIdx.x < 8) present[threadIdx.x] = 0u;
  __syncthreads();

  // 1. stage the codes of tile + halo; outside the image and beyond column 64 + 2 r: inert
  {
    int last[2] = {-1, -1};
    for (int sy = wave; sy < rows; sy += 4) {
      const int Y = y0 - r + sy;
#pragma unroll
      for (int q = 0; q < 2; ++q) {
        const int sx = lane + 64 * q, X = x0 - r + sx;
        int code = MAJ_ROLE_INERT << 8;
        if (sx < MAJ_TILE_W + 2 * r && Y >= 0 && Y < H && X >= 0 && X < W) {
          const int v = img[(long)Y * W + X];
          const int ro = min((int)role_s[v], MAJ_ROLE_INERT);
          code = v | (ro << 8);
          if (ro == MAJ_ROLE_VOTER && v != last[q]) {
            atomicOr(&present[v >> 5], 1u << (v & 31));
            last[q] = v;
          }
        }
        st[sy * MAJ_PITCH + sx] = (unsigned short)code;
      }
    }
  }
  __syncthreads();

  // the lane's strip: output column `lane`, rows wave * S .. wave * S + S - 1 of the tile
  const int sy0 = wave * S;                                            // the first staged row of the first window
  int own[S];
  unsigned bp[S], ot[S];                                               // n_best << 8 | its value;  n_own | T << 16
#pragma unroll
  for (int j = 0; j < S; ++j) {
    own[j] = st[(sy0 + j + r) * MAJ_PITCH + lane + r];
    bp[j] = 0u;
    ot[j] = 0u;
  }
  const unsigned long long mlo = 2 * r + 1 >= 64 ? ~0ull : (1ull << (2 * r + 1)) - 1ull;
  const unsigned long long mhi = 2 * r + 1 > 64 ? 1ull : 0ull;       // r = 32: the 65th bit of the span

  // 2. value by value, ascending
  int turn = 0;
  for (int w = 0; w < 8; ++w) {
    unsigned bits = present[w];                                        // the same word in every lane
    while (bits) {
      const int v = 32 * w + __builtin_ctz(bits);
      bits &= bits - 1u;
      unsigned char* h = hc + turn * rows * MAJ_TILE_W;
      turn ^= 1;
      // rows: the mask of a staged row, and per output column the popcount of its span
      for (int sy = wave; sy < rows; sy += 4) {
        const unsigned long long lo = __ballot(st[sy * MAJ_PITCH + lane] == v), hi = __ballot(st[sy * MAJ_PITCH + 64 + lane] == v);
        const unsigned long long span = lane ? (lo >> lane) | (hi << (64 - lane)) : lo;
        h[sy * MAJ_TILE_W + lane] = (unsigned char)(__popcll(span & mlo) + (int)((hi >> lane) & mhi));
      }
      __syncthreads();
      // columns: the vertical sum slides down the strip
      int sum = 0;
      for (int k = 0; k <= 2 * r; ++k) sum += h[(sy0 + k) * MAJ_TILE_W + lane];
#pragma unroll
      for (int j = 0; j < S; ++j) {
        const unsigned n = (unsigned)sum;
        if (n > (bp[j] >> 8)) bp[j] = (n << 8) | (unsigned)v;
        ot[j] += n << 16;
        if (own[j] == v) ot[j] |= n;                                   // own is a voter's code then; a value comes by once
        if (j + 1 < S) sum += (int)h[(sy0 + j + 1 + 2 * r) * MAJ_TILE_W + lane] - (int)h[(sy0 + j) * MAJ_TILE_W + lane];
      }
    }
  }

  // 3. the result
  const int X = x0 + lane;
  if (X >= W) return;
#pragma unroll
  for (int j = 0; j < S; ++j) {
    const int Y = y0 + sy0 + j;
    if (Y >= H) break;
    const int ro = own[j] >> 8, ov = own[j] & 255;
    const int nb = (int)(bp[j] >> 8), bv = (int)(bp[j] & 255u), no = (int)(ot[j] & 0xFFFFu), T = (int)(ot[j] >> 16);
    const bool target = ro == MAJ_ROLE_HOLE || (g.all && ro == MAJ_ROLE_VOTER);
    const int win = (ro == MAJ_ROLE_VOTER && no == nb) ? ov : bv;
    const bool change = target && T > 0 && (!g.half || 2 * nb > T);
    const long at = ((long)b * H + Y) * W + X;
    out[at] = (unsigned char)(change ? win : ov);
    if (support) support[at] = (unsigned short)(target ? nb : 0);
  }
}

extern "C" int mmsa_majority_filter_u8(const unsigned char* src, int B, int H, int W, const unsigned char* role, int radius, int all, int half,
                                       unsigned char* out, unsigned short* support, hipStream_t stream) {
  const char* name = "majority_filter_u8";
  MMSA_CHECK_ARG(src && role && out, "%s: src, role and out are required", name);
  MMSA_CHECK_ARG((const void*)out != (const void*)src, "%s: out is src; a stencil cannot run in place", name);
  MMSA_CHECK_ARG((const void*)support != (const void*)src && (void*)support != (void*)out, "%s: support is a plane of its own, neither src nor out", name);
  MMSA_CHECK_ARG(B > 0 && H > 0 && W > 0 && (long)H * W < (1l << 31), "%s: bad map size", name);
  MMSA_CHECK_ARG(radius >= 1 && radius <= MAJ_MAX_RADIUS, "%s: radius = %d; 1..%d are supported", name, radius, MAJ_MAX_RADIUS);
  MMSA_CHECK_ARG(all == 0 || all == 1, "%s: all = %d; 0 (the holes alone are rewritten) or 1 (the voters as well)", name, all);
  MMSA_CHECK_ARG(half == 0 || half == 1, "%s: half = %d; 0 or 1 (a pixel changes only where one value holds more than half of the votes)", name, half);
  const int TH = maj_tile_h(radius), tiles_x = cdiv(W, MAJ_TILE_W), tiles = tiles_x * cdiv(H, TH);
  MMSA_CHECK_ARG((long)tiles * B < (1l << 31), "%s: %d maps of %d x %d are more workgroups than a launch holds", name, B, H, W);
  const MajGeom g = {H, W, radius, all, half, TH + 2 * radius, tiles_x, tiles};
  const dim3 grid((unsigned)tiles * (unsigned)B);
  const size_t lds = maj_lds_bytes(radius);
  if (TH == 64) hipLaunchKernelGGL(majority_kernel<16>, grid, dim3(256), lds, stream, src, role, g, out, support);
  else if (TH == 32) hipLaunchKernelGGL(majority_kernel<8>, grid, dim3(256), lds, stream, src, role, g, out, support);
  else hipLaunchKernelGGL(majority_kernel<4>, grid, dim3(256), lds, stream, src, role, g, out, support);
  MMSA_CHECK_LAUNCH("majority_filter_u8");
  return MMSA_OK;
}
