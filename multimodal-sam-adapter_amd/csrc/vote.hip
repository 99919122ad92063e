// Guided vote filter on device (mmsa_vote_filter_u8): the joint-bilateral weighted mode filter of a byte map.  Every voter of a (2 r + 1) x (2 r + 1) window
// votes for its value with a weight that falls with the difference of its GUIDE pixel (a raw uint8 frame, 1 or 3 channels) from the centre's, and rises with
// its own confidence; every target pixel takes the value with the largest sum.  A contour snaps to the guide's edge, and a 0.3-confidence pixel no longer
// counts like a 0.99-confidence one.  Integers only: the same bytes run after run.
//
// The quantity.  role[256], the window (clipped at the image border, no padding), the targets and the half rule are csrc/majority.hip's.  Over the voter
// pixels q of value v in the window of p:
//   d(p, q) = sum_c |g_p[c] - g_q[c]|, 0 .. 255 G, on the top-left H x W of the guide [B, Hg, Wg, G];  lut[d] in 0 .. 4096 (uint16, 255 G + 1 entries);
//   wq(q) = min(255, (int)(conf_clamp(weight[q]) * 256.0f)) (csrc/conf_bin.h: NaN, negatives and anything below 1 / 256 vote nothing); 1 without weights;
//   S_v(p) = sum lut[d(p, q)] wq(q) (lut = 1 without a guide);  T(p) = sum_v S_v(p);  S_best(p) = max_v S_v(p).
//   w(p) = p's own value if p is a voter and S_own(p) = S_best(p), else the smallest v with S_v = S_best.
//   out[p] = w(p) iff p is a target and T(p) > 0 and (half = 0 or 2 S_best(p) > T(p)); else src[p].  support[p] = S_best(p) at a target, 0 elsewhere.
// Overflow bound: a tap adds at most 4096 * 255 = 1 044 480 < 2^20 and a window holds at most 33^2 = 1089 < 2^11 taps, so T <= 1 137 438 720 < 2^31: the
// uint32 sums are exact, and so is 2 S_best < 2^32 of the half rule.
//
// The kernel.  ONE launch, a workgroup of 256 lanes per tile of VOTE_TILE_W x TH output pixels, no workgroup waits for another, every loop bounded by the
// tile, by the radius or by 256 values.  TH = 8 up to radius 2, 16 above, by measurement (profiles/vote_filter.txt: 8 / 16 / 32 rows at radius 1, 2, 4, 8 and
// 16 -- at radius 1 and 2 eight rows are 8 % faster than 16 and 32 rows 18 - 20 % slower; at radius 4, 8 and 16 sixteen rows are 1.5 - 4 % ahead of eight and
// 7 - 13 % ahead of 32, which do not fit 64 KiB at radius 16; a debug-knob build reads MMSA_VOTE_TH = 8 / 16 / 32).
//   stage     the tile with a halo of r on every side: per pixel the guide channels packed into ONE dword, and a uint16 code = value | wq << 8, wq = 0 for a
//             hole, an inert pixel and a pixel outside the image (which is the clipped window).  A voter ORs its value's bit into the 256-bit set of values
//             present.  The range table is staged next to them.
//   slots     the values present are compacted to dense SLOTS: the rank of the value in the set, by popcounts (ranks keep the order of the values); the staged
//             code then holds slot | wq << 8.
//   walk      a lane owns output column `lane` of a strip of TH / 4 rows (2 or 4) and takes its pixels one after the other.  Per pixel a private column of 32 uint32
//             sums in LDS, laid out [slot][lane of the workgroup]: the 64 lanes of a wave hit 64 consecutive dwords, an update never conflicts and no barrier
//             is needed from here on.  Per tap: the neighbour's guide dword and code (neighbouring lanes read neighbouring addresses), d by one
//             sum-of-absolute-differences instruction on the packed dwords, lut[d] * wq added to the tap's slot by an LDS add without a return value (the
//             column is private; the add is used because nothing has to wait for it), four taps of a row in flight.  With more than 32 slots present the walk
//             repeats per group of 32 (the count is uniform over the workgroup, at most 8: a class map needs one pass, 200-value noise seven).
//   winner    the column read in ascending slot order -- ascending value -- with a strict >, which keeps the smallest of equal sums; the own slot's sum apart.
// Work per pixel is O((2 r + 1)^2) whatever the map holds; csrc/majority.hip's O(values present) form cannot carry weights, its counts being popcounts.
//
// LDS: (TH + 2 r) rows of 64 + 2 r pixels at 6 bytes (2 without a guide), the 32 KiB of columns, the range table, the role table, the two slot tables and the
// set.  The largest configuration is TH + 2 r = 48 rows at r = 16 with a 3-channel table: 27 648 + 32 768 + 1 532 + 768 + 32 = 62 748 B.
#include "common.h"
#include "conf_bin.h"

#define VOTE_MAX_RADIUS 16
#define VOTE_TILE_W 64
#define VOTE_MAX_ROWS 48             // TH + 2 r: 16 + 32, or 32 + 16
#define VOTE_GROUP 32                // the slots of one walk
#define VOTE_TAPS 4                  // the taps of a row a lane has in flight: 2 r + 1 = 4 k + 1 at every even radius
#define VOTE_MAX_LUT (255 * 3 + 1)
#define VOTE_ROLE_VOTER 0
#define VOTE_ROLE_HOLE 1
#define VOTE_ROLE_INERT 2

static inline int vote_tile_h(int r) {
  const int th = MMSA_KNOB("MMSA_VOTE_TH", 0);
  return (th == 8 || th == 16 || th == 32) && th + 2 * r <= VOTE_MAX_ROWS ? th : r <= 2 ? 8 : 16;
}
static inline size_t vote_lut_bytes(int G) { return (size_t)(((255 * G + 1) * 2 + 3) & ~3); }
static inline size_t vote_lds_bytes(int rows, int r, int G) {
  return (size_t)rows * (VOTE_TILE_W + 2 * r) * (G ? 6 : 2) + VOTE_GROUP * 256 * 4 + (G ? vote_lut_bytes(G) : 0) + 3 * 256 + 32;
}
static_assert(VOTE_MAX_ROWS * (VOTE_TILE_W + 2 * VOTE_MAX_RADIUS) * 6 + VOTE_GROUP * 256 * 4 + ((VOTE_MAX_LUT * 2 + 3) & ~3) + 3 * 256 + 32 <= 65536,
              "the tallest staged region at the largest radius with a 3-channel table fits 64 KiB of LDS");

struct VoteGeom {                    // the geometry of a launch, formed once on the host
  int H, W, r, all, half;
  int th, rows, pitch;               // tile height; staged rows th + 2 r; staged pixels per row 64 + 2 r
  int tiles_x, tiles;                // tiles per row of tiles; tiles per image
  int Hg, Wg, G, nlut;               // the guide's frame, its channels (0: no guide) and the entries of the range table
};

__device__ __forceinline__ unsigned vote_sad(unsigned a, unsigned b) { return __builtin_amdgcn_sad_u8(a, b, 0u); }

// One tap: code = slot | wq << 8, k = the range weight.  The vote goes to the lane's own column with an LDS add that returns nothing, so that no tap waits for
// the sum before it; a tap of another slot group, or without a vote, adds 0 to slot s & 31 of the column (no branch).  That slot may lie at or beyond ns:
// its dword was not zeroed in this walk, holds whatever an earlier walk left, and is never read -- the winner reads the slots below ns alone.  The price: every
// tap of every walk is an LDS add, so a tile of 200 values pays 7 (2 r + 1)^2 adds per pixel, six in seven of them zeros.
__device__ __forceinline__ void vote_add(unsigned* col, unsigned code, unsigned k, int base, int ns) {
  const unsigned s = (code & 255u) - (unsigned)base;
  const unsigned w = s < (unsigned)ns ? (code >> 8) * k : 0u;
  __hip_atomic_fetch_add(col + (s & (VOTE_GROUP - 1)) * 256, w, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT);
}

template <bool GUIDE>
__global__ __launch_bounds__(256) void vote_kernel(const unsigned char* __restrict__ src, const unsigned char* __restrict__ role, VoteGeom g,
                                                   const unsigned char* __restrict__ guide, const unsigned short* __restrict__ range_lut,
                                                   const float* __restrict__ weight, unsigned char* __restrict__ out, unsigned* __restrict__ support) {
  extern __shared__ unsigned vote_lds[];
  const int r = g.r, rows = g.rows, pitch = g.pitch, H = g.H, W = g.W;
  unsigned* hist = vote_lds;                                            // [VOTE_GROUP][256] sums: the column of lane t is hist[s * 256 + t]
  unsigned* sg = hist + VOTE_GROUP * 256;                               // [rows][pitch] guide dwords
  unsigned* present = sg + (GUIDE ? rows * pitch : 0);                  // [8]
  unsigned short* sc = (unsigned short*)(present + 8);                  // [rows][pitch] codes; rows * pitch is even
  unsigned short* lut = sc + rows * pitch;                              // [nlut], padded to a dword
  unsigned char* role_s = (unsigned char*)(lut + (GUIDE ? ((g.nlut + 1) & ~1) : 0));
  unsigned char* slot_of = role_s + 256;                                // value -> slot
  unsigned char* value_of = slot_of + 256;                              // slot -> value
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int b = (int)(blockIdx.x / (unsigned)g.tiles), t = (int)(blockIdx.x - (unsigned)b * (unsigned)g.tiles);
  const int ty = t / g.tiles_x, tx = t - ty * g.tiles_x;
  const int y0 = ty * g.th, x0 = tx * VOTE_TILE_W;
  const unsigned char* __restrict__ img = src + (long)b * H * W;

  role_s[tid] = role[tid];
  if (tid < 8) present[tid] = 0u;
  if (GUIDE)
    for (int i = tid; i < g.nlut; i += 256) lut[i] = range_lut[i];
  __syncthreads();

  // 1. stage tile + halo: the guide dword and value | wq << 8; outside the image wq = 0
  for (int sy = wave; sy < rows; sy += 4) {
    const int Y = y0 - r + sy;
    for (int sx = lane; sx < pitch; sx += 64) {
      const int X = x0 - r + sx;
      unsigned code = 0u, gd = 0u;
      if (Y >= 0 && Y < H && X >= 0 && X < W) {
        const long at = (long)Y * W + X;
        const unsigned v = img[at];
        if (role_s[v] == VOTE_ROLE_VOTER) {
          const unsigned wq = weight ? (unsigned)conf_bin(conf_clamp(weight[(long)b * H * W + at]), 256, 256.0f) : 1u;
          code = v | (wq << 8);
          atomicOr(&present[v >> 5], 1u << (v & 31));
        }
        if (GUIDE) {
          const unsigned char* gp = guide + (((long)b * g.Hg + Y) * g.Wg + X) * g.G;
          gd = gp[0];
          if (g.G == 3) gd |= ((unsigned)gp[1] << 8) | ((unsigned)gp[2] << 16);
        }
      }
      sc[sy * pitch + sx] = (unsigned short)code;
      if (GUIDE) sg[sy * pitch + sx] = gd;
    }
  }
  __syncthreads();

  // 2. slots: the rank of every value present
  int nslots = 0;
  {
    int below = 0;
    const unsigned v = (unsigned)tid;
#pragma unroll
    for (int w = 0; w < 8; ++w) {
      const unsigned bits = present[w];
      nslots += __popc(bits);
      below += (int)v >= 32 * (w + 1) ? __popc(bits) : (int)(v >> 5) == w ? __popc(bits & ((1u << (v & 31)) - 1u)) : 0;
    }
    if ((present[v >> 5] >> (v & 31)) & 1u) {
      slot_of[v] = (unsigned char)below;
      value_of[below] = (unsigned char)v;
    }
  }
  __syncthreads();
  for (int sy = wave; sy < rows; sy += 4)
    for (int sx = lane; sx < pitch; sx += 64) {                         // every lane rewrites the codes it staged
      const unsigned c = sc[sy * pitch + sx];
      sc[sy * pitch + sx] = (unsigned short)((c >> 8) ? (c & 0xFF00u) | slot_of[c & 255u] : 0u);
    }
  __syncthreads();

  // 3. the lane's strip: output column `lane`, rows wave * S .. wave * S + S - 1 of the tile; no barrier from here on
  const int X = x0 + lane;
  if (X >= W) return;
  const int S = g.th >> 2, win = 2 * r + 1;
  unsigned* col = hist + tid;
  for (int j = 0; j < S; ++j) {
    const int ry = wave * S + j, Y = y0 + ry;                           // ry: the first staged row of the window
    if (Y >= H) break;
    const long at = (long)Y * W + X;
    const int ov = img[at], ro = role_s[ov];
    const int own_slot = ro == VOTE_ROLE_VOTER ? (int)slot_of[ov] : -1;
    const unsigned gp = GUIDE ? sg[(ry + r) * pitch + lane + r] : 0u;
    unsigned best = 0u, total = 0u, own = 0u;
    int best_slot = 0;
    for (int base = 0; base < nslots; base += VOTE_GROUP) {             // uniform over the workgroup
      const int ns = min(VOTE_GROUP, nslots - base);
      for (int s = 0; s < ns; ++s) col[s * 256] = 0u;
      for (int dy = 0; dy < win; ++dy) {
        const unsigned short* crow = sc + (ry + dy) * pitch + lane;
        const unsigned* grow = sg + (ry + dy) * pitch + lane;
        int dx = 0;
        for (; dx + VOTE_TAPS <= win; dx += VOTE_TAPS) {                // VOTE_TAPS taps in flight: their reads first, then the table, then the adds
          unsigned c[VOTE_TAPS], d[VOTE_TAPS], k[VOTE_TAPS];
#pragma unroll
          for (int i = 0; i < VOTE_TAPS; ++i) {
            c[i] = crow[dx + i];
            if (GUIDE) d[i] = grow[dx + i];
          }
#pragma unroll
          for (int i = 0; i < VOTE_TAPS; ++i) k[i] = GUIDE ? lut[vote_sad(d[i], gp)] : 1u;
#pragma unroll
          for (int i = 0; i < VOTE_TAPS; ++i) vote_add(col, c[i], k[i], base, ns);
        }
        for (; dx < win; ++dx) vote_add(col, crow[dx], GUIDE ? lut[vote_sad(grow[dx], gp)] : 1u, base, ns);
      }
      for (int s = 0; s < ns; ++s) {                                    // ascending slot = ascending value
        const unsigned n = col[s * 256];
        total += n;
        if (n > best) {
          best = n;
          best_slot = base + s;
        }
        if (base + s == own_slot) own = n;
      }
    }
    const bool target = ro == VOTE_ROLE_HOLE || (g.all && ro == VOTE_ROLE_VOTER);
    const int winner = (ro == VOTE_ROLE_VOTER && own == best) ? ov : (int)value_of[best_slot];
    const bool change = target && total > 0u && (!g.half || 2u * best > total);
    out[(long)b * H * W + at] = (unsigned char)(change ? winner : ov);
    if (support) support[(long)b * H * W + at] = target ? best : 0u;
  }
}

extern "C" int mmsa_vote_filter_u8(const unsigned char* src, int B, int H, int W, const unsigned char* role, int radius, int all, int half,
                                   const unsigned char* guide, int Hg, int Wg, int G, const unsigned short* range_lut, const float* weight,
                                   unsigned char* out, unsigned* support, hipStream_t stream) {
  const char* name = "vote_filter_u8";
  MMSA_CHECK_ARG(src && role && out, "%s: src, role and out are required", name);
  MMSA_CHECK_ARG((guide == nullptr) == (range_lut == nullptr), "%s: guide and range_lut come together; one of them is null", name);
  MMSA_CHECK_ARG((const void*)out != (const void*)src, "%s: out is src; a stencil cannot run in place", name);
  MMSA_CHECK_ARG((const void*)support != (const void*)src && (void*)support != (void*)out, "%s: support is a plane of its own, neither src nor out", name);
  MMSA_CHECK_ARG((const void*)out != (const void*)guide && (const void*)out != (const void*)weight && (!support || ((const void*)support != (const void*)guide &&
                 (const void*)support != (const void*)weight)), "%s: out and support are planes of their own, neither the guide nor the weights", name);
  MMSA_CHECK_ARG(B > 0 && H > 0 && W > 0 && (long)H * W < (1l << 31), "%s: bad map size", name);
  MMSA_CHECK_ARG(radius >= 1 && radius <= VOTE_MAX_RADIUS, "%s: radius = %d; 1..%d are supported", name, radius, VOTE_MAX_RADIUS);
  MMSA_CHECK_ARG(all == 0 || all == 1, "%s: all = %d; 0 (the holes alone are rewritten) or 1 (the voters as well)", name, all);
  MMSA_CHECK_ARG(half == 0 || half == 1, "%s: half = %d; 0 or 1 (a pixel changes only where one value holds more than half of the votes)", name, half);
  if (guide) {
    MMSA_CHECK_ARG(G == 1 || G == 3, "%s: G = %d; a guide of 1 or 3 channels is supported", name, G);
    MMSA_CHECK_ARG(Hg >= H && Wg >= W, "%s: the guide is %d x %d, the map %d x %d; the map is the guide's top-left corner", name, Hg, Wg, H, W);
    MMSA_CHECK_ARG((long)Hg * Wg < (1l << 31), "%s: bad guide size", name);
  }
  const int TH = vote_tile_h(radius), tiles_x = cdiv(W, VOTE_TILE_W), tiles = tiles_x * cdiv(H, TH);
  MMSA_CHECK_ARG((long)tiles * B < (1l << 31), "%s: %d maps of %d x %d are more workgroups than a launch holds", name, B, H, W);
  const int Gk = guide ? G : 0;
  const VoteGeom g = {H, W, radius, all, half, TH, TH + 2 * radius, VOTE_TILE_W + 2 * radius, tiles_x, tiles, Hg, Wg, Gk, guide ? 255 * G + 1 : 0};
  const dim3 grid((unsigned)tiles * (unsigned)B);
  const size_t lds = vote_lds_bytes(g.rows, radius, Gk);
  if (guide) hipLaunchKernelGGL(vote_kernel<true>, grid, dim3(256), lds, stream, src, role, g, guide, range_lut, weight, out, support);
  else hipLaunchKernelGGL(vote_kernel<false>, grid, dim3(256), lds, stream, src, role, g, guide, range_lut, weight, out, support);
  MMSA_CHECK_LAUNCH("vote_filter_u8");
  return MMSA_OK;
}
