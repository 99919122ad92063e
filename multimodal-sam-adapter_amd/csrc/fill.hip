// Nearest-label fill on device (mmsa_fill_nearest_u8): every HOLE pixel of a byte map takes the value of the nearest SOURCE pixel of its image within `cap`
// pixels (Euclidean), so that a class map whose small blobs, dropped segments or unsure pixels were painted over is handed back as a full map.  Integers
// only: the same bytes run after run.
//
// The quantity.  role[256] gives every byte one of three roles: 0 = source (keeps its value and offers it), 1 = hole (is to be filled), 2 = inert (keeps its
// value, offers nothing, blocks nothing: the fill is Euclidean, not geodesic).  For a hole p = (py, px):
//   q* = the source pixel q of the image with d2 = (qy - py)^2 + (qx - px)^2 <= cap^2 and the smallest key (d2, qy, qx), compared lexicographically
//        (nearest first, then topmost, then leftmost);  out[p] = M[q*], d2[p] = its d2;  no such q: out[p] = M[p], d2[p] = 65535 (FILL_FAR).
//   Every pixel that is not a hole: out[p] = M[p], d2[p] = 0.
// The key is separable.  Within one row the nearest source to column px has the smallest |dx|, and of a left and a right source equally far the left one has
// the smaller qx.  Across rows a candidate is the row's nearest source at its row distance g: keys (dy^2 + g^2, qy).
//
// Two launches in the frame of csrc/row_scan.h, no dependence between workgroups inside either, every loop bounded by the row length, by cap or by the
// image height:
//   row pass     the row pass of csrc/row_scan.h with a source pixel as the marked index: a lane finds the first and the last source of its piece, row_scan
//                gives it the last source before and the first source after the piece, and the lane walks its piece again and writes, per pixel, ONE
//                uint16 into the scratch plane [B, H, W]: the value of the row's nearest source (left on ties) in the low byte, the distance g (0 at a
//                source) in the high byte.  No source of the row within 255 columns: the low byte is `none_byte`, a hole byte, which is the value of no
//                source.
//   column pass  a lane per pixel, a wave on 64 consecutive x.  A lane whose own pixel is no hole copies it and leaves (a wave without holes: one read).  A
//                hole lane walks dy = 0, 1, 2, ... over both rows at distance dy while dy <= min(cap, max(y, H - 1 - y)) and dy^2 <= best: one coalesced
//                128-byte read of the scratch plane per wave and row.  The row above at the same d2 beats what was found (its qy is smaller: <=), the row
//                below never does (<), and the loop still enters the dy whose dy^2 equals best, for the row above it.
// out may be src: a lane of the column pass reads its own pixel of src and the scratch plane, nothing else.
#include "common.h"
#include "row_scan.h"

#define FILL_FAR 65535
#define FILL_MAX_CAP 255
#define FILL_ROLE_SOURCE 0
#define FILL_ROLE_HOLE 1
#define FILL_BIG (1 << 20)        // a row distance no uint8 holds

// rows = B * H; the workgroup blockIdx.x owns one row
__global__ __launch_bounds__(256) void fill_rows_kernel(const unsigned char* __restrict__ src, const unsigned char* __restrict__ role, int W, int none_byte,
                                                        unsigned short* __restrict__ plane) {
  __shared__ unsigned char role_s[256];
  __shared__ int wave_last[4], wave_first[4];
  const long row = blockIdx.x;
  const unsigned char* __restrict__ srow = src + row * W;
  unsigned short* __restrict__ prow = plane + row * W;
  int x0, x1, before, after;
  row_piece(W, x0, x1);
  role_s[threadIdx.x] = role[threadIdx.x];
  __syncthreads();

  // 1. the first and the last source of this lane's piece
  int fs = ROW_NONE, ls = -1;
  for (int x = x0; x < x1; ++x) {
    if (role_s[srow[x]] == FILL_ROLE_SOURCE) {
      fs = min(fs, x);
      ls = x;
    }
  }
  // 2. the last source in front of the piece, the first source behind it (every lane of the workgroup is here: a row is a workgroup's)
  row_scan(fs, ls, wave_last, wave_first, before, after);
  if (x0 >= x1) return;

  // 3. stretch by stretch: the pixels [a, x) that are no sources lie between the source `st` (-1: none to the left) and the source `en` (ROW_NONE: none to the
  //    right); before and after are indices of this row, 0 <= before < x0 and x1 <= after < W where there are any
  const unsigned short none = (unsigned short)(none_byte | (255 << 8));
  int a = x0, st = before, stv = before >= 0 ? (int)srow[before] : 0;
  for (int x = x0; x <= x1; ++x) {
    int en = ROW_NONE, env = 0;
    if (x < x1) {
      env = srow[x];
      if (role_s[env] != FILL_ROLE_SOURCE) continue;
      en = x;
    } else if (after != ROW_NONE) {
      en = after;
      env = srow[after];
    }
    for (int q = a; q < x; ++q) {                                            // every pixel of the piece is written once
      const int dl = st >= 0 ? q - st : FILL_BIG, dr = en != ROW_NONE ? en - q : FILL_BIG;
      const int g = min(dl, dr), v = dl <= dr ? stv : env;                   // equally far: the left one
      prow[q] = g <= 255 ? (unsigned short)(v | (g << 8)) : none;
    }
    if (x < x1) prow[x] = (unsigned short)env;                               // a source: its own value at distance 0
    st = x;
    stv = env;
    a = x + 1;
  }
}

// the grid of col_tile (csrc/row_scan.h).  src and out may be one buffer: no __restrict__ on them.
__global__ __launch_bounds__(256) void fill_cols_kernel(const unsigned char* src, const unsigned char* __restrict__ role,
                                                        const unsigned short* __restrict__ plane, int H, int W, int tiles_x, int groups_y, int none_byte, int cap,
                                                        unsigned char* out, unsigned short* __restrict__ d2) {
  __shared__ unsigned char role_s[256];
  role_s[threadIdx.x] = role[threadIdx.x];
  int b, y, x;
  const bool inside = col_tile(H, W, tiles_x, groups_y, b, y, x);
  const long at = ((long)b * H + (inside ? y : 0)) * W + (inside ? x : 0);
  const int own = src[at];                                                   // a pixel of the map for the lanes outside too: they write nothing
  __syncthreads();
  if (!inside) return;
  if (role_s[own] != FILL_ROLE_HOLE) {
    out[at] = (unsigned char)own;
    if (d2) d2[at] = 0;
    return;
  }
  const unsigned short* __restrict__ col = plane + (long)b * H * W + x;
  const int limit = cap * cap;
  int best = limit + 1, val = own;
  {
    const int v = col[(long)y * W], g = v >> 8;                              // the own row: g >= 1, a hole is no source
    if ((v & 255) != none_byte && g * g <= limit) {
      best = g * g;
      val = v & 255;
    }
  }
  const int reach = min(cap, max(y, H - 1 - y));                            // no row of the image lies further
  for (int dy = 1; dy <= reach && dy * dy <= best; ++dy) {
    if (y - dy >= 0) {
      const int v = col[(long)(y - dy) * W], g = v >> 8, d = dy * dy + g * g;
      if ((v & 255) != none_byte && d <= limit && d <= best) {               // a row further up at the same d2: the smaller qy
        best = d;
        val = v & 255;
      }
    }
    if (y + dy < H) {
      const int v = col[(long)(y + dy) * W], g = v >> 8, d = dy * dy + g * g;
      if ((v & 255) != none_byte && d < best) {                              // best <= limit + 1: d < best keeps d <= limit
        best = d;
        val = v & 255;
      }
    }
  }
  out[at] = (unsigned char)val;
  if (d2) d2[at] = (unsigned short)(best <= limit ? best : FILL_FAR);
}

extern "C" int mmsa_fill_nearest_u8(const unsigned char* src, int B, int H, int W, const unsigned char* role, int none_byte, int cap, unsigned short* scratch,
                                    unsigned char* out, unsigned short* d2, hipStream_t stream) {
  const char* name = "fill_nearest_u8";
  MMSA_CHECK_ARG(src && role && scratch && out, "%s: src, role, scratch and out are required", name);
  MMSA_CHECK_ARG(scratch != d2 && (const void*)scratch != (const void*)src && (void*)scratch != (void*)out && (void*)d2 != (void*)out &&
                     (const void*)d2 != (const void*)src,
                 "%s: scratch and d2 are two planes, and neither is src or out", name);
  MMSA_CHECK_ARG(B > 0 && H > 0 && W > 0 && (long)H * W < (1l << 31), "%s: bad map size", name);
  MMSA_CHECK_ARG(cap >= 1 && cap <= FILL_MAX_CAP, "%s: cap = %d; 1..%d are supported (cap^2 must fit the uint16 map below 65535)", name, cap, FILL_MAX_CAP);
  MMSA_CHECK_ARG(none_byte >= 0 && none_byte <= 255, "%s: none_byte = %d; a byte 0..255 whose role is 1 (a hole) is expected", name, none_byte);
  RowColGrid g;
  const int rc = row_col_grid(name, B, H, W, g);
  if (rc) return rc;
  hipLaunchKernelGGL(fill_rows_kernel, dim3((unsigned)g.rows), dim3(256), 0, stream, src, role, W, none_byte, scratch);
  hipLaunchKernelGGL(fill_cols_kernel, dim3((unsigned)g.blocks), dim3(256), 0, stream, src, role, scratch, H, W, g.tiles_x, g.groups_y, none_byte, cap, out, d2);
  MMSA_CHECK_LAUNCH("fill_nearest_u8");
  return MMSA_OK;
}
