// The band of a code map -- "some pixel within Chebyshev distance r holds another code" -- as the separable window-uniform test on dwords of staged codes,
// shared by csrc/boundary.hip (the counts per zone) and csrc/render_diag.hip (the picture of the band): ONE statement, so that the picture and the counts
// can never disagree.  The staging, the row pass and the column pass are described at the top of csrc/boundary.hip.
#pragma once

#define BND_MAX_RADIUS 32             // the largest radius the staged row pitch (bnd_pitch_dw) and a lane's two staged columns (64 + 2 r <= 128) serve
#define BND_TILE_W 64                 // tile columns: 16 dwords of row-pass bytes per row
#define BND_MIXED 0xFEFEFEFEu         // the row-pass byte of a window that is not uniform, in every byte

static inline int bnd_tile_h(int r) { return r <= 16 ? 64 : 32; }
static inline int bnd_pitch_dw(int r) { return BND_TILE_W / 4 + r / 2 + 1; }

// bytes s .. s + 3 of the dword pair (lo, hi)
__device__ __forceinline__ unsigned bnd_bytes(unsigned lo, unsigned hi, int s) { return (unsigned)(((((unsigned long long)hi) << 32) | lo) >> (8 * s)); }
// 0x80 in every byte of x that is not zero
__device__ __forceinline__ unsigned bnd_nonzero(unsigned x) { return (((x & 0x7f7f7f7fu) + 0x7f7f7f7fu) | x) & 0x80808080u; }

// one staged row of one map, four tile columns from dword `row`: the row-pass dword
__device__ __forceinline__ unsigned bnd_row_pass(const unsigned* row, int r) {
  const unsigned c = bnd_bytes(row[r >> 2], row[(r >> 2) + 1], r & 3);
  const int n = 2 * r + 1, nfull = n >> 2, rem = n & 3;        // n is odd: rem is 1 or 3
  unsigned acc = 0u, lo = row[0];
  for (int j = 0; j < nfull; ++j) {
    const unsigned hi = row[j + 1];
    acc |= (lo ^ c) | (bnd_bytes(lo, hi, 1) ^ c) | (bnd_bytes(lo, hi, 2) ^ c) | (bnd_bytes(lo, hi, 3) ^ c);
    lo = hi;
  }
  const unsigned hi = row[nfull + 1];                          // nfull + 1 <= r / 2 + 1: inside the row's pitch
  acc |= lo ^ c;
  if (rem == 3) acc |= (bnd_bytes(lo, hi, 1) ^ c) | (bnd_bytes(lo, hi, 2) ^ c);
  const unsigned mixed = (bnd_nonzero(acc) >> 7) * 0xffu;      // 0xff in every byte whose window is not uniform
  return (c & ~mixed) | (BND_MIXED & mixed);
}

// four tile pixels from dword `col` of the row-pass image (16 dwords per row): 0x80 in the byte of every pixel near a boundary
__device__ __forceinline__ unsigned bnd_col_pass(const unsigned* col, int r) {
  const unsigned c = col[r * (BND_TILE_W / 4)];
  unsigned acc = 0u;
  for (int k = 0; k <= 2 * r; ++k) acc |= col[k * (BND_TILE_W / 4)] ^ c;
  return bnd_nonzero(acc) | (~bnd_nonzero(c ^ BND_MIXED) & 0x80808080u);
}
