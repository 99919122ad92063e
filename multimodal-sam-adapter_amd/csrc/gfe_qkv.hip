// GFE qkv: qkv2(qkv1(x)) (AM:87-92: a grouped 1x1 conv c -> 3c followed by a grouped 3x3 conv 3c -> 3c, both 32 groups, no bias, nothing in
// between) as ONE grouped 3x3 conv with the folded weights W_eff[g][tap][ci][co] = sum_m q1[g][ci][m] q2[g][tap][m][co] (packed once,
// backbone._pack): cin_g = c / 32 = 3 / 6 / 12 / 24 inputs and cout_g = 3 cin_g outputs per group.  A third of the contraction of the
// 3x3 conv it replaces, no 1x1 launch and no 3c-wide intermediate.
//
// Work split.  A group's 3 ... 24 input channels are 12 ... 96 bytes of a pixel's row, so a workgroup that owns ONE group fetches whole
// 128-byte lines for a fraction of them (gconv_mfma.hip: 511 MB fetched for 151 MB at the 1/4-resolution level).  Here a workgroup owns a
// 16 x 16 pixel tile for a run of 24-channel CHUNKS (24 channels = 8 / 4 / 2 / 1 whole groups = 96 bytes in, 72 outputs = 288 contiguous
// bytes out per pixel); four chunks are three whole lines.  Per chunk the 18 x 18 halo of its 24 channels is staged in LDS once and every
// group of the chunk is computed from it on the fp32 matrix pipe, exactly as gconv3_mfma_kernel does (fp32 operands, fp32 accumulation):
//   D[pixel][co] = sum over k = (tap, ci) of x[pixel + tap][ci] * W_eff[k][co],  M = 256 pixels, N = cout_g (padded to 16 NT),
//   K = 9 cin_g FLATTENED over (tap, ci) and walked in MFMA k-steps of 4 (27 -> 7 steps, 54 -> 14; k >= K multiplies a zero weight).
//   * A fragment: lane (l15, kk) reads halo[ci(k)][(row + kh(k)) * 18 + l15 + kw(k)], k = 4 ks + kk; channel stride 336 floats (= 16 mod
//     64 banks): for cin_g = 12 / 24 the four kk of a wave are four consecutive channels, four disjoint 16-bank blocks;
//   * B fragment: lane (l15, kk) reads W_eff[g][k][16 nt + l15] straight from memory -- [tap][ci] IS the flattened k, the weights of a level
//     are 31 KB ... 2 MB shared by every workgroup, and a fragment is four 64-byte runs; columns >= cout_g and rows >= K read as zero;
//   * wave w owns pixel rows 4w .. 4w+3 (4 m-tiles) x NT n-tiles of the current group.
// Dispatch order as in gconv_tiled_kernel (conv.hip): tiles fastest, so the chunk runs of a pixel tile are in flight together.
#include "common.h"

template <int CIN_G>
__global__ __launch_bounds__(256, CIN_G == 24 ? 2 : 3) void gfe_qkv_kernel(const float* __restrict__ x, long ldx, const float* __restrict__ w, float* __restrict__ y,
                                                      long ldy, int H, int W, int tilesX, int chunks_per_wg) {
  constexpr int COUT_G = 3 * CIN_G, NT = (COUT_G + 15) / 16, K = 9 * CIN_G, KS = (K + 3) / 4;
  constexpr int CH = 24, GPC = CH / CIN_G, TW = 18, CST = 336;   // halo 18 x 18 = 324 floats per channel, padded to 336
  __shared__ float halo[CH * CST];
  const int b = blockIdx.z;
  const int tx0 = (blockIdx.x % tilesX) * 16, ty0 = (blockIdx.x / tilesX) * 16;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int l15 = lane & 15, kk = lane >> 4;

  // A-fragment offset of k-step ks for this lane's k = 4 ks + kk (a k beyond K reads k = K - 1's element against a zero weight).  cin_g = 12 / 24:
  // a k-step stays inside one tap, so the taps are a rolled loop of cin_g / 4 k-steps each and the offset is (ci0 + kk) * CST plus the tap's.
  constexpr bool TAPS = CIN_G % 4 == 0;
  constexpr int NOFF = TAPS ? 1 : KS;
  int aoff[NOFF];
  if constexpr (TAPS) {
    aoff[0] = kk * CST;
  } else {
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) {
      const int k = min(4 * ks + kk, K - 1);
      const int tap = k / CIN_G, ci = k - tap * CIN_G;
      const int kh = tap / 3, kw = tap - kh * 3;
      aoff[ks] = ci * CST + kh * TW + kw;
    }
  }

  for (int cc = 0; cc < chunks_per_wg; ++cc) {
    const int chunk = blockIdx.y * chunks_per_wg + cc;
    const float* xb = x + (long)b * H * W * ldx + chunk * CH;
    __syncthreads();   // the previous chunk is fully consumed
    // the loads of a lane in batches of 8 in flight before their LDS writes (gconv_tiled_kernel; all 31 at once cost more registers than the k loop)
    constexpr int NIT = (TW * TW * CH + 255) / 256, NB = 8;   // 31
#pragma unroll 1
    for (int it0 = 0; it0 < NIT; it0 += NB) {
      float v[NB];
#pragma unroll
      for (int it = 0; it < NB; ++it) {
        const int i = threadIdx.x + (it0 + it) * 256;
        const int pos = i / CH, ci = i - pos * CH;
        const int ly = pos / TW, lx = pos - ly * TW;
        const int iy = ty0 + ly - 1, ix = tx0 + lx - 1;
        v[it] = 0.f;
        if (pos < TW * TW && iy >= 0 && iy < H && ix >= 0 && ix < W) v[it] = xb[((long)iy * W + ix) * ldx + ci];
      }
#pragma unroll
      for (int it = 0; it < NB; ++it) {
        const int i = threadIdx.x + (it0 + it) * 256;
        const int pos = i / CH, ci = i - pos * CH;
        if (pos < TW * TW) halo[ci * CST + pos] = v[it];
      }
    }
    __syncthreads();

#pragma unroll 1
    for (int gl = 0; gl < GPC; ++gl) {
      const int g = chunk * GPC + gl;
      const float* wg = w + (long)g * K * COUT_G;                        // [tap][ci][co] = [k][co]
      const float* hb = halo + gl * CIN_G * CST + 4 * wave * TW + l15;
      f32x4 acc[4][NT];
#pragma unroll
      for (int mt = 0; mt < 4; ++mt)
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) acc[mt][nt] = (f32x4){0.f, 0.f, 0.f, 0.f};
      auto kstep = [&](const int k0 /* the step's first k: uniform */, const float* ha) {
        const int k = k0 + kk;
        float bf[NT], af[4];
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) {
          const int co = nt * 16 + l15;
          bf[nt] = 0.f;
          if ((K % 4 == 0 || k < K) && ((nt + 1) * 16 <= COUT_G || co < COUT_G)) bf[nt] = wg[k * COUT_G + co];
        }
#pragma unroll
        for (int mt = 0; mt < 4; ++mt) af[mt] = ha[mt * TW];
#pragma unroll
        for (int mt = 0; mt < 4; ++mt)
#pragma unroll
          for (int nt = 0; nt < NT; ++nt) acc[mt][nt] = __builtin_amdgcn_mfma_f32_16x16x4f32(af[mt], bf[nt], acc[mt][nt], 0, 0, 0);
      };
      if constexpr (TAPS) {
#pragma unroll 1
        for (int tap = 0; tap < 9; ++tap) {
          const float* ht = hb + aoff[0] + (tap / 3) * TW + tap % 3;
#pragma unroll
          for (int ks = 0; ks < CIN_G / 4; ++ks) kstep(tap * CIN_G + 4 * ks, ht + 4 * ks * CST);
        }
      } else {
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) kstep(4 * ks, hb + aoff[ks]);
      }
      // D: lane (l15 = output column within the n-tile, kk): pixels 4 kk + r of pixel row 4 wave + mt
#pragma unroll
      for (int mt = 0; mt < 4; ++mt) {
        const int oy = ty0 + 4 * wave + mt;
        if (oy >= H) continue;
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) {
          const int co = nt * 16 + l15;
          if (co >= COUT_G) continue;
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const int ox = tx0 + 4 * kk + r;
            if (ox < W) y[((long)b * H * W + (long)oy * W + ox) * ldy + g * COUT_G + co] = acc[mt][nt][r];
          }
        }
      }
    }
  }
}

template <int CIN_G>
static void launch_gfe_qkv(const float* x, long ldx, const float* w, float* y, long ldy, int B, int H, int W, int nchunks, hipStream_t stream) {
  const int tx = cdiv(W, 16), ty = cdiv(H, 16);
  // a workgroup walks up to four chunks (three whole lines of a pixel), fewer while the launch would leave the CUs short of workgroups
  int cpw = 4;
  while (cpw > 1 && (nchunks % cpw != 0 || (long)tx * ty * B * (nchunks / cpw) < 1024)) cpw >>= 1;
  hipLaunchKernelGGL((gfe_qkv_kernel<CIN_G>), dim3(tx * ty, nchunks / cpw, B), dim3(256), 0, stream, x, ldx, w, y, ldy, H, W, tx, cpw);
}

extern "C" int mmsa_gfe_qkv_conv(const float* x, long ldx, const float* w, float* y, long ldy, int B, int H, int W, int G, int cin_g,
                                 int cout_g, int* covered, hipStream_t stream) {
  MMSA_CHECK_ARG(x && w && y && covered && B > 0 && H > 0 && W > 0 && G > 0 && cin_g > 0 && cout_g > 0, "gfe_qkv_conv: bad args");
  MMSA_CHECK_ARG(ldx >= (long)G * cin_g && ldy >= (long)G * cout_g, "gfe_qkv_conv: row strides %ld / %ld shorter than the %d / %d channels", ldx, ldy,
                 G * cin_g, G * cout_g);
  *covered = 0;
  const int c = G * cin_g;
  if (cout_g != 3 * cin_g || c % 24 != 0 || B > 65535 || c / 24 > 65535) return MMSA_OK;
  switch (cin_g) {
    case 3: launch_gfe_qkv<3>(x, ldx, w, y, ldy, B, H, W, c / 24, stream); break;
    case 6: launch_gfe_qkv<6>(x, ldx, w, y, ldy, B, H, W, c / 24, stream); break;
    case 12: launch_gfe_qkv<12>(x, ldx, w, y, ldy, B, H, W, c / 24, stream); break;
    case 24: launch_gfe_qkv<24>(x, ldx, w, y, ldy, B, H, W, c / 24, stream); break;
    default: return MMSA_OK;   // not covered: the caller keeps the two mmsa_gconv_nhwc launches
  }
  MMSA_CHECK_LAUNCH("gfe_qkv_conv");
  *covered = 1;
  return MMSA_OK;
}
