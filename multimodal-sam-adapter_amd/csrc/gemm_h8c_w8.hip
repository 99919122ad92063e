// h8c activations x W8 (fp8 e4m3) weights: the opt-in fp8 weight path of the ViT-block GEMMs (`model.fp8_weights`, mmsa/backbone.py).
// Same tiles (256 x 128, 8 waves, wave tile 64 x 64), persistent workgroups, tile order, A operand stream (h8c planes through LDS-DMA)
// and epilogue (gemm_v2_epilogue.inc -> gemm_epilogue_regs.inc) as gemm_h8c.hip -- read that file first; what the two share is the text of gemm_h8c_shared.h,
// so only the differences are written (and noted) here.
//
// Weights.  W_eff[n, k] = 2^e_n * e4m3(code[n, k]) (common.h "W8"): every value is exact in fp16, so its h8 lo part is zero and of the two
// cross terms of the h8 product only q(hi_W) . lo_A is left:
//   a . w ~= hi_a . w  +  lo_a . q(w)
// with w = the fp16 value converted in registers from the e4m3 code (v_cvt_scalef32_pk_f16_fp8 with the lane's column scale 2^e_n: exact) and
// q(w) = the TRUNCATED top byte of that fp16 value (v_perm_b32), as gemm_h8c.hip takes q(hi_A) -- the h8c lo bytes of A carry
// MMSA_H8C_LO_COMP for exactly that truncation, so the e4m3 code itself must NOT be the lo-term operand (it would bias the term by +9 %).
// The lo term of 128 k fits ONE block-scaled fp8 MFMA per 16 x 16 output (A operand [lo of chunk 2c | lo of chunk 2c + 1], W operand
// [q(w) of chunk 2c | q(w) of chunk 2c + 1], both e5m2, A scale MMSA_H8_MFMA_SCALE, W scale 127): per 32-wide k-block one fp16 MFMA + 1/4
// fp8 MFMA instead of 1 + 1/2.
//
// Loop.  The pair of gemm_h8c.hip (one 64-k chunk: phase X = hi fragments + 32 fp16 MFMAs, phase Y = lo fragments + the fp8 MFMAs) is kept,
// with the lo term cut per STEP of two chunks: an even chunk's phase Y only keeps q(w) of its chunk in registers (16), the odd chunk's phase Y
// reads A's lo bytes of both chunks, completes the tuples and issues the 16 fp8 MFMAs.  A step of 128 k is X Y' X Y: three matrix phases of 512
// cycles and one without matrix work instead of four.  The W side of a chunk is 64 code bytes per column (half of the column's 128-byte line):
// one LDS-DMA instruction per wave and chunk (16 columns x 64 B) instead of two hi + one lo instruction of h8c weights.  A's lo lines come per
// step (both chunks, 4 instructions per wave, requested in the even chunk's phase X) into LO units of 32 KiB: keeping the even chunk's lo bytes
// in registers instead spilled (28-39 scratch instructions per instantiation in the first build).
// LDS: HI unit = A hi (32 KiB, as gemm_h8c.hip) + the W codes of the chunk (8 KiB: column c at 64 c, its four 16-byte groups in slot order
// g ^ ((c >> 2) & 3): the 16 lanes of a ds_read_b128 lane group hit 16 distinct bank groups); two LO units with 16 KiB between them, so that
// (free LO unit + gap) is the epilogue's staging area, as in gemm_h8c.hip.
// Column scales: the wave's 64 exponent bytes of the output tile come with scalar LOADS (lgkmcnt: the k loop's DMA stream -- vmcnt -- is not
// touched) at the top of every output tile; a lane selects the four bytes of its columns.
#include "gemm_h8c_shared.h"

typedef __attribute__((ext_vector_type(2))) _Float16 hw_h2;

#define HW_H_UNIT 40960   // A hi 32 KiB + W codes 8 KiB
#define HW_L_UNIT 32768   // A lo of the two chunks of a step
#define HW_LDS_H(i_) ((i_) * HW_H_UNIT)
#define HW_LDS_L(i_) (2 * HW_H_UNIT + (i_) * (HW_L_UNIT + 16384))
#define HW_LDS_TOTAL (2 * HW_H_UNIT + 2 * HW_L_UNIT + 16384)   // 160 KiB

// 4 e4m3 codes (one dword) -> 4 fp16 (two dwords), scaled by 2^e: exact for codes x 2^e inside fp16 (e in [-15, 7], common.h W8)
__device__ __forceinline__ uint2 w8_cvt4(unsigned c, float s) {
  const hw_h2 lo = __builtin_amdgcn_cvt_scalef32_pk_f16_fp8(c, s, false);   // bytes 0, 1
  const hw_h2 hi = __builtin_amdgcn_cvt_scalef32_pk_f16_fp8(c, s, true);    // bytes 2, 3
  return make_uint2(__builtin_bit_cast(unsigned, lo), __builtin_bit_cast(unsigned, hi));
}

template <bool GEN, int ACT>
__global__ __launch_bounds__(512, 1) void gemm_h8c_w8_kernel(GemmV2Args a) {
  constexpr bool PP = true;
  constexpr bool EPI_UNROLL = ACT >= 0;
  constexpr int V2_BM = 256;
  constexpr int V2_NST = 3;   // (epilogue include: unused on the PP path)
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = wave >> 1, wn = wave & 1, grp = wave >> 2;
  const int l15 = lane & 15, g = lane >> 4;
  const int K = a.K;
  const int np = K >> 6;                      // 64-k chunks (pairs) per output tile: even (K % 128 == 0)
  const bool ni4 = true;
  const int swid = 64;
  const int G = gridDim.x;
  int rb = blockIdx.x;
  V2_XCD_REMAP(rb, G)
  const int my_tiles = (a.ntiles - rb + G - 1) / G;
  if (my_tiles <= 0) return;
  V2_SLACK_STAGGER(a, rb, G)
  const int total = my_tiles * np;
  const int nsteps = np >> 1, total_s = my_tiles * nsteps;   // 128-k steps per tile / of the stream (the LO cursor counts steps)

  // ---- DMA lane mapping.  A: as gemm_h8c.hip.  W: one instruction = 16 columns x 64 B of one chunk, lane -> (column wcol = lane >> 2,
  // LDS slot = lane & 3), the piece fetched into slot s of column c is s ^ ((c >> 2) & 3) (= s ^ ((lane >> 4) & 3): wave * 16 is a multiple of 16)
  H8C_DMA_LANE();
  const int lds_ha = wave * 32 * 128, lds_hw = 32768 + wave * 1024;
  const int lds_la = wave * 2048;
  const unsigned ldaB = (unsigned)(a.lda * 2);           // A row-PAIR stride in bytes
  const unsigned ldwB = (unsigned)(a.ldw * 2);           // W row stride in bytes (= K)
  const unsigned K2 = (unsigned)K * 2u, K4 = (unsigned)K * 4u;
  H8C_A_LANE_HI();
  const int wcol = lane >> 2;
  const unsigned wpiece = (unsigned)(((lane & 3) ^ ((lane >> 4) & 3)) * 16);
  const unsigned LW = (unsigned)wcol * ldwB + wpiece;
  H8C_A_LANE_LO();

  const unsigned char *hA, *hW, *lA;
  int h_m0 = 0, h_n0 = 0, l_m0 = 0, l_n0 = 0;
  bool h_edge = false, l_edge = false;
  int hp_tile = rb, hp_p = 0, hp_j = 0, lp_tile = rb, lp_p = 0, lp_j = 0;
#define HW_SET_H(t_)                                                                                        \
  { int bz_; H8C_TILE(t_, 256, bz_, h_m0, h_n0)                                                                   \
    hA = reinterpret_cast<const unsigned char*>(a.Ap + (long)bz_ * a.strideA + (long)(h_m0 >> 1) * a.lda);  \
    hW = reinterpret_cast<const unsigned char*>(a.Wp + (long)bz_ * a.strideW) + (long)h_n0 * ldwB;          \
    h_edge = h_m0 + 256 > a.M || h_n0 + 128 > a.N; }
#define HW_SET_L(t_)                                                                                        \
  { int bz_; H8C_TILE(t_, 256, bz_, l_m0, l_n0)                                                                   \
    lA = reinterpret_cast<const unsigned char*>(a.Ap + (long)bz_ * a.strideA + (long)(l_m0 >> 1) * a.lda);  \
    l_edge = l_m0 + 256 > a.M; }
  HW_SET_H(hp_tile) HW_SET_L(lp_tile)
#define HW_H_ISSUE_FAST()                                                                                   \
  { unsigned char* d_ = smem + HW_LDS_H(hp_j & 1);                                                          \
    const unsigned char* sa_ = hA + (long)hp_p * 128 + (unsigned long)((unsigned)(wave * 16) * ldaB);       \
    const unsigned char* sw_ = hW + (long)hp_p * 64 + (unsigned long)((unsigned)(wave * 16) * ldwB);        \
    H8C_A_HI_FAST(sa_, d_)                                                                                  \
    GLDS16(sw_ + LW, d_ + lds_hw); }
#define HW_L_ISSUE_FAST()                                                                                   \
  { unsigned char* d_ = smem + HW_LDS_L(lp_j & 1);                                                          \
    const unsigned char* sa_ = lA + (long)lp_p * 256 + (unsigned long)((unsigned)(wave * 16) * ldaB);       \
    H8C_A_LO_FAST(sa_, d_) H8C_A_LO_FAST(sa_ + 128, d_ + 16384) }
#define HW_H_ISSUE()                                                                                        \
  if (!h_edge) HW_H_ISSUE_FAST() else {                                                                     \
    unsigned char* d_ = smem + HW_LDS_H(hp_j & 1); const long ko_ = (long)hp_p * 128;                       \
    const int ab_ = h_m0 + wave * 32 + drow, wb_ = h_n0 + wave * 16 + wcol;                                  \
    H8C_A_HI_EDGE(hA + ko_, ab_, h_m0, d_)                                                                  \
    GLDS16(hW + (long)hp_p * 64 + (unsigned long)((unsigned)(min(wb_, a.N - 1) - h_n0) * ldwB + wpiece), d_ + lds_hw); }
#define HW_H_ADVANCE() { ++hp_j; if (++hp_p == np) { hp_p = 0; hp_tile += G; if (hp_j < total) HW_SET_H(hp_tile) } }
#define HW_L_ISSUE()                                                                                        \
  if (!l_edge) HW_L_ISSUE_FAST() else {                                                                     \
    unsigned char* d_ = smem + HW_LDS_L(lp_j & 1); const long ko_ = (long)lp_p * 256;                       \
    const int aj_ = (l_m0 >> 1) + wave * 16 + drow;                                                          \
    const unsigned o0_ = H8C_A_LO_OFF(aj_, l_m0), o1_ = H8C_A_LO_OFF(aj_ + 8, l_m0);                         \
    GLDS16(lA + ko_ + o0_, d_ + lds_la); GLDS16(lA + ko_ + o1_, d_ + lds_la + 1024);                         \
    GLDS16(lA + ko_ + 128 + o0_, d_ + 16384 + lds_la); GLDS16(lA + ko_ + 128 + o1_, d_ + 16384 + lds_la + 1024); }
#define HW_L_ADVANCE() { ++lp_j; if (++lp_p == nsteps) { lp_p = 0; lp_tile += G; if (lp_j < total_s) HW_SET_L(lp_tile) } }

  // ---- fragment offsets: A as gemm_h8c.hip; W codes of column cw = wn * 64 + ni * 16 + l15 (ni: + 1024 bytes per step), group g
  H8C_FRAG_HI();
  const int fha = (wm * 64) * 128;
  const int fcw = 32768 + (wn * 64 + l15) * 64 + ((g ^ ((l15 >> 2) & 3)) * 16);
  H8C_FRAG_LO();
  const int fla = (wm * 4) * 1024 + lo_off;

  f32x4 acc[4][4];   // [ni][mi]
  H8C_ZERO_ACC()
  h8c_u4 ah0[4], ah1[4];
  h8c_u4 cW[4];            // q(w) of the even chunk, completed into the fp8 tuples by the odd chunk
  float wsc[4];           // 2^e of the lane's four columns in the output tile being computed

  // column scales of output tile t_: the wave's 64 exponent bytes by scalar loads, lane l15 of group ni takes byte l15 of dwords 4 ni .. 4 ni + 3
  const signed char* wexp = reinterpret_cast<const signed char*>(a.Wp) + (long)a.N * ldwB;   // (batch 1: mmsa_gemm_v2_launch)
#define HW_SCALES(t_)                                                                                       \
  { int bz_, m0_, n0_; H8C_TILE(t_, 256, bz_, m0_, n0_) (void)bz_; (void)m0_;                                     \
    const __attribute__((address_space(4))) unsigned* e4_ =                                                 \
        (const __attribute__((address_space(4))) unsigned*)(wexp + n0_ + wn * 64);                          \
    int lane_s_ = lane; asm volatile("" : "+v"(lane_s_));                                                   \
    const int q_ = (lane_s_ & 15) >> 2, sh_ = (lane_s_ & 3) * 8;                                            \
    _Pragma("unroll") for (int ni = 0; ni < 4; ++ni) {                                                      \
      const unsigned d0_ = e4_[4 * ni], d1_ = e4_[4 * ni + 1], d2_ = e4_[4 * ni + 2], d3_ = e4_[4 * ni + 3]; \
      const unsigned d_ = q_ == 0 ? d0_ : q_ == 1 ? d1_ : q_ == 2 ? d2_ : d3_;                               \
      const int e_ = (int)(signed char)(unsigned char)(d_ >> sh_);                                           \
      wsc[ni] = __int_as_float((e_ + 127) << 23);                                                           \
    } }

  // ---- prologue: HI(0), HI(1), LO(step 0) of the stream
  HW_H_ISSUE() HW_H_ADVANCE()
  if (total > 1) { HW_H_ISSUE() HW_H_ADVANCE() }
  HW_L_ISSUE() HW_L_ADVANCE()
  H8C_WAIT(0);
  __builtin_amdgcn_s_barrier();

  int j = 0, tile = rb, nowait = 0;
// One pair (one 64-k chunk); barriers as gemm_h8c.hip.  ODD_ (literal): 0 = the even chunk of a 128-k step (phase X requests LO(step + 1), phase Y
// keeps q(w), no fp8 MFMA), 1 = the odd chunk (phase Y reads LO(step) and issues the 16 fp8 MFMAs of both chunks).  Stream order of one wave's DMA
// instructions: ... H(2s+1) [Y of 2s-1] | L(s+1) [X of 2s, 4] | H(2s+2) [Y of 2s, 5] | H(2s+3) [Y of 2s+1, 5] ...  Visibility (group 0 / 1 one barrier apart,
// every wave executes every wait): H(j+1) before the phase after d / c of pair j -- younger: 4 + 5 = 9 (j even) or 5 (j odd); L(s) before the phase
// after b / a of pair 2s+1 -- younger: 5 + 5 + 4 + 5 = 19; the waits a / b of an even pair need nothing.
#define HW_PAIR(FAST_, ODD_)                                                                                               \
  {                                                                                                                   \
    const unsigned char* hb = smem + HW_LDS_H(j & 1);                                                                 \
    const unsigned char* lb = smem + HW_LDS_L((j >> 1) & 1);                                                          \
    const bool last = !(FAST_) && p == np - 1;                                                                        \
    const bool tail = !(FAST_) && j + 2 >= total;                                                                     \
    const bool skipw = !(FAST_) && nowait > 0;                                                                        \
    /* ======== phase X, read part: A hi fragments, W codes */                                                                                   \
    _Pragma("unroll") for (int i = 0; i < 4; ++i) {                                                                   \
      ah0[i] = *reinterpret_cast<const h8c_u4*>(hb + fha + i * 2048 + frag0);                                         \
      ah1[i] = *reinterpret_cast<const h8c_u4*>(hb + fha + i * 2048 + frag1);                                         \
    }                                                                                                                 \
    h8c_u4 wc_[4];                                                                                                    \
    _Pragma("unroll") for (int i = 0; i < 4; ++i) wc_[i] = *reinterpret_cast<const h8c_u4*>(hb + fcw + i * 1024);    \
    H8C_SB();                                                                                                         \
    const bool do_l = !(ODD_) && ((FAST_) || lp_j < total_s);                                                         \
    if (!(ODD_)) { if (FAST_) { HW_L_ISSUE_FAST() } else if (do_l) { HW_L_ISSUE() } }                                 \
    H8C_SB();                                                                                                         \
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");                                                                \
    if (tail) H8C_WAIT(0); else if ((ODD_) && ((FAST_) || !skipw)) H8C_WAIT(19);                                      \
    H8C_BAR()                                                                                                         \
    /* ======== phase X, matrix part: per k-tile, codes -> fp16 (column scale), 16 fp16 MFMAs, q(w) = top bytes; the conversions sit here, */ \
    /* not in the read part: there the fp16 image of both k-tiles beside the codes spilled (first build) */           \
    h8c_u4 q_[4];                                                                                                     \
    _Pragma("unroll") for (int t = 0; t < 2; ++t) {                                                                   \
      h8c_u4 wt_[4];                                                                                                  \
      _Pragma("unroll") for (int i = 0; i < 4; ++i) {                                                                 \
        const uint2 x0_ = w8_cvt4(wc_[i][2 * t], wsc[i]), x1_ = w8_cvt4(wc_[i][2 * t + 1], wsc[i]);                   \
        wt_[i] = (h8c_u4){x0_.x, x0_.y, x1_.x, x1_.y};                                                                \
      }                                                                                                               \
      _Pragma("unroll") for (int ni = 0; ni < 4; ++ni)                                                                \
        _Pragma("unroll") for (int mi = 0; mi < 4; ++mi)                                                              \
          acc[ni][mi] = __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(mx_h8, wt_[ni]), __builtin_bit_cast(mx_h8, t ? ah1[mi] : ah0[mi]), acc[ni][mi], 0, 0, 0); \
      _Pragma("unroll") for (int i = 0; i < 4; ++i) {                                                                 \
        unsigned u0_, u1_;                                                                                            \
        H8C_PERM(u0_, wt_[i][1], wt_[i][0]); H8C_PERM(u1_, wt_[i][3], wt_[i][2]);                                     \
        q_[i][2 * t] = u0_; q_[i][2 * t + 1] = u1_;                                                                   \
      }                                                                                                               \
      H8C_SB();                                                                                                       \
    }                                                                                                                 \
    if (tail) H8C_WAIT(0); else if ((ODD_) && ((FAST_) || !skipw)) H8C_WAIT(19);                                      \
    H8C_BAR()                                                                                                         \
    /* ======== phase Y, read part (odd chunk): lo of A of both chunks (16 bytes each: k = 8g .. +7 and 32 + 8g .. +7 of a chunk) */ \
    mx_v8i opA[4], opW[4];                                                                                            \
    _Pragma("unroll") for (int i = 0; i < 4; ++i) {                                                                   \
      if (ODD_) {                                                                                                     \
        const h8c_u4 l0_ = *reinterpret_cast<const h8c_u4*>(lb + fla + i * 1024);                                    \
        const h8c_u4 l1_ = *reinterpret_cast<const h8c_u4*>(lb + 16384 + fla + i * 1024);                             \
        opA[i] = (mx_v8i){(int)l0_[0], (int)l0_[1], (int)l0_[2], (int)l0_[3], (int)l1_[0], (int)l1_[1], (int)l1_[2], (int)l1_[3]}; \
        opW[i] = (mx_v8i){(int)cW[i][0], (int)cW[i][1], (int)cW[i][2], (int)cW[i][3], (int)q_[i][0], (int)q_[i][1], (int)q_[i][2], (int)q_[i][3]}; \
      } else {                                                                                                        \
        cW[i] = q_[i];                                                                                                \
      }                                                                                                               \
    }                                                                                                                 \
    H8C_SB();                                                                                                         \
    const bool do_h = (FAST_) || hp_j < total;                                                                        \
    if (FAST_) { HW_H_ISSUE_FAST() } else if (do_h) { HW_H_ISSUE() }                                                   \
    H8C_SB();                                                                                                         \
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");                                                                \
    if (tail) H8C_WAIT(0); else if ((FAST_) || !skipw) { if (ODD_) H8C_WAIT(5); else H8C_WAIT(9); }                  \
    H8C_BAR()                                                                                                         \
    /* ======== phase Y, matrix part (odd chunk): 16 block-scaled fp8 MFMAs, K = 128 = the lo terms of both chunks */  \
    if (ODD_) {                                                                                                       \
      _Pragma("unroll") for (int ni = 0; ni < 4; ++ni)                                                                \
        _Pragma("unroll") for (int mi = 0; mi < 4; ++mi)                                                              \
          acc[ni][mi] = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(opW[ni], opA[mi], acc[ni][mi], 1, 1, 0, 0x7f7f7f7f, 0, MMSA_H8_MFMA_SCALE); \
    }                                                                                                                 \
    H8C_SB();                                                                                                         \
    if (FAST_) { if (!(ODD_)) { ++lp_j; ++lp_p; } ++hp_j; ++hp_p; } else { if (do_l) HW_L_ADVANCE() if (do_h) HW_H_ADVANCE() } \
    H8C_SB();                                                                                                         \
    if (tail || last) H8C_WAIT(0); else if ((FAST_) || !skipw) { if (ODD_) H8C_WAIT(5); else H8C_WAIT(9); }          \
    H8C_BAR()                                                                                                         \
    if (!(FAST_)) nowait = 0;                                                                                         \
    ++j;                                                                                                              \
  }

  for (int tdone = 0; tdone < my_tiles; ++tdone) {
    if (grp) H8C_BAR()
    bool interior;
    { int bz_, m0_, n0_; H8C_TILE(tile, 256, bz_, m0_, n0_) interior = m0_ + 256 <= a.M && n0_ + 128 <= a.N; }
    HW_SCALES(tile)
    int p = 0;
    HW_PAIR(0, 0)
    ++p;
    HW_PAIR(0, 1)
    ++p;
    if (interior) {
#pragma unroll 1
      for (; p < np - 2; p += 2) { HW_PAIR(1, 0) HW_PAIR(1, 1) }
      if (hp_p == np) { hp_p = 0; hp_tile += G; if (hp_j < total) HW_SET_H(hp_tile) }   // the straight-line pairs left the HI cursor at the end of this tile
      if (lp_p == nsteps) { lp_p = 0; lp_tile += G; if (lp_j < total_s) HW_SET_L(lp_tile) }   // ... and the LO cursor
    }
#pragma unroll 1
    for (; p < np; ) {
      HW_PAIR(0, 0)
      ++p;
      HW_PAIR(0, 1)
      ++p;
    }
    if (!grp) H8C_BAR()
    // ---- tile boundary (every DMA issued so far has landed: the last pair drained)
    if (V2_DBG(a) == 2) H8C_NO_EPILOGUE() else {
#define EPI_STAGING_BASE (smem + ((((j - 1) >> 1) & 1) ? HW_LDS_L(1) - 16384 : HW_LDS_L(0)))   // the last step's LO unit + the gap
#include "gemm_v2_epilogue.inc"
    }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    H8C_BAR()   // the staging area is free again
    tile += G;
  }
}

// Launch (called by mmsa_gemm_v2_launch in gemm_v2.hip for fmt = MMSA_FMT_W8: A = h8c planes, W = W8 weights, batch 1).
int mmsa_gemm_h8c_w8_dispatch(const GemmV2Args& a, int grid, bool gen, int act, hipStream_t stream) {
  static MmsaPerDevice per_dev_ = {};
  (void)mmsa_per_device(per_dev_, [] {
#define HW_ATTR(GEN_, ACT_) (void)hipFuncSetAttribute((const void*)gemm_h8c_w8_kernel<GEN_, ACT_>, hipFuncAttributeMaxDynamicSharedMemorySize, HW_LDS_TOTAL);
    V2_EPI_TABLE(HW_ATTR)
#undef HW_ATTR
  });
#define HW_LAUNCH(GEN_, ACT_) if (v2_epi_serves(gen, act, GEN_, ACT_)) hipLaunchKernelGGL((gemm_h8c_w8_kernel<GEN_, ACT_>), dim3(grid), dim3(512), HW_LDS_TOTAL, stream, a);
  V2_EPI_TABLE(HW_LAUNCH)
#undef HW_LAUNCH
  MMSA_CHECK_LAUNCH("gemm_split3(h8c x w8)");
  return MMSA_OK;
}
