// Shared by the GEMM kernels on h8c operand planes (gemm_h8c.hip: the default kernel; gemm_h8c_w8.hip: fp8 weights; gemm_h8c4.hip: 4 waves): everything the
// three state in the same words -- tile index, scheduling vocabulary, the A operand's DMA stream, fragment offsets, the fp8 operand tuple, accumulator
// zeroing, the no-epilogue ablation.  The design notes stay with the kernels (gemm_h8c.hip first).  All of it is TEXT: macros expanded inside the kernel
// body, using its locals (a, wave, lane, l15, g, K, smem, acc, ...).  The kernels' scheduling is pinned by hand and their register budget is full; the rule
// for this header is that every kernel compiles to the instruction stream it had with the text written out (python tools/isa_scratch.py --digest <source>;
// profiles/gemm_shared_header_isa.txt).  That rule shaped two things: the lane constants come as H8C_*_HI() / H8C_*_LO() pairs because the kernels declare
// their W-side constants between them (the ORDER of these declarations shows in the register allocation), and the XCD remap of gemm_v2_shared.h is a macro.
#pragma once
#include "gemm_v2_shared.h"

typedef __attribute__((ext_vector_type(4))) unsigned h8c_u4;

// ---- output tile index -> batch, first row, first column; BM_ = rows per tile (256, or 128 for the 4-wave flavour), 128 columns
#define H8C_TILE(t_, BM_, bz_, m0_, n0_)                                                                    \
  { const int per_b_ = a.nbm * a.nbn; bz_ = (t_) / per_b_; const int r_ = (t_) - bz_ * per_b_; int tmi_, tni_;  \
    V2_TILE_MN(r_, tmi_, tni_); m0_ = tmi_ * (BM_); n0_ = tni_ * 128; }

// ---- scheduling and wait vocabulary: sched_barrier on both sides of every s_barrier; v_perm_b32 as volatile asm (the compiler sank it into the MFMA
// phase) taking q(hi) = the top bytes of two fp16 pairs; counted waits for the DMA stream
#define H8C_SB() __builtin_amdgcn_sched_barrier(0)
#define H8C_BAR() { H8C_SB(); __builtin_amdgcn_s_barrier(); H8C_SB(); }
#define H8C_PERM(d_, hi_, lo_) asm volatile("v_perm_b32 %0, %1, %2, %3" : "=v"(d_) : "v"(hi_), "v"(lo_), "s"(0x07050301u))
#define H8C_WAIT(n_) asm volatile("s_waitcnt vmcnt(" #n_ ")" ::: "memory")

// ---- DMA lane mapping of h8c planes.  HI: one instruction = 8 rows x 128 B (a row's 64-k chunk), lane -> (row = lane >> 3, LDS slot = lane & 7), the
// piece fetched into slot s of row r is s ^ ((r >> 1) & 7) (the fragment reads' swizzle, as gemm_v2).  LO: one instruction = one 16-row
// tile = 8 row-pair lines, lane -> (pair jj = lane >> 3, slot = lane & 7), piece = slot ^ f(jj >> 1), f = {0, 3, 2, 1}: with a pair's two
// rows in one 128-byte LDS row that permutation makes the 16 lanes of every ds_read_b128 lane group hit 16 distinct 16-byte bank groups.
#define H8C_DMA_LANE()                                                                                      \
  const int drow = lane >> 3;                                                                               \
  const int dpiece = ((lane & 7) ^ (drow >> 1)) * 16;                                                       \
  const int lq = ((lane & 7) ^ ((-(drow >> 1)) & 3)) * 16
// fragment offsets (HI image: the GEMM's LDS image of gemm_v2 with the two k-tiles of a chunk where it has hi | lo; LO image: a row pair per 128-byte row)
#define H8C_FRAG_HI()                                                                                       \
  const int fslot = g ^ ((l15 >> 1) & 7);                                                                   \
  const int frag0 = l15 * 128 + fslot * 16, frag1 = l15 * 128 + (fslot ^ 4) * 16
#define H8C_FRAG_LO() const int lo_off = 128 * (l15 >> 1) + 16 * ((((l15 & 1) << 2) | g) ^ ((-(l15 >> 2)) & 3))

// ---- the A operand's stream in the persistent 8-wave kernels (gemm_h8c.hip, gemm_h8c_w8.hip).  A lane's source offset inside an INTERIOR tile does not
// depend on the tile: lane constants (LA_E / LA_O: hi, even / odd 8-row group; LLA: lo) + scalar piece offsets + the cursor's scalar tile base.  Tiles that
// overhang M clamp their rows per lane, on the fly (general pairs only; the clamped rows' products are never stored).  No per-tile lane state: a spilled
// register reloaded in front of a DMA instruction would put an s_waitcnt vmcnt(0) -- the whole prefetch stream -- there.
// Uses ldaB (A's row-PAIR stride in bytes), K2 = 2 K, K4 = 4 K, lds_ha / lds_la (the wave's rows in a HI / LO unit).
#define H8C_A_LANE_HI() const unsigned LA_E = (unsigned)(drow >> 1) * ldaB + (unsigned)(drow & 1) * K2 + dpiece, LA_O = LA_E ^ 64u   /* (dpiece ^ 64: the sum's bit 6 is dpiece's: every other term is a multiple of 128) */
#define H8C_A_LANE_LO() const unsigned LLA = (unsigned)drow * ldaB + K4 + lq
#define H8C_HOFF(row_, m0_, ld_) (((unsigned)((row_) - (m0_)) >> 1) * (ld_) + ((unsigned)((row_) - (m0_)) & 1u) * K2)
// hi rows: sa_ = first row pair of the wave's 32 rows at the cursor's chunk (interior) / src_ = the tile's first row pair at that chunk (any tile)
#define H8C_A_HI_FAST(sa_, d_)                                                                              \
    GLDS16((sa_) + LA_E, (d_) + lds_ha); GLDS16((sa_) + 4u * ldaB + LA_O, (d_) + lds_ha + 1024);            \
    GLDS16((sa_) + 8u * ldaB + LA_E, (d_) + lds_ha + 2048); GLDS16((sa_) + 12u * ldaB + LA_O, (d_) + lds_ha + 3072);
#define H8C_A_HI_EDGE(src_, ab_, m0_, d_)                                                                   \
    GLDS16((src_) + (unsigned long)(H8C_HOFF(min(ab_, a.M - 1), m0_, ldaB) + dpiece), (d_) + lds_ha);        \
    GLDS16((src_) + (unsigned long)(H8C_HOFF(min(ab_ + 8, a.M - 1), m0_, ldaB) + (dpiece ^ 64)), (d_) + lds_ha + 1024); \
    GLDS16((src_) + (unsigned long)(H8C_HOFF(min(ab_ + 16, a.M - 1), m0_, ldaB) + dpiece), (d_) + lds_ha + 2048);       \
    GLDS16((src_) + (unsigned long)(H8C_HOFF(min(ab_ + 24, a.M - 1), m0_, ldaB) + (dpiece ^ 64)), (d_) + lds_ha + 3072);
// lo lines of one chunk: the wave's 16 row pairs
#define H8C_A_LO_FAST(sa_, d_) GLDS16((sa_) + LLA, (d_) + lds_la); GLDS16((sa_) + 8u * ldaB + LLA, (d_) + lds_la + 1024);
#define H8C_A_LO_OFF(aj_, m0_) ((unsigned)(min(aj_, (a.M - 1) >> 1) - ((m0_) >> 1)) * ldaB + K4 + lq)

// ---- lo pairs -> fp8 operand tuples (gemm_h8c.hip, gemm_h8c4.hip).  A operand: [q(hi) k-tile 0 | q(hi) k-tile 1 | lo 0 | lo 1], W operand:
// [lo 0 | lo 1 | q(hi) 0 | q(hi) 1] -- byte p of A meets byte p of W with the roles crossed: both cross terms of two k-tiles.
// Whole-tuple definitions: an element-wise assignment would keep the old tuple live (across the epilogue).
#define H8C_FP8_TUPLES(lb_)                                                                                           \
    _Pragma("unroll") for (int i = 0; i < 4; ++i) {                                                                   \
      const h8c_u4 lo_a_ = *reinterpret_cast<const h8c_u4*>((lb_) + fla + i * 1024);                                    \
      const h8c_u4 lo_w_ = *reinterpret_cast<const h8c_u4*>((lb_) + flw + i * 1024);                                    \
      int a0_, a1_, a2_, a3_, w0_, w1_, w2_, w3_;                                                                     \
      H8C_PERM(a0_, ah0[i][1], ah0[i][0]); H8C_PERM(a1_, ah0[i][3], ah0[i][2]);                                       \
      H8C_PERM(a2_, ah1[i][1], ah1[i][0]); H8C_PERM(a3_, ah1[i][3], ah1[i][2]);                                       \
      H8C_PERM(w0_, wh0[i][1], wh0[i][0]); H8C_PERM(w1_, wh0[i][3], wh0[i][2]);                                       \
      H8C_PERM(w2_, wh1[i][1], wh1[i][0]); H8C_PERM(w3_, wh1[i][3], wh1[i][2]);                                       \
      opA[i] = (mx_v8i){a0_, a1_, a2_, a3_, (int)lo_a_[0], (int)lo_a_[1], (int)lo_a_[2], (int)lo_a_[3]};                       \
      opW[i] = (mx_v8i){(int)lo_w_[0], (int)lo_w_[1], (int)lo_w_[2], (int)lo_w_[3], w0_, w1_, w2_, w3_};                       \
    }

// ---- accumulators acc[ni][mi]
#define H8C_ZERO_ACC()                                                                                      \
  _Pragma("unroll") for (int i = 0; i < 4; ++i)                                                             \
    _Pragma("unroll") for (int j_ = 0; j_ < 4; ++j_) acc[i][j_] = (f32x4){0.f, 0.f, 0.f, 0.f};
// timing ablation (debug-knob builds, V2_DBG == 2): no epilogue -- the accumulators are consumed and zeroed, the next pair skips its counted waits
#define H8C_NO_EPILOGUE()                                                                                   \
  { _Pragma("unroll") for (int i = 0; i < 4; ++i)                                                           \
      _Pragma("unroll") for (int j_ = 0; j_ < 4; ++j_) { asm volatile("" :: "v"(acc[i][j_])); acc[i][j_] = (f32x4){0.f, 0.f, 0.f, 0.f}; } \
    nowait = 1; }
