// Register-resident tile epilogue of the LDS-DMA GEMM kernels (round 5), included textually by gemm_v2_epilogue.inc in front of the
// LDS-staged epilogue.  Same arithmetic, same call sites (IE:154-167,488,499; AM:447-451; TC:107-111; ops/modules/ms_deform_attn.py:103-129).
//
// Why.  The ISA of the staged epilogue (round 4) showed what its 19-26 k cycles per 256 x 128 tile were made of: every run-time-uniform
// case distinction inside the sub-tile loop (output format, row-normalising form, null pointers, ragged rows) is a scalar branch -- 170 per
// wave and tile -- and at every join behind a branch that contains a load the compiler can only wait with s_waitcnt vmcnt(0); vmcnt retires
// in order and counts stores, so each sub-tile began by draining the previous sub-tile's global stores (four exposed store round trips per
// tile, in a phase in which every CU of the chip is storing).  On top: two LDS round trips per sub-tile, 229 v_readlane reloads of spilled
// scalars, 128 ds_bpermute for the strip sums.  This version, for INTERIOR tiles (whole 256 x 128 tile inside M x N, 16-byte aligned
// operands) of the configurations the model runs:
//   * every case is a compile-time parameter of one generic lambda: the sub-tile loop is straight-line code, the compiler places counted
//     waits; all loads of a tile (column vectors, row mean / rstd of the four sub-tiles, residual rows one sub-tile ahead) are issued
//     before the stores they would otherwise queue behind;
//   * operand planes are stored straight from the accumulator layout (lane = row l15, columns 16 ni + 4 g .. + 3), no LDS: widened to 16 bytes
//     per lane with v_permlane16_swap_b32 (gfx950: exchanges lanes
//     l <-> l ^ 16, i.e. g <-> g ^ 1, between the registers of two neighbouring n-tiles), which gives 64 contiguous bytes per row and
//     instruction in every plane format -- and for the h8c lo bytes whole 128-byte lines (a row pair's two halves);
//   * fp32-ONLY outputs go once per 16-row sub-tile through the wave's staging rows in LDS and leave as 256-byte row segments (epi_rows_ below: stored from the
//     accumulator layout they are 16 rows x 64 B per instruction, which measured a wash against the staged epilogue);
//   * the strip sums of the LayerNorm fold (rs_out) are two swap + add steps per sub-tile instead of eight ds_bpermute per row group.
// Everything else (ragged tiles, pixel-shuffle stores, split plane formats, other activations) runs the staged code below.
// What a tile boundary costs with this epilogue is issue time of its arithmetic, not stores and not load latency (cycle stamps: profiles/r05_epi_stamps.txt; issue
// costs: profiles/r05_gelu_forms.txt) -- hence the one-transcendental GELU of common.h; the same arithmetic
// in packed pairs (v_pk_fma_f32 for bias / row norm / scale / residual) measured within 0.5 % and is not used.
//
// Expects in scope what gemm_v2_epilogue.inc has set up: a, bz, m0, n0, nb_, bias, colscale, resid, C, Cp, cp_base, cp_split, cp_kpad,
// wm, l15, g, ni4, acc[4][4]; defines `regs_done`.
#ifndef MMSA_EPI_REGS
#define MMSA_EPI_REGS 1   // 0 (A/B builds): every tile runs the LDS-staged epilogue
#endif
#ifndef MMSA_EPI_REGS_FP32
#define MMSA_EPI_REGS_FP32 0   // 1 (A/B builds): fp32-ONLY outputs (no planes beside them) take this path too.  Measured a wash (profiles/r05_epilogue_regs.txt:
                               // fc1 / value projections -3 ... -9 %, extractor output projection +2 ... +9 %, the N = 192 / 576 projections +4 ... +18 %): their
                               // epilogues are bound by the chip-wide read-modify-write burst on the 176 MB adapter tensor, where 16 rows x 64 B per store
                               // instruction touch twice the lines of the staged epilogue's 4 rows x 256 B -- and a launch whose ragged last column tile runs the
                               // staged code beside this one no longer fits the instruction cache.  Off: they keep the staged epilogue.
#endif
#ifndef MMSA_EPI_ROWS
#define MMSA_EPI_ROWS 1        // 0 (A/B builds): fp32-only outputs keep the staged epilogue
#endif
#ifndef MMSA_EPI_NOSTORE
#define MMSA_EPI_NOSTORE 0     // 1 (timing builds, results garbage): everything but the global stores of this path
#endif
#if MMSA_EPI_NOSTORE
#define EPI_ST16(ptr_, val_) { const uint4 v__ = __builtin_bit_cast(uint4, val_); asm volatile("" :: "v"(v__.x), "v"(v__.y), "v"(v__.z), "v"(v__.w), "v"(ptr_)); }
#else
#define EPI_ST16(ptr_, val_) { *reinterpret_cast<uint4*>(ptr_) = __builtin_bit_cast(uint4, val_); }
#endif
#ifndef EPI_STAMP
#define EPI_STAMP(i_)
#define EPI_STAMP_WAIT()
#define EPI_STAMP_DEFAULTED_ 1
#endif
      bool regs_done = false;
      if constexpr (MMSA_EPI_REGS && EPI_UNROLL && !GEN && (ACT == ACT_NONE || ACT == ACT_GELU)) {
        const bool interior_ = m0 + V2_BM <= a.M && n0 + a.bn <= a.N;   // (96-column tiles: the "rows" form only)
        const bool al16_ = ((((uintptr_t)bias) | ((uintptr_t)colscale) | ((uintptr_t)resid) | ((uintptr_t)C) | ((uintptr_t)Cp) | ((uintptr_t)a.rn_cs)) & 15) == 0 &&
                           ((a.ldc | a.ldr) & 3) == 0 && (a.ldcp & 7) == 0 && (a.strideBias & 3) == 0;
        if (interior_ && al16_ && V2_DBG(a) == 0 && !cp_split && (ni4 || (C && !Cp && !a.rs_out && !a.rn_mr))) {
          auto swap16_ = [](unsigned& x_, unsigned& y_) {   // x of lanes 16..31 / 48..63 <-> y of lanes 0..15 / 32..47
            const auto r_ = __builtin_amdgcn_permlane16_swap(x_, y_, false, false);
            x_ = r_[0]; y_ = r_[1];
          };
          auto epi_regs_ = [&](auto c_C, auto c_R, auto c_CPF, auto c_RS, auto c_RN, auto c_CS) {
            constexpr bool kC = decltype(c_C)::value, kR = decltype(c_R)::value, kRS = decltype(c_RS)::value, kRN = decltype(c_RN)::value;
            constexpr bool kCS = decltype(c_CS)::value;    // a per-column scale (colscale, alpha != 1): 16 registers most sites do not need
            constexpr int kCPF = decltype(c_CPF)::value;   // plane format of Cp, -1: no planes output
            const int row0 = m0 + wm * 64 + l15;           // + 16 mi
            const int col0 = nb_ + 4 * g;                  // + 16 ni
            float4 bn_[4], cn_[4], sn_[4];
#pragma unroll
            for (int ni = 0; ni < 4; ++ni) {
              const int ci = col0 + ni * 16;
              bn_[ni] = bias ? *reinterpret_cast<const float4*>(bias + ci) : make_float4(0.f, 0.f, 0.f, 0.f);
              if constexpr (kCS) {
                cn_[ni] = colscale ? *reinterpret_cast<const float4*>(colscale + ci) : make_float4(1.f, 1.f, 1.f, 1.f);
                cn_[ni].x *= a.alpha; cn_[ni].y *= a.alpha; cn_[ni].z *= a.alpha; cn_[ni].w *= a.alpha;
              }
              if constexpr (kRN) sn_[ni] = *reinterpret_cast<const float4*>(a.rn_cs + (long)bz * a.strideBias + ci);
            }
            float2 mr_[4];
            if constexpr (kRN) {
#pragma unroll
              for (int mi = 0; mi < 4; ++mi) mr_[mi] = *reinterpret_cast<const float2*>(a.rn_mr + 2 * ((long)bz * a.M + row0 + 16 * mi));
            }
            // residual rows: ALL sixteen loads of the tile in flight at once (64 registers -- the k loop's fragments are dead here).  One sub-tile ahead (4 KiB per wave
            // in flight) left a CU with 32 KiB of outstanding reads against ~2 us of loaded-memory latency, i.e. ~16 GB/s per CU: the read-modify-write epilogues
            // of the adapter-token GEMMs ran at that, not at the chip's bandwidth (profiles/r05_epilogue_regs.txt, slack-stagger experiment).
#ifndef MMSA_EPI_PREFETCH_ALL
#define MMSA_EPI_PREFETCH_ALL 0   // 1 (A/B builds): all sixteen residual loads of a tile up front -- measured no faster (the read-modify-write epilogues are bandwidth-bound,
                                  // profiles/r05_epilogue_regs.txt), and the 48 extra live registers push loop invariants of the kernel into scratch
#endif
            float4 rra[4][4];
            const float* rbase = nullptr;
            if constexpr (kR) {
              rbase = resid + (long)row0 * a.ldr + col0;
#pragma unroll
              for (int mi = 0; mi < (MMSA_EPI_PREFETCH_ALL ? 4 : 1); ++mi)
#pragma unroll
                for (int ni = 0; ni < 4; ++ni) rra[mi][ni] = *reinterpret_cast<const float4*>(rbase + (long)mi * 16 * a.ldr + ni * 16);
            }
            EPI_STAMP(1) EPI_STAMP_WAIT() EPI_STAMP(2)
            float* cbase = nullptr;
            if constexpr (kC) cbase = C + (long)row0 * a.ldc + col0;
            // plane addressing: hcol = this lane's 8 columns inside a 32-column group after the swap, schunk = its 16-byte chunk of the group's
            // second half (h8 lines: lo | q(hi) chunk; h8c: lo group of the 64-column chunk)
            const int hcol = 16 * (g & 1) + 8 * (g >> 1);
            const int schunk = 16 * (2 * (g & 1) + (g >> 1));
            unsigned short* prow = nullptr;    // this lane's plane row (h8c: its hi row), sub-tile 0
            unsigned char* plo = nullptr;      // h8c: this lane's 16-byte lo group, sub-tile 0
            long pstep = 0;                    // uint16 units per 16 rows
            if constexpr (kCPF == MMSA_FMT_H8C) {
              unsigned short* pb = Cp + (long)(row0 >> 1) * a.ldcp;
              prow = pb + (row0 & 1) * cp_kpad + nb_ + hcol;
              plo = reinterpret_cast<unsigned char*>(pb + 2 * cp_kpad) + (row0 & 1) * 64 + ((nb_ >> 6) << 7) + schunk;
              pstep = 8 * a.ldcp;
            } else if constexpr (kCPF >= 0) {
              prow = Cp + (long)row0 * a.ldcp + ((nb_ >> 5) << 6) + hcol;
              pstep = 16 * a.ldcp;
            }
            // clamp watch (common.h) without a vector register: a lane mask of "this lane converted a value beyond the format's range", OR-ed in scalar
            // registers (a running per-lane maximum cost the ACT_NONE instantiation ~20 more scratch instructions and its sites 3 ... 9 %:
            // profiles/r05_clamp_watch.txt).  What is reported is therefore the format's limit, not the magnitude met.
            unsigned long long cwm_ = 0ull;
            constexpr bool kWatch = MMSA_CLAMP_WATCH && MMSA_CW_REGS && (kCPF == MMSA_FMT_H8C || kCPF == MMSA_FMT_H8 || kCPF == MMSA_FMT_F3);
            constexpr float kLimit = (kCPF == MMSA_FMT_F3) ? MMSA_F3_MAX : MMSA_H8_MAX;
            float* rsb = nullptr;
            if constexpr (kRS) rsb = a.rs_out + (((long)bz * a.M + row0) * a.rs_strips + (nb_ >> 6)) * 2;
#pragma unroll
            for (int mi = 0; mi < 4; ++mi) {
              if constexpr (kR && !MMSA_EPI_PREFETCH_ALL) {
                if (mi < 3) {
#pragma unroll
                  for (int ni = 0; ni < 4; ++ni) rra[mi + 1][ni] = *reinterpret_cast<const float4*>(rbase + (long)(mi + 1) * 16 * a.ldr + ni * 16);
                }
              }
              float s1 = 0.f, s2 = 0.f;
              uint2 H[4], Lp[4];        // hi halves; second halves of the 16-bit pair formats
              unsigned L8[4], Q8[4];    // h8 / h8c: lo bytes, q(hi) bytes
#pragma unroll
              for (int ni = 0; ni < 4; ++ni) {
                float4 o;
                if constexpr (kRN) {
                  const float mu = mr_[mi].x, rs = mr_[mi].y;
                  o = make_float4(fmaf(rs, fmaf(-mu, sn_[ni].x, acc[ni][mi][0]), bn_[ni].x), fmaf(rs, fmaf(-mu, sn_[ni].y, acc[ni][mi][1]), bn_[ni].y),
                                  fmaf(rs, fmaf(-mu, sn_[ni].z, acc[ni][mi][2]), bn_[ni].z), fmaf(rs, fmaf(-mu, sn_[ni].w, acc[ni][mi][3]), bn_[ni].w));
                } else {
                  o = make_float4(acc[ni][mi][0] + bn_[ni].x, acc[ni][mi][1] + bn_[ni].y, acc[ni][mi][2] + bn_[ni].z, acc[ni][mi][3] + bn_[ni].w);
                }
                acc[ni][mi] = (f32x4){0.f, 0.f, 0.f, 0.f};
                if constexpr (ACT == ACT_GELU) o = gelu4(o);
                if constexpr (kCS) { o.x *= cn_[ni].x; o.y *= cn_[ni].y; o.z *= cn_[ni].z; o.w *= cn_[ni].w; }
                if constexpr (kR) { o.x += a.beta * rra[mi][ni].x; o.y += a.beta * rra[mi][ni].y; o.z += a.beta * rra[mi][ni].z; o.w += a.beta * rra[mi][ni].w; }
                if constexpr (kC) EPI_ST16(cbase + (long)mi * 16 * a.ldc + ni * 16, o)
                if constexpr (kRS) {
                  s1 += (o.x + o.y) + (o.z + o.w);
                  s2 += fmaf(o.x, o.x, o.y * o.y) + fmaf(o.z, o.z, o.w * o.w);
                }
                if constexpr (kWatch) cwm_ |= __builtin_amdgcn_ballot_w64(fmaxf(fmaxf(fabsf(o.x), fabsf(o.y)), fmaxf(fabsf(o.z), fabsf(o.w))) > kLimit);
                if constexpr (kCPF == MMSA_FMT_H8C) h8_split4<true>(o, H[ni], L8[ni], Q8[ni]);
                else if constexpr (kCPF == MMSA_FMT_H8) h8_split4<false>(o, H[ni], L8[ni], Q8[ni]);
                else if constexpr (kCPF == MMSA_FMT_F3) f3_split4(o, H[ni], Lp[ni]);
                else if constexpr (kCPF == MMSA_FMT_B3) split4(o, H[ni], Lp[ni]);
              }
              if constexpr (kCPF >= 0) {
                unsigned short* pr = prow + (long)mi * pstep;
#pragma unroll
                for (int p = 0; p < 2; ++p) {   // n-tiles 2p, 2p+1 = columns 32p .. 32p+31 of the strip
                  swap16_(H[2 * p].x, H[2 * p + 1].x);
                  swap16_(H[2 * p].y, H[2 * p + 1].y);
                  const uint4 hv = make_uint4(H[2 * p].x, H[2 * p].y, H[2 * p + 1].x, H[2 * p + 1].y);
                  if constexpr (kCPF == MMSA_FMT_H8C) {
                    EPI_ST16(pr + 32 * p, hv)
                  } else {
                    EPI_ST16(pr + 64 * p, hv)
                    if constexpr (kCPF == MMSA_FMT_H8) {
                      swap16_(L8[2 * p], L8[2 * p + 1]);
                      swap16_(Q8[2 * p], Q8[2 * p + 1]);
                      EPI_ST16(reinterpret_cast<unsigned char*>(pr + 64 * p - hcol) + 64 + schunk, make_uint4(L8[2 * p], L8[2 * p + 1], Q8[2 * p], Q8[2 * p + 1]))
                    } else {
                      swap16_(Lp[2 * p].x, Lp[2 * p + 1].x);
                      swap16_(Lp[2 * p].y, Lp[2 * p + 1].y);
                      EPI_ST16(pr + 64 * p + 32, make_uint4(Lp[2 * p].x, Lp[2 * p].y, Lp[2 * p + 1].x, Lp[2 * p + 1].y))
                    }
                  }
                }
                if constexpr (kCPF == MMSA_FMT_H8C) {   // lo bytes: one 16-byte group per lane, a row pair's two 64-byte halves = one whole line
                  swap16_(L8[0], L8[1]);
                  swap16_(L8[2], L8[3]);
                  EPI_ST16(plo + (long)mi * pstep * 2, make_uint4(L8[0], L8[1], L8[2], L8[3]))
                }
              }
              if constexpr (kRS) {   // the row's 64 columns sit in the four lanes l15 + 16 g
                {
                  const auto r1 = __builtin_amdgcn_permlane32_swap(__float_as_uint(s1), __float_as_uint(s1), false, false);
                  const auto r2 = __builtin_amdgcn_permlane32_swap(__float_as_uint(s2), __float_as_uint(s2), false, false);
                  s1 = __uint_as_float(r1[0]) + __uint_as_float(r1[1]);
                  s2 = __uint_as_float(r2[0]) + __uint_as_float(r2[1]);
                }
                {
                  const auto r1 = __builtin_amdgcn_permlane16_swap(__float_as_uint(s1), __float_as_uint(s1), false, false);
                  const auto r2 = __builtin_amdgcn_permlane16_swap(__float_as_uint(s2), __float_as_uint(s2), false, false);
                  s1 = __uint_as_float(r1[0]) + __uint_as_float(r1[1]);
                  s2 = __uint_as_float(r2[0]) + __uint_as_float(r2[1]);
                }
                if (g == 0) *reinterpret_cast<float2*>(rsb + (long)mi * 16 * a.rs_strips * 2) = make_float2(s1, s2);
              }
              EPI_STAMP(3 + mi)
            }
            if constexpr (kWatch) { if (cwm_ != 0ull && a.clamp_max != nullptr && lane == 0) atomicMax(reinterpret_cast<int*>(a.clamp_max), __float_as_int(kLimit)); }
          };
          // fp32-ONLY outputs: "rows" form.  Stored straight from the accumulator layout they leave as 16 rows x 64 B per instruction, twice the lines of 4 rows
          // x 256 B -- measured a wash against the staged epilogue on the bandwidth-bound read-modify-writes of the adapter tensor (MMSA_EPI_REGS_FP32).  Here each
          // 16-row sub-tile goes once through the wave's staging rows in LDS (4 ds_write_b128 in the accumulator layout, 4 ds_read_b128 as rows: a lane then holds
          // the SAME four columns of rows rl + 4 i) and leaves, like the residual rows arrive, as whole 256-byte row segments -- in straight-line code: the four
          // column parameters per lane, the rows' mean / rstd and the residual rows (one sub-tile ahead) are all requested before the first store.
          // c_RN: the row-normalising form on an fp32 output (the adapter tokens' LayerNorm folded into value / offset projections and fc1, AM:490-511,525-542).
          // 96-column tiles (a wave's strip is 48 columns; its fourth n-tile stays zero): the four lanes that would hold columns 48 .. 63 repeat columns 0 .. 15 --
          // the same loads, the same values stored to the same addresses -- so that the form needs no predicate.  c_CS: a per-column scale (ConvNeXt's gamma).
          auto epi_rows_ = [&](auto c_R, auto c_RN, auto c_CS) {
            constexpr bool kR = decltype(c_R)::value, kRN = decltype(c_RN)::value, kCS = decltype(c_CS)::value;
            float* stg_ = reinterpret_cast<float*>(EPI_STAGING_BASE) + wave * (16 * 68);
            const int l16_ = lane & 15;
            const int rl = lane >> 4, cl4 = (ni4 ? l16_ : (l16_ < 12 ? l16_ : l16_ - 12)) * 4;
            const int col = nb_ + cl4;
            const int rowb = m0 + wm * 64 + rl;            // + 16 mi + 4 i
            float4 bv4 = bias ? *reinterpret_cast<const float4*>(bias + col) : make_float4(0.f, 0.f, 0.f, 0.f);
            float4 sn4 = make_float4(0.f, 0.f, 0.f, 0.f), cv4 = make_float4(1.f, 1.f, 1.f, 1.f);
            if constexpr (kRN) sn4 = *reinterpret_cast<const float4*>(a.rn_cs + (long)bz * a.strideBias + col);
            if constexpr (kCS) {
              if (colscale) cv4 = *reinterpret_cast<const float4*>(colscale + col);
              cv4.x *= a.alpha; cv4.y *= a.alpha; cv4.z *= a.alpha; cv4.w *= a.alpha;
            }
            float2 mr4[4][4];
            if constexpr (kRN) {
#pragma unroll
              for (int mi = 0; mi < 4; ++mi)
#pragma unroll
                for (int i = 0; i < 4; ++i) mr4[mi][i] = *reinterpret_cast<const float2*>(a.rn_mr + 2 * ((long)bz * a.M + rowb + 16 * mi + 4 * i));
            }
            const float* rb_ = nullptr;
            float4 rq[2][4];
            if constexpr (kR) {
              rb_ = resid + (long)rowb * a.ldr + col;
#pragma unroll
              for (int i = 0; i < 4; ++i) rq[0][i] = *reinterpret_cast<const float4*>(rb_ + (long)(4 * i) * a.ldr);
            }
            EPI_STAMP(1) EPI_STAMP_WAIT() EPI_STAMP(2)
            float* cb_ = C + (long)rowb * a.ldc + col;
#pragma unroll
            for (int mi = 0; mi < 4; ++mi) {
              if constexpr (kR) {
                if (mi < 3) {
#pragma unroll
                  for (int i = 0; i < 4; ++i) rq[(mi + 1) & 1][i] = *reinterpret_cast<const float4*>(rb_ + (long)(16 * (mi + 1) + 4 * i) * a.ldr);
                }
              }
#pragma unroll
              for (int ni = 0; ni < 4; ++ni) {
                *reinterpret_cast<f32x4*>(stg_ + l15 * 68 + ni * 16 + 4 * g) = acc[ni][mi];
                acc[ni][mi] = (f32x4){0.f, 0.f, 0.f, 0.f};
              }
#pragma unroll
              for (int i = 0; i < 4; ++i) {
                const float4 t = *reinterpret_cast<const float4*>(stg_ + (rl + 4 * i) * 68 + cl4);
                float4 o;
                if constexpr (kRN) {
                  const float mu = mr4[mi][i].x, rs = mr4[mi][i].y;
                  o = make_float4(fmaf(rs, fmaf(-mu, sn4.x, t.x), bv4.x), fmaf(rs, fmaf(-mu, sn4.y, t.y), bv4.y), fmaf(rs, fmaf(-mu, sn4.z, t.z), bv4.z), fmaf(rs, fmaf(-mu, sn4.w, t.w), bv4.w));
                } else {
                  o = make_float4(t.x + bv4.x, t.y + bv4.y, t.z + bv4.z, t.w + bv4.w);
                }
                if constexpr (kCS) { o.x *= cv4.x; o.y *= cv4.y; o.z *= cv4.z; o.w *= cv4.w; }
                if constexpr (kR) { const float4 r_ = rq[mi & 1][i]; o.x += a.beta * r_.x; o.y += a.beta * r_.y; o.z += a.beta * r_.z; o.w += a.beta * r_.w; }
                EPI_ST16(cb_ + (long)(16 * mi + 4 * i) * a.ldc, o)
              }
              EPI_STAMP(3 + mi)
            }
          };
          const int cpf_ = Cp ? cp_base : -1;
          const bool rn_ = a.rn_mr != nullptr, rso_ = a.rs_out != nullptr;
          const bool scaled_ = colscale != nullptr || a.alpha != 1.0f;
#define EPI_REGS_RUN1(C_, R_, F_, S_, N_, CS_)                                                                                        \
  { epi_regs_(std::integral_constant<bool, C_>{}, std::integral_constant<bool, R_>{}, std::integral_constant<int, F_>{},               \
              std::integral_constant<bool, S_>{}, std::integral_constant<bool, N_>{}, std::integral_constant<bool, CS_>{}); regs_done = true; }
#define EPI_REGS_RUN(C_, R_, F_, S_, N_) { if (!scaled_) EPI_REGS_RUN1(C_, R_, F_, S_, N_, false) }   /* a scaled output of a variant without its scaled form: staged path */
          if (!C && !resid && !rso_) {   // planes-only outputs: lin1, qkv, the ConvNeXt / neck pw1s
            if (cpf_ == MMSA_FMT_H8C) { if (rn_) EPI_REGS_RUN(false, false, MMSA_FMT_H8C, false, true) else EPI_REGS_RUN(false, false, MMSA_FMT_H8C, false, false) }
            else if (cpf_ == MMSA_FMT_H8) { if (rn_) EPI_REGS_RUN(false, false, MMSA_FMT_H8, false, true) else EPI_REGS_RUN(false, false, MMSA_FMT_H8, false, false) }
            else if (cpf_ == MMSA_FMT_F3 && !rn_) EPI_REGS_RUN(false, false, MMSA_FMT_F3, false, false)
            else if (cpf_ == MMSA_FMT_B3 && !rn_) EPI_REGS_RUN(false, false, MMSA_FMT_B3, false, false)
          } else if (C && cpf_ < 0 && !rso_ && MMSA_EPI_ROWS) {
            if constexpr (ACT == ACT_NONE) {   // fp32-only outputs ("rows" form): extractor output projection, ConvFFN fc1 / fc2, value / offset projections, the neck's fc convs, ConvNeXt pw2
              if (scaled_) {
                if (!rn_) { if (resid) epi_rows_(std::true_type{}, std::false_type{}, std::true_type{}); else epi_rows_(std::false_type{}, std::false_type{}, std::true_type{}); regs_done = true; }
              } else if (resid) { if (!rn_) { epi_rows_(std::true_type{}, std::false_type{}, std::false_type{}); regs_done = true; } }
              else if (rn_) { epi_rows_(std::false_type{}, std::true_type{}, std::false_type{}); regs_done = true; }
              else { epi_rows_(std::false_type{}, std::false_type{}, std::false_type{}); regs_done = true; }
            }
          } else if (C && !rn_) {
            if constexpr (ACT == ACT_NONE) {   // fp32 outputs: the residual-stream producers (proj, lin2, out-proj), pw2, fc1 / fc2, value / offset projections
              if (resid && rso_ && cpf_ == MMSA_FMT_H8C) { if (scaled_) EPI_REGS_RUN1(true, true, MMSA_FMT_H8C, true, false, true) else EPI_REGS_RUN1(true, true, MMSA_FMT_H8C, true, false, false) }   // (scaled: the injector's gamma)
              else if (resid && rso_ && cpf_ == MMSA_FMT_F3) EPI_REGS_RUN(true, true, MMSA_FMT_F3, true, false)
              else if (MMSA_EPI_REGS_FP32 && resid && !rso_ && cpf_ < 0) EPI_REGS_RUN(true, true, -1, false, false)
              else if (MMSA_EPI_REGS_FP32 && !resid && !rso_ && cpf_ < 0) EPI_REGS_RUN(true, false, -1, false, false)
            }
          }
#undef EPI_REGS_RUN
#undef EPI_REGS_RUN1
#undef EPI_ST16
        }
      }
