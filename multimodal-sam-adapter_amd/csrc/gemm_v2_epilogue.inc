// Tile-boundary epilogue of the LDS-DMA GEMM kernels, included textually into the kernel body (gemm_v2.hip, gemm_h8c.hip).  Expects in scope:
// GemmV2Args a; template parameters GEN, ACT, PP (+ constexpr EPI_UNROLL, V2_BM, V2_NST); acc[4][4] (accumulators, zeroed on the way out);
// tile (output tile index), wave / lane / wm / wn, ni4 / swid, nowait; smem; and EPI_STAGING_BASE = byte address of >= 34816 B of
// LDS that no DMA in flight targets (8 waves x 16 rows x 68 floats), #defined by the kernel in front of the #include and #undef'd here.
    {
      // The epilogue sees the lane id through an opaque copy: everything it derives from it (row / column indices, 64-bit addresses) is
      // computed HERE, per tile.  Hoisted above the tile loop -- what LICM does with them otherwise -- those values are live across the k
      // loops, whose steady state needs 192 registers for accumulators, hi fragments and fp8 tuples alone: ~200 spilled registers in
      // gemm_h8c.hip, 143-184 scratch instructions in gemm_v2.hip's h8-line flavours (round 4 ISA), reloaded (scratch loads, one exposed
      // round trip per group) in every epilogue -- and a scratch reload in front of an LDS-DMA instruction is an s_waitcnt vmcnt(0), i.e.
      // a drain of the prefetch stream.
      int lane_o_ = lane;
      asm volatile("" : "+v"(lane_o_));
      const int lane = lane_o_, l15 = lane_o_ & 15, g = lane_o_ >> 4;
    // ---- tile boundary.  MFMA layout: lane holds C[m = ..+l15][n = ..+4g .. +3].  Each wave transposes 16 x 64
    // sub-tiles through the ring slot it has just finished computing from, so that residual loads and output stores
    // are FULL 256-byte row segments (4 rows per wave-instruction).  After the transpose a lane owns the SAME 4
    // columns in every row, so the column-wise part needs 8 registers.
    {
      const int per_b = a.nbm * a.nbn;
      const int bz = tile / per_b;
      const int rt = tile - bz * per_b;
      int tmi, tni;
      V2_TILE_MN(rt, tmi, tni);
      const int m0 = tmi * V2_BM, n0 = tni * a.bn;
      const float* bias = a.bias ? a.bias + (long)bz * a.strideBias : nullptr;
      const float* colscale = a.colscale ? a.colscale + (long)bz * a.strideBias : nullptr;   // per-column vectors share the batch stride
      const float* resid = a.resid ? a.resid + (long)bz * a.strideR : nullptr;
      float* C = a.C ? a.C + (long)bz * a.strideC : nullptr;
      unsigned short* Cp = a.Cp ? a.Cp + (long)bz * a.strideCp : nullptr;
      const bool vec_ok = ((a.ldc & 3) == 0) && (!resid || (a.ldr & 3) == 0) && ((a.N & 3) == 0) && ((a.ldcp & 3) == 0);
      if constexpr (PP) {
        nowait = 1;   // both groups drained before the last barrier of the k loop: k-tile j (and j+1) are visible
      } else {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // DMAs of j, j+1 (already issued) and every store issued so far
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();  // every wave has read its fragments of slot st_cur; the k-tiles already issued (two, or one with the 2-slot ring) landed for all
        nowait = V2_NST - 1;
      }
      float* stg = reinterpret_cast<float*>(EPI_STAGING_BASE) + wave * (16 * 68);
      const int nb_ = n0 + wn * swid;
      const int cp_base = MMSA_CP_BASE(a.cp_fmt);
      const bool cp_split = MMSA_CP_SPLIT(a.cp_fmt) != 0;   // kernel-uniform: columns >= the split leave as h8 planes (common.h)
      // planes output, all three formats.  A 64-column strip of a row is staged as an LDS row image and read back 16 bytes per lane so
      // that it leaves in whole 16-byte pieces: bf16 hi/lo and h8 line planes = 256 B (two 128-byte lines: lanes 0..15); h8c planes = the
      // row's 128-byte hi line of that chunk (lanes 0..7) + its 64 lo bytes (lanes 8..11; lanes 12..15 store nothing).
      const bool cp_h8c = cp_base == MMSA_FMT_H8C;
      const int cp_kpad = MMSA_PAD64((GEN && a.out_mode == 1) ? a.ps_C : a.N);   // h8c: fp16 values per row of the output planes
#include "gemm_epilogue_regs.inc"
      if (!regs_done) {   // ---- the LDS-staged epilogue: ragged tiles, 96-column tiles, pixel-shuffle stores, split plane formats, other activations
      // clamp watch of this path (common.h): checked per stored group, nothing carried (a running maximum kept across this path's unrolled sub-tiles cost the
      // kernel ~200 bytes of scratch and the extractor output projection 35 %: profiles/r05_clamp_watch.txt); a split output (f3 | h8 columns) is held to
      // the h8 limit throughout
      const float cw_lim_ = cp_split ? MMSA_H8_MAX : mmsa_clamp_limit(cp_base);
      auto cp_stage4 = [&](unsigned short* srow_, int c_, const float4 o_, int col_) {
#if MMSA_CW_LEG
        { float m_ = 0.f; clamp_see(m_, o_); clamp_report(a.clamp_max, m_, cw_lim_); }
#endif
        if (cp_h8c) {
          uint2 hi_; unsigned lo8_, qh8_;
          h8_split4<true>(o_, hi_, lo8_, qh8_);   // h8c: lo scaled for the truncated q(hi) (common.h MMSA_H8C_LO_COMP)
          *reinterpret_cast<uint2*>(srow_ + c_) = hi_;
          *reinterpret_cast<unsigned*>(reinterpret_cast<unsigned char*>(srow_) + 128 + h8c_lo_off(c_)) = lo8_;
        } else {
          store_planes4(srow_, c_, o_, cp_split ? MMSA_CP_AT(a.cp_fmt, col_) : cp_base);
        }
      };
      auto cp_store16 = [&](long drow__, int dcol__, const uint4 pk_) {   // dcol__: any column of the strip (its 64-column chunk is what counts)
        if (cp_h8c) {
          const H8cRow r_ = h8c_row(Cp, a.ldcp, drow__, cp_kpad);
          const int l_ = lane & 15, ch_ = (dcol__ >> 6) << 7;
          if (l_ < 8) *reinterpret_cast<uint4*>(reinterpret_cast<unsigned char*>(r_.hi) + ch_ + 16 * l_) = pk_;
          else if (l_ < 12) *reinterpret_cast<uint4*>(r_.lo + ch_ + 16 * (l_ - 8)) = pk_;
        } else {
          *reinterpret_cast<uint4*>(Cp + drow__ * a.ldcp + ilv(dcol__ & ~63) + 8 * (lane & 15)) = pk_;
        }
      };
      auto cp_store1 = [&](long drow__, int dcol__, float x_) {
#if MMSA_CW_LEG
        clamp_report(a.clamp_max, fabsf(x_), cw_lim_);
#endif
        if (cp_h8c) h8c_store1(h8c_row(Cp, a.ldcp, drow__, cp_kpad), dcol__, x_);
        else store_planes1(Cp + drow__ * a.ldcp, dcol__, x_, MMSA_CP_AT(a.cp_fmt, dcol__));
      };
      const int rl0 = lane >> 4;            // read-back: lane -> (row = rl0 + 4*i, columns cl .. cl+3)
      const int cl = (lane & 15) * 4;
      const bool lane_ok = cl < swid;        // 96-column tiles: the lanes of the (skipped) fourth n-tile only keep the loads in bounds
      const int n = nb_ + (lane_ok ? cl : 0);
      // column parameters of this lane's 4 columns: loaded ONCE per tile, unconditionally (clamped index)
      float bv[4], cv[4];
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        int ci = min(n + r, a.N - 1);
        bv[r] = bias ? bias[ci] : 0.f;
        if constexpr (GEN) { if (a.out_mode == 1) ci %= a.ps_C; }
        cv[r] = colscale ? colscale[ci] * a.alpha : a.alpha;
      }
      // row mapping (destination row / column, residual row); identity unless GEN
      // pixel-shuffle store: the (i, j) quadrant of this lane's own columns is fixed for the tile -- one division per tile, not per row
      int ij_n = 0, dcol_n = n;
      if constexpr (GEN) { if (a.out_mode == 1) { ij_n = n / a.ps_C; dcol_n = n - ij_n * a.ps_C; } }
      auto map_row = [&](int m, int nn, long& drow_, int& dcol, long& rrow) {
        drow_ = m; dcol = nn; rrow = m;
        if constexpr (GEN) {
          if (a.out_mode == 1) {
            int ij = ij_n;
            dcol = dcol_n;
            if (nn != n) { ij = nn / a.ps_C; dcol = nn - ij * a.ps_C; }
            int w_, h_, b_;
            if (a.ps_sw >= 0 && a.ps_sh >= 0) {   // power-of-two grids (every shipped config): shifts and masks
              w_ = m & (a.ps_W - 1);
              const int t_ = m >> a.ps_sw;
              h_ = t_ & (a.ps_H - 1);
              b_ = t_ >> a.ps_sh;
            } else {
              w_ = m % a.ps_W;
              const int t_ = m / a.ps_W;
              h_ = t_ % a.ps_H;
              b_ = t_ / a.ps_H;
            }
            drow_ = ((long)(b_ * 2 * a.ps_H + 2 * h_ + (ij >> 1))) * (2 * a.ps_W) + 2 * w_ + (ij & 1);
          }
          rrow = a.resid_mod > 0 ? (long)((int)drow_ % a.resid_mod) : drow_;
        }
      };
      // wave-uniform: whole 64-column strip inside N, 16-byte aligned (and, for the planes output of a pixel-shuffle
      // store, inside one destination row: ps_C a multiple of 64)
      const bool fast = vec_ok && (nb_ + swid <= a.N) && (ni4 || !Cp) && (!GEN || !Cp || a.out_mode != 1 || (a.ps_C & 63) == 0);
      // The four 16-row sub-tiles are handled by a ROLLED loop: the code always takes accumulator column 0 and then
      // rotates the columns down by register moves (48 v_mov per pass).  Fully unrolled -- with the activation switch
      // expanded per element -- the epilogue was ~100 KiB of straight-line code, far beyond the 64 KiB instruction
      // cache two CUs share, and ran at instruction-fetch speed: ~45 of the kernel's ~200 us at K = 1024 with
      // only ~13 us of that being the stores themselves (MMSA_GEMM_DEBUG 1 / 10 / 2 ablations).
      const int act = ACT >= 0 ? ACT : a.act;
      // Planes-only outputs (lin1, qkv, the ConvNeXt pw1s: no fp32 copy, no residual, plain row mapping): bias / activation / scale are
      // applied in the NATIVE accumulator layout (lane = row l15, columns 16 ni + 4g .. +3) and the split values go straight into the
      // LDS line image, which is read back 16 bytes per lane for whole-line stores: ONE LDS round trip per sub-tile instead of two
      // (transpose to rows, then re-stage as lines), and the four sub-tiles' LDS traffic and arithmetic are free to overlap -- a wave's
      // LDS instructions execute in order, so sub-tile mi + 1 may overwrite the staging rows as soon as mi's read-backs are ISSUED.
      bool direct = false;
      if constexpr (EPI_UNROLL && !GEN) direct = fast && Cp && !C && !resid && ni4 && V2_DBG(a) == 0 && (((uintptr_t)bias | (uintptr_t)colscale) & 15) == 0;
      if constexpr (EPI_UNROLL && !GEN) {
        if (direct) {
          float4 bn_[4], cn_[4], sn_[4];
          const bool rn = a.rn_mr != nullptr;       // kernel-uniform: row-normalising epilogue (LayerNorm folded in)
#pragma unroll
          for (int ni = 0; ni < 4; ++ni) {
            const int ci = nb_ + ni * 16 + 4 * g;     // fast: the whole 64-column strip is inside N
            bn_[ni] = bias ? *reinterpret_cast<const float4*>(bias + ci) : make_float4(0.f, 0.f, 0.f, 0.f);
            cn_[ni] = colscale ? *reinterpret_cast<const float4*>(colscale + ci) : make_float4(1.f, 1.f, 1.f, 1.f);
            cn_[ni].x *= a.alpha; cn_[ni].y *= a.alpha; cn_[ni].z *= a.alpha; cn_[ni].w *= a.alpha;
            sn_[ni] = rn ? *reinterpret_cast<const float4*>(a.rn_cs + (long)bz * a.strideBias + ci) : make_float4(0.f, 0.f, 0.f, 0.f);
          }
          unsigned short* wrow = reinterpret_cast<unsigned short*>(stg + l15 * 68);
#pragma unroll
          for (int mi = 0; mi < 4; ++mi) {
            const int mb = m0 + wm * 64 + mi * 16;
            float mu = 0.f, rs = 1.f;                 // this lane's row of the sub-tile (rows beyond M: clamped, never stored)
            if (rn) {
              const float2 mr = *reinterpret_cast<const float2*>(a.rn_mr + 2 * ((long)bz * a.M + min(mb + l15, a.M - 1)));
              mu = mr.x; rs = mr.y;
            }
#pragma unroll
            for (int ni = 0; ni < 4; ++ni) {
              float4 o;
              if (rn) {   // rstd * (acc - mean * colsum) + bias: the two roundings of the reference's (x - mean) * rstd are not reproduced, the value is
                o = make_float4(fmaf(rs, fmaf(-mu, sn_[ni].x, acc[ni][mi][0]), bn_[ni].x), fmaf(rs, fmaf(-mu, sn_[ni].y, acc[ni][mi][1]), bn_[ni].y),
                                fmaf(rs, fmaf(-mu, sn_[ni].z, acc[ni][mi][2]), bn_[ni].z), fmaf(rs, fmaf(-mu, sn_[ni].w, acc[ni][mi][3]), bn_[ni].w));
              } else {
                o = make_float4(acc[ni][mi][0] + bn_[ni].x, acc[ni][mi][1] + bn_[ni].y, acc[ni][mi][2] + bn_[ni].z, acc[ni][mi][3] + bn_[ni].w);
              }
              acc[ni][mi] = (f32x4){0.f, 0.f, 0.f, 0.f};
              if (act != ACT_NONE) {
                if (act == ACT_GELU) o = gelu4(o);
                else { o.x = apply_act(o.x, act); o.y = apply_act(o.y, act); o.z = apply_act(o.z, act); o.w = apply_act(o.w, act); }
              }
              o.x *= cn_[ni].x; o.y *= cn_[ni].y; o.z *= cn_[ni].z; o.w *= cn_[ni].w;
              cp_stage4(wrow, ni * 16 + 4 * g, o, nb_ + ni * 16 + 4 * g);
            }
            uint4 pk[4];
#pragma unroll
            for (int i = 0; i < 4; ++i)
              pk[i] = *reinterpret_cast<const uint4*>(reinterpret_cast<const unsigned short*>(stg + (rl0 + 4 * i) * 68) + 8 * (lane & 15));
#pragma unroll
            for (int i = 0; i < 4; ++i) {
              const int m = mb + rl0 + 4 * i;
              if (m < a.M) cp_store16(m, n, pk[i]);
            }
          }
        }
      }
      // (fp32-only outputs stored straight from the accumulator layout -- 16 rows x 64 bytes per instruction, no LDS transpose --
      // measured time-neutral against the transposed whole-row stores on every shape and on the step, same box: not kept.)
      if (direct) {
      } else if constexpr (EPI_UNROLL) {
        // residual rows one sub-tile AHEAD: the 4 loads of sub-tile mi + 1 are issued before sub-tile mi is processed (its LDS round
        // trips, arithmetic and stores cover their latency).  Requested per sub-tile -- behind the previous sub-tile's stores, which the
        // compiler must assume alias them when the GEMM updates its residual in place -- a tile's epilogue was four serialised memory
        // round trips: 33 us of a 127 us launch at one tile per workgroup (lin2 of one image, profiles/r03_v3_vs_v2.txt).  (All four
        // sub-tiles up front would need 64 registers and spills.)
        float4 rrn[4];
        auto load_rr = [&](int mi_) {
#pragma unroll
          for (int i = 0; i < 4; ++i) {
            long drow_, rrow; int dcol;
            map_row(min(m0 + wm * 64 + mi_ * 16 + rl0 + 4 * i, a.M - 1), n, drow_, dcol, rrow);
            rrn[i] = *reinterpret_cast<const float4*>(resid + rrow * a.ldr + dcol);
          }
        };
        if (fast && resid) load_rr(0);
#pragma unroll
        for (int mi = 0; mi < 4; ++mi) {
        const int mb = m0 + wm * 64 + mi * 16;
        float4 rr[4];
        if (fast && resid) {
#pragma unroll
          for (int i = 0; i < 4; ++i) rr[i] = rrn[i];
          if (mi < 3) load_rr(mi + 1);
        }
#pragma unroll
        for (int ni = 0; ni < 4; ++ni) {
          *reinterpret_cast<f32x4*>(stg + l15 * 68 + ni * 16 + 4 * g) = acc[ni][mi];
          acc[ni][mi] = (f32x4){0.f, 0.f, 0.f, 0.f};
        }
        if (V2_DBG(a) == 1) continue;
        if (fast) {
#pragma unroll
          for (int i = 0; i < 4; ++i) {
            const int rl = rl0 + 4 * i;
            float4 o = *reinterpret_cast<const float4*>(stg + rl * 68 + cl);
            o.x += bv[0]; o.y += bv[1]; o.z += bv[2]; o.w += bv[3];
            if (act != ACT_NONE) {   // ONE wave-uniform branch per 4 values (none when ACT is a template constant)
              if (act == ACT_GELU) o = gelu4(o);
              else { o.x = apply_act(o.x, act); o.y = apply_act(o.y, act); o.z = apply_act(o.z, act); o.w = apply_act(o.w, act); }
            }
            o.x *= cv[0]; o.y *= cv[1]; o.z *= cv[2]; o.w *= cv[3];
            if (resid) { o.x += a.beta * rr[i].x; o.y += a.beta * rr[i].y; o.z += a.beta * rr[i].z; o.w += a.beta * rr[i].w; }
            // planes output: split in registers, re-stage the bf16 pairs in the INTERLEAVED layout (hi 32 | lo 32 per
            // k-block) in the same LDS row and read them back 16 bytes per lane, so that a row-group leaves as ONE
            // instruction of 4 x 256 contiguous bytes = full 128-byte lines (8-byte hi / lo stores wrote every line as
            // two half-lines from two instructions).  LDS executes a wave's instructions in order: the row was fully
            // read (above) before it is overwritten here.
            uint4 pk = make_uint4(0u, 0u, 0u, 0u);
            if (Cp) {   // either planes format: stage the row image, read it back 16 bytes per lane
              unsigned short* srow = reinterpret_cast<unsigned short*>(stg + rl * 68);
              cp_stage4(srow, cl, o, nb_ + cl);
              pk = *reinterpret_cast<const uint4*>(srow + 8 * (lane & 15));
            }
            const int m = mb + rl;
            if (a.rs_out) {   // kernel-uniform: sum and sum of squares of this row's 64 columns (the 16 lanes of one DPP row hold them)
              float s1 = (o.x + o.y) + (o.z + o.w), s2 = fmaf(o.x, o.x, o.y * o.y) + fmaf(o.z, o.z, o.w * o.w);
#pragma unroll
              for (int sh = 8; sh > 0; sh >>= 1) { s1 += __shfl_xor(s1, sh, 64); s2 += __shfl_xor(s2, sh, 64); }
              if ((lane & 15) == 0 && m < a.M)
                *reinterpret_cast<float2*>(a.rs_out + (((long)bz * a.M + m) * a.rs_strips + (nb_ >> 6)) * 2) = make_float2(s1, s2);
            }
            if (V2_DBG(a) == 10) { asm volatile("" :: "v"(o.x), "v"(o.y), "v"(o.z), "v"(o.w), "v"(pk.x), "v"(pk.w)); }   // timing: everything but the stores
            else if (m < a.M && lane_ok) {
              long drow_, rrow; int dcol;
              map_row(m, n, drow_, dcol, rrow);
              if (C) *reinterpret_cast<float4*>(C + drow_ * a.ldc + dcol) = o;
              if (Cp) cp_store16(drow_, dcol, pk);
            }
          }
        } else {  // ragged right edge or unaligned leading dimensions: element-wise, rare
#pragma unroll 1
          for (int e = 0; e < 16; ++e) {
            const int i = e >> 2, r = e & 3;
            const int rl = rl0 + 4 * i;
            const int m = mb + rl;
            if (m >= a.M || n + r >= a.N || !lane_ok) continue;
            float x = stg[rl * 68 + cl + r];
            {
              int ci = n + r;
              const float b_ = bias ? bias[ci] : 0.f;
              if constexpr (GEN) { if (a.out_mode == 1) ci %= a.ps_C; }
              x = apply_act(x + b_, act) * (colscale ? colscale[ci] * a.alpha : a.alpha);
            }
            long drow_, rrow; int dcol;
            map_row(m, n + r, drow_, dcol, rrow);
            if (resid) x += a.beta * resid[rrow * a.ldr + dcol];
            if (C) C[drow_ * a.ldc + dcol] = x;
            if (Cp) cp_store1(drow_, dcol, x);
          }
        }
        }
      } else {
#pragma unroll 1
        for (int mi = 0; mi < 4; ++mi) {
        const int mb = m0 + wm * 64 + mi * 16;
        // residual rows first: 4 independent 16-byte loads in flight, no waits inside the element loops
        float4 rr[4];
        if (fast && resid) {
#pragma unroll
          for (int i = 0; i < 4; ++i) {
            long drow_, rrow; int dcol;
            map_row(min(mb + rl0 + 4 * i, a.M - 1), n, drow_, dcol, rrow);
            rr[i] = *reinterpret_cast<const float4*>(resid + rrow * a.ldr + dcol);
          }
        }
#pragma unroll
        for (int ni = 0; ni < 4; ++ni) {
          *reinterpret_cast<f32x4*>(stg + l15 * 68 + ni * 16 + 4 * g) = acc[ni][0];
          acc[ni][0] = acc[ni][1];
          acc[ni][1] = acc[ni][2];
          acc[ni][2] = acc[ni][3];
          acc[ni][3] = (f32x4){0.f, 0.f, 0.f, 0.f};
        }
        if (V2_DBG(a) == 1) continue;
        if (fast) {
#pragma unroll
          for (int i = 0; i < 4; ++i) {
            const int rl = rl0 + 4 * i;
            float4 o = *reinterpret_cast<const float4*>(stg + rl * 68 + cl);
            o.x += bv[0]; o.y += bv[1]; o.z += bv[2]; o.w += bv[3];
            if (act != ACT_NONE) {   // ONE wave-uniform branch per 4 values (none when ACT is a template constant)
              if (act == ACT_GELU) o = gelu4(o);
              else { o.x = apply_act(o.x, act); o.y = apply_act(o.y, act); o.z = apply_act(o.z, act); o.w = apply_act(o.w, act); }
            }
            o.x *= cv[0]; o.y *= cv[1]; o.z *= cv[2]; o.w *= cv[3];
            if (resid) { o.x += a.beta * rr[i].x; o.y += a.beta * rr[i].y; o.z += a.beta * rr[i].z; o.w += a.beta * rr[i].w; }
            // planes output: split in registers, re-stage the bf16 pairs in the INTERLEAVED layout (hi 32 | lo 32 per
            // k-block) in the same LDS row and read them back 16 bytes per lane, so that a row-group leaves as ONE
            // instruction of 4 x 256 contiguous bytes = full 128-byte lines (8-byte hi / lo stores wrote every line as
            // two half-lines from two instructions).  LDS executes a wave's instructions in order: the row was fully
            // read (above) before it is overwritten here.
            uint4 pk = make_uint4(0u, 0u, 0u, 0u);
            if (Cp) {   // either planes format: stage the row image, read it back 16 bytes per lane
              unsigned short* srow = reinterpret_cast<unsigned short*>(stg + rl * 68);
              cp_stage4(srow, cl, o, nb_ + cl);
              pk = *reinterpret_cast<const uint4*>(srow + 8 * (lane & 15));
            }
            const int m = mb + rl;
            if (V2_DBG(a) == 10) { asm volatile("" :: "v"(o.x), "v"(o.y), "v"(o.z), "v"(o.w), "v"(pk.x), "v"(pk.w)); }   // timing: everything but the stores
            else if (m < a.M && lane_ok) {
              long drow_, rrow; int dcol;
              map_row(m, n, drow_, dcol, rrow);
              if (C) *reinterpret_cast<float4*>(C + drow_ * a.ldc + dcol) = o;
              if (Cp) cp_store16(drow_, dcol, pk);
            }
          }
        } else {  // ragged right edge or unaligned leading dimensions: element-wise, rare
#pragma unroll 1
          for (int e = 0; e < 16; ++e) {
            const int i = e >> 2, r = e & 3;
            const int rl = rl0 + 4 * i;
            const int m = mb + rl;
            if (m >= a.M || n + r >= a.N || !lane_ok) continue;
            float x = stg[rl * 68 + cl + r];
            {
              int ci = n + r;
              const float b_ = bias ? bias[ci] : 0.f;
              if constexpr (GEN) { if (a.out_mode == 1) ci %= a.ps_C; }
              x = apply_act(x + b_, act) * (colscale ? colscale[ci] * a.alpha : a.alpha);
            }
            long drow_, rrow; int dcol;
            map_row(m, n + r, drow_, dcol, rrow);
            if (resid) x += a.beta * resid[rrow * a.ldr + dcol];
            if (C) C[drow_ * a.ldc + dcol] = x;
            if (Cp) cp_store1(drow_, dcol, x);
          }
        }
        }
      }
      }
    }
    }
#undef EPI_STAGING_BASE
#ifdef EPI_STAMP_DEFAULTED_
#undef EPI_STAMP_DEFAULTED_
#undef EPI_STAMP
#undef EPI_STAMP_WAIT
#endif
