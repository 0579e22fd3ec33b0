// Flash-attention BACKWARD v2 — CDNA4 MFMA 32x32x16, causal, GQA, D=128.
//
// The tuned backward: the patterns proven out in attention_fwd.hip, through
// the same fa32_common.h helpers
// (ff_stage swizzled staging, ff_relayout permlane relayout, ff_tr_read8
// 4x4-group ds_read_b64_tr_b16 transpose reads — all probe-verified on
// hardware, tools/tr_probe_check.py).  ff_tr_read8 reads only the low 4 bits
// of its l15 argument; these kernels hand it tid.
//
//   fa2_dq : grid over q-tiles (fwd-shaped; wave owns 32 q rows).
//            Per 64-kv tile:
//              ST' = mfma(A=K_lds, B=Q_regs)          -> D[kv][q], col=q
//              dP' = mfma(A=V_lds, B=dO_lds B-frags)  -> D[kv][q]
//              P'  = exp2(st*scale*log2e - lse2[q])   (lse known: no online
//                    max bookkeeping; masked entries -> exp2(-inf) = 0)
//              dS' = P' * (dP' - delta[q])            (lane-local, col=q)
//              dQacc[d][q] += mfma(A=K^T tr-frags, B=relayout(dS'))
//            Epilogue dQ[q][d] = scale * acc — the fwd's O-epilogue shape.
//   fa2_dv : grid over kv-tiles (wave owns 32 kv rows). Per 64-q tile
//            (diagonal..S):
//              ST = mfma(A=Q_lds, B=K_regs)           -> D[q][kv], col=kv
//              P  = exp2(st*scale2 - lse2[row q])     (LDS broadcast reads)
//              dVacc[d][kv] += mfma(A=dO^T tr-frags, B=relayout(P))
//   fa2_dk : the same body (template <bool DK>); adds
//              dP = mfma(A=dO_lds, B=V_regs)          -> D[q][kv]
//              dS = P * (dP - delta[row q])
//              dKacc[d][kv] += mfma(A=Q^T tr-frags, B=relayout(dS))
//            Epilogue dK[kv][d] = scale * acc.
//
// fa_bwd_preprocess provides delta = rowsum(dO*O); dV/dK write per-Hq
// partials and fa_bwd_reduce_gqa sums the GQA groups.
//
// Reference parity: the reference framework uses the stock flash kernels;
// this replaces the train step's heaviest kernel (the library backward is
// 30% of the Llama-8B step — profiles/bench_kernel_stats_r1_final.txt).
#include "fa32_common.h"

#define FB_D FF_D
#define FB_OWN 32             // rows owned per wave (q for dq; kv for dv/dk)
#define FB_WAVES 8
#define FB_TILE (FB_OWN * FB_WAVES)  // 256 own-rows per block
#define FB_OTH 64             // other-side tile (kv for dq; q for dv/dk)
#define FB_THREADS (FB_WAVES * 64)

// ---------------------------------------------------------------------------
// delta = rowsum(dO * O)   [B*H*S rows of D elems]
// ---------------------------------------------------------------------------
extern "C" __global__ void __launch_bounds__(256)
fa_bwd_preprocess(const unsigned short* __restrict__ dout,
                  const unsigned short* __restrict__ o,
                  float* __restrict__ delta, int64_t rows, int Hq, int S, int bshd) {
  // 16 lanes per row (8 elems each), 16 rows per 256-thread block per
  // iteration; fully coalesced loads, shfl-xor reduce inside each 16-lane
  // group, no barriers — HBM-roofline for this pure-bandwidth pass.
  const int sub = threadIdx.x & 15;         // lane within row
  int64_t row = (int64_t)blockIdx.x * 16 + (threadIdx.x >> 4);
  const int64_t stride = (int64_t)gridDim.x * 16;
  for (; row < rows; row += stride) {
    const unsigned short* pd = dout + row * FB_D + sub * 8;
    const unsigned short* po = o + row * FB_D + sub * 8;
    ff_shortx8 a = *reinterpret_cast<const ff_shortx8*>(pd);
    ff_shortx8 b = *reinterpret_cast<const ff_shortx8*>(po);
    float s = 0.f;
#pragma unroll
    for (int j = 0; j < 8; ++j)
      s += bf16_to_f32((unsigned short)a[j]) * bf16_to_f32((unsigned short)b[j]);
#pragma unroll
    for (int off = 8; off >= 1; off >>= 1)
      s += __shfl_xor(s, off, 64);
    // delta is [B,Hq,S] in both layouts.  bshd: dout and o are [B,S,Hq,D] and
    // `row` walks them in memory order, row = (b*S + s)*Hq + h (rows fits 31
    // bits there, the binding checks), so only the 4-byte store is scattered.
    int64_t drow = row;
    if (bshd) {
      const unsigned r = (unsigned)row, bs = r / (unsigned)Hq, h = r - bs * (unsigned)Hq;
      const unsigned bi = bs / (unsigned)S, sq = bs - bi * (unsigned)S;
      drow = ((int64_t)bi * Hq + h) * S + sq;
    }
    if (sub == 0) delta[drow] = s;
  }
}

// ---------------------------------------------------------------------------
// reduce GQA partials: dk[b,hkv,s,d] = sum over group of dk_part[b,h,s,d]
// ---------------------------------------------------------------------------
extern "C" __global__ void __launch_bounds__(256)
fa_bwd_reduce_gqa(const unsigned short* __restrict__ part,  // [B,Hq,S,D]
                  unsigned short* __restrict__ out,         // [B,Hkv,S,D]
                  int B, int Hq, int Hkv, int64_t SD) {
  int group = Hq / Hkv;
  int64_t total = (int64_t)B * Hkv * SD;
  int64_t i0 = (int64_t)(blockIdx.x * 256 + threadIdx.x) * 8;
  int64_t stride = (int64_t)gridDim.x * 256 * 8;
  for (int64_t i = i0; i < total; i += stride) {
    int64_t bh = i / SD;
    int64_t off = i % SD;
    int64_t b = bh / Hkv;
    int64_t hk = bh % Hkv;
    float acc[8] = {0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll 4
    for (int g = 0; g < group; ++g) {
      const unsigned short* p =
          part + ((b * Hq + hk * group + g) * SD) + off;
      ff_shortx8 v = *reinterpret_cast<const ff_shortx8*>(p);
#pragma unroll
      for (int j = 0; j < 8; ++j) acc[j] += bf16_to_f32((unsigned short)v[j]);
    }
    ff_shortx8 o;
#pragma unroll
    for (int j = 0; j < 8; ++j) o[j] = (short)f32_to_bf16(acc[j]);
    *reinterpret_cast<ff_shortx8*>(out + i) = o;
  }
}

// ---------------------------------------------------------------------------
// fa2_dq: dQ = scale * K^T-contract(dS'); grid (S/256, Hq, B)
// ---------------------------------------------------------------------------
extern "C" __global__ void __launch_bounds__(FB_THREADS, 2)
fa2_dq_bf16(const unsigned short* __restrict__ q,
            const unsigned short* __restrict__ k,
            const unsigned short* __restrict__ v,
            const unsigned short* __restrict__ dout,
            const float* __restrict__ lse,
            const float* __restrict__ delta,
            unsigned short* __restrict__ dq,
            int B, int Hq, int Hkv, int S, float scale, int bshd) {
  __shared__ unsigned short lk[FB_OTH * FB_D];    // K kv-tile (swz)
  __shared__ unsigned short lv[FB_OTH * FB_D];    // V kv-tile (swz)
  __shared__ unsigned short ldo[FB_TILE * FB_D];  // block's dO q rows (swz)

  const ff_ctx c = ff_prologue(Hq, Hkv, S);
  const int tid = c.tid, l31 = c.l31, half = c.half;
  // The wave index in a scalar register: `active` and `need_mask` below are
  // then scalar compares and branches, and the epilogue rebuilds its row from
  // it (see there).
  const int wave = __builtin_amdgcn_readfirstlane(c.wave);
  // Tile t costs t + 1 units of work and the hardware dispatches blocks in
  // grid order: walk a head's tiles from the last (heaviest) one down, so the
  // blocks that start last are the cheap ones and the kernel's tail is short
  // (4.66 -> 4.50 ms per call at the bench shape).  Blocks do not
  // communicate: results are bitwise those of the ascending order.
  const int qt = (int)gridDim.x - 1 - c.tile;
  const int64_t qbase = c.qbase, kbase = c.kbase;
  const int q0 = qt * FB_TILE + wave * FB_OWN;
  const int my_q = q0 + l31;
  const float scale2 = scale * FF_LOG2E;

  // lane-local per-q constants (col = q = l31)
  const int64_t lrow = c.rbase + my_q;
  const float lse2 = lse[lrow] * FF_LOG2E;
  const float dlt = delta[lrow];

  // Q fragments (B-operand, like the fwd's qf)
  ff_shortx8 qf[8];
  ff_row_frags(q + qbase + (int64_t)my_q * FB_D, qf, half);
  // stage the block's FB_TILE dO rows once (swizzled)
  // (dout is [B,Hq,S,D] or, bshd, [B,S,Hq,D]: a row stride and a head base)
  const ff_rows dorow = ff_o_rows(c, Hq, S, bshd);
  ff_stage_rows<FB_TILE, FB_THREADS>(
      dout + dorow.base + (int64_t)qt * FB_TILE * dorow.stride, dorow.stride, ldo, tid);

  ff_floatx16 dqacc[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) dqacc[i] = (ff_floatx16)(0.f);

  const int last_kv = min((qt + 1) * (FB_TILE / FB_OTH), S / FB_OTH);
  const unsigned short* kg = k + kbase;
  const unsigned short* vg = v + kbase;

  for (int jkv = 0; jkv < last_kv; ++jkv) {
    const int kv0 = jkv * FB_OTH;
    const bool active = (kv0 <= q0 + FB_OWN - 1);
    const bool need_mask = (kv0 + FB_OTH - 1 > q0);
    __syncthreads();  // previous tile's readers done
    ff_stage<FB_OTH, FB_THREADS>(kg + (int64_t)kv0 * FB_D, lk, tid);
    ff_stage<FB_OTH, FB_THREADS>(vg + (int64_t)kv0 * FB_D, lv, tid);
    __syncthreads();

    if (active) {
      // ST' = K.Q^T and dP' = V.dO^T — both D[kv][q], col = q = l31
      ff_floatx16 st[2], dp[2];
#pragma unroll
      for (int s2 = 0; s2 < 2; ++s2) {
        st[s2] = (ff_floatx16)(0.f);
        dp[s2] = (ff_floatx16)(0.f);
      }
#pragma unroll
      for (int s2 = 0; s2 < 2; ++s2)
#pragma unroll
        for (int ks = 0; ks < 8; ++ks) {
          ff_shortx8 kfr = ff_afrag(lk, s2, ks, l31, half);
          st[s2] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(kfr, qf[ks], st[s2], 0, 0, 0);
          ff_shortx8 vfr = ff_afrag(lv, s2, ks, l31, half);
          ff_shortx8 dof = ff_bfrag(ldo, wave * FB_OWN + l31, ks, half);
          dp[s2] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(vfr, dof, dp[s2], 0, 0, 0);
        }
      // mask kv > q: only a diagonal tile (wave-uniform need_mask, 4 of a
      // block's tiles) pays for it
      if (need_mask) ff_mask<true>(st, my_q - kv0 - 4 * half);
      // dS' = P' * (dP' - delta); P' = exp2(st*scale2 - lse2)
#pragma unroll
      for (int s2 = 0; s2 < 2; ++s2)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          float p = __builtin_amdgcn_exp2f(st[s2][r] * scale2 - lse2);
          st[s2][r] = p * (dp[s2][r] - dlt);
        }
      ff_shortx8 pb[4];
      ff_relayout(st, pb);  // B-frags [q][kv-contraction]
      // dQacc[d][q] += K^T . dS' (fwd's PV shape: A via tr, B = relayout)
#pragma unroll
      for (int ds = 0; ds < 4; ++ds) {
        ff_shortx4 t[4][2];
        ff_tr_read8(lk, ds, tid, l31, half, t);
#pragma unroll
        for (int ks = 0; ks < 4; ++ks)
          dqacc[ds] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(
              ff_cat(t[ks][0], t[ks][1]), pb[ks], dqacc[ds], 0, 0, 0);
      }
    }
  }

  // epilogue: dQ[q][d] = scale * acc (D-layout: rows = d, col = q = l31).
  // The row address and `half` are worked out again here, from the scalar
  // wave index and a lane id read afresh (volatile, so it stays below the
  // loop): otherwise the compiler keeps them in three VGPRs across the tile
  // loop, which has none to spare, and spills them to scratch (16 B/lane).
  // This steers the register allocator of one compiler: tests/
  // test_fa32_resources.py (scratch 0, <= 256 VGPRs) is what says when it no
  // longer suffices, and building without it under that test, when it is no
  // longer needed.
  int elane;
  asm volatile("v_mbcnt_lo_u32_b32 %0, -1, 0\n\tv_mbcnt_hi_u32_b32 %0, -1, %0" : "=v"(elane));
  const int e_q = qt * FB_TILE + wave * FB_OWN + (elane & 31);
  ff_store_row(dq + qbase + (int64_t)e_q * FB_D, dqacc, scale, elane >> 5);
}

// ---------------------------------------------------------------------------
// fa2_dv / fa2_dk: one body, two instantiations; grid (S/256 kv-tiles, Hq, B),
// per-Hq partials.
//   DK=false: dV[kv][d] = sum_q P dO          (v and delta unused: no V
//             fragments, no dP MFMAs, no delta row in LDS)
//   DK=true : dK[kv][d] = scale * sum_q dS Q, dS = P * (dP - delta)
// ---------------------------------------------------------------------------
template <bool DK>
DEV void fa2_dv_dk_t(const unsigned short* __restrict__ q,
                     const unsigned short* __restrict__ k,
                     const unsigned short* __restrict__ v,
                     const unsigned short* __restrict__ dout,
                     const float* __restrict__ lse,
                     const float* __restrict__ delta,
                     unsigned short* __restrict__ out_part,
                     int Hq, int Hkv, int S, float scale, int bshd) {
  __shared__ unsigned short lq[FB_OTH * FB_D];    // Q q-tile (swz)
  __shared__ unsigned short ldo[FB_OTH * FB_D];   // dO q-tile (swz)
  __shared__ float llse[FB_OTH];                  // q-tile rows' lse2
  __shared__ float ldelta[FB_OTH];                // dk only: never referenced, so never allocated, in dv

  const ff_ctx c = ff_prologue(Hq, Hkv, S);
  const int tid = c.tid, wave = c.wave, l31 = c.l31, half = c.half;
  const int64_t qbase = c.qbase, kbase = c.kbase;
  const int kvB = c.tile * FB_TILE;
  const int kv0w = kvB + wave * FB_OWN;
  const int my_kv = kv0w + l31;
  const float scale2 = scale * FF_LOG2E;

  // K (dk: and V) fragments (B-operands): lane holds K[my_kv][ks*16 + half*8 + e]
  // (v and delta are null in dv: every use of them is under if constexpr (DK))
  ff_shortx8 kf[8], vf[DK ? 8 : 1];
  {
    const unsigned short* kg = k + kbase + (int64_t)my_kv * FB_D;
    const unsigned short* vg = DK ? v + kbase + (int64_t)my_kv * FB_D : nullptr;
#pragma unroll
    for (int ks = 0; ks < 8; ++ks) {
      kf[ks] = ff_row_frag(kg, ks, half);
      if constexpr (DK) vf[ks] = ff_row_frag(vg, ks, half);
    }
  }

  ff_floatx16 acc[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) acc[i] = (ff_floatx16)(0.f);

  const int jq0 = kvB / FB_OTH;       // diagonal q tile, block-uniform
  const int n_jq = S / FB_OTH;
  const float* lseg = lse + c.rbase;
  const float* dltg = DK ? delta + c.rbase : nullptr;
  const ff_rows dorow = ff_o_rows(c, Hq, S, bshd);  // dout in either layout

  for (int jq = jq0; jq < n_jq; ++jq) {
    const int qt0 = jq * FB_OTH;
    const bool active = (qt0 + FB_OTH - 1 >= kv0w);
    const bool need_mask = (qt0 < kv0w + FB_OWN - 1);
    __syncthreads();
    ff_stage<FB_OTH, FB_THREADS>(q + qbase + (int64_t)qt0 * FB_D, lq, tid);
    ff_stage_rows<FB_OTH, FB_THREADS>(dout + dorow.base + (int64_t)qt0 * dorow.stride,
                                      dorow.stride, ldo, tid);
    if (tid < FB_OTH) {
      llse[tid] = lseg[qt0 + tid] * FF_LOG2E;
      if constexpr (DK) ldelta[tid] = dltg[qt0 + tid];
    }
    __syncthreads();

    if (active) {
      // ST = Q.K^T (dk: and dP = dO.V^T) -> D[q][kv], col = kv = l31
      ff_floatx16 st[2], dp[DK ? 2 : 1];
#pragma unroll
      for (int s2 = 0; s2 < 2; ++s2) {
        st[s2] = (ff_floatx16)(0.f);
        if constexpr (DK) dp[s2] = (ff_floatx16)(0.f);
      }
      if constexpr (!DK) {
        // dv has the registers (186 of 256) to read its 16 row fragments 4
        // MFMAs ahead: left alone the compiler reads one or two, waits and
        // multiplies, a full LDS round trip per pair of MFMAs.  The two
        // accumulator chains alternate; each chain's ks order, and so every
        // bit, is unchanged.  The group barriers pin the order: 4 reads, then
        // 12 x (MFMA, read), then the last 4 MFMAs (0x100 = DS read, 0x008 =
        // MFMA).  2.65 -> 2.50 ms per call at the bench shape; dk (254 VGPRs)
        // has no room for it.
        ff_shortx8 qfr[16];
#pragma unroll
        for (int i = 0; i < 16; ++i) qfr[i] = ff_afrag(lq, i & 1, i >> 1, l31, half);
#pragma unroll
        for (int i = 0; i < 16; ++i)
          st[i & 1] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(qfr[i], kf[i >> 1], st[i & 1], 0, 0, 0);
        __builtin_amdgcn_sched_group_barrier(0x100, 4, 0);
#pragma unroll
        for (int i = 0; i < 12; ++i) {
          __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
          __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);
        }
        __builtin_amdgcn_sched_group_barrier(0x008, 4, 0);
      } else {
#pragma unroll
        for (int s2 = 0; s2 < 2; ++s2)
#pragma unroll
          for (int ks = 0; ks < 8; ++ks) {
            ff_shortx8 qfr = ff_afrag(lq, s2, ks, l31, half);
            st[s2] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(qfr, kf[ks], st[s2], 0, 0, 0);
            ff_shortx8 dofr = ff_afrag(ldo, s2, ks, l31, half);
            dp[s2] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(dofr, vf[ks], dp[s2], 0, 0, 0);
          }
      }
      // mask q < kv: only a diagonal tile (wave-uniform need_mask) pays for it
      if (need_mask) ff_mask<false>(st, my_kv - qt0 - 4 * half);
      // P = exp2(st*scale2 - lse2[q row]) (broadcast reads);
      // dk: dS = P * (dP - delta[q row])
#pragma unroll
      for (int s2 = 0; s2 < 2; ++s2)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          int qrow = ff_drow(s2 * 32, r, half);
          float p = __builtin_amdgcn_exp2f(st[s2][r] * scale2 - llse[qrow]);
          if constexpr (DK) st[s2][r] = p * (dp[s2][r] - ldelta[qrow]);
          else st[s2][r] = p;
        }
      ff_shortx8 pb[4];
      ff_relayout(st, pb);  // B-frags [kv][q-contraction]
      // dv: acc[d][kv] += dO^T . P   |   dk: acc[d][kv] += Q^T . dS
      // (A via tr reads of dO | Q)
#pragma unroll
      for (int ds = 0; ds < 4; ++ds) {
        ff_shortx4 t[4][2];
        ff_tr_read8(DK ? lq : ldo, ds, tid, l31, half, t);
#pragma unroll
        for (int ks = 0; ks < 4; ++ks)
          acc[ds] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(
              ff_cat(t[ks][0], t[ks][1]), pb[ks], acc[ds], 0, 0, 0);
      }
    }
  }

  // epilogue (rows = d over regs, col = kv = l31 -> row write); dK = scale * acc
  unsigned short* og = out_part + qbase + (int64_t)my_kv * FB_D;
  ff_store_row<DK>(og, acc, scale, half);
}

extern "C" __global__ void __launch_bounds__(FB_THREADS, 2)
fa2_dv_bf16(const unsigned short* __restrict__ q,
            const unsigned short* __restrict__ k,
            const unsigned short* __restrict__ dout,
            const float* __restrict__ lse,
            unsigned short* __restrict__ dv_part,
            int B, int Hq, int Hkv, int S, float scale, int bshd) {
  fa2_dv_dk_t<false>(q, k, nullptr, dout, lse, nullptr, dv_part, Hq, Hkv, S, scale, bshd);
}

extern "C" __global__ void __launch_bounds__(FB_THREADS, 2)
fa2_dk_bf16(const unsigned short* __restrict__ q,
            const unsigned short* __restrict__ k,
            const unsigned short* __restrict__ v,
            const unsigned short* __restrict__ dout,
            const float* __restrict__ lse,
            const float* __restrict__ delta,
            unsigned short* __restrict__ dk_part,
            int B, int Hq, int Hkv, int S, float scale, int bshd) {
  fa2_dv_dk_t<true>(q, k, v, dout, lse, delta, dk_part, Hq, Hkv, S, scale, bshd);
}

// ---------------------------------------------------------------------------
// fa2_dvdk: fused dV + dK.  The two split kernels share the Q/dO staging,
// the ST = Q.K^T GEMM, the lse/delta loads and a barrier pair per q-tile;
// fusing removes that duplicated work plus one kernel launch.
//
// Geometry: 4 waves / 256 threads, 128-kv-row block tile (HALF the split
// kernels' 8-wave/256-row blocks).  Reason: a wave needs two fp32
// accumulator banks (dV, dK: 64 VGPRs each) + st/dp + operands ~ 320 regs.
// A gfx950 wave can hold up to 512 (256 arch VGPRs + AGPR overflow) but
// only at 1 wave/SIMD — so an 8-wave block (which forces >= 2 waves/SIMD)
// pins the budget at 256 and spills 264-484 B/lane to scratch (measured
// via -Rpass-analysis).  At 4 waves/block the block fits one-per-CU with
// each wave on its own SIMD and the full 512-reg budget.
//
// K and V live in LDS (staged ONCE - the block's own kv-tile never
// changes), read as B-fragments with ff_bfrag, the same pattern fa2_dq
// uses for dO.  lse/delta travel as one wave register each (lane i holds
// row qt0+i) broadcast per-element with ds_bpermute.  st[] is rewritten in
// place P -> dS between the two MFMA phases so relayout/tr temporaries are
// shared.  LDS 96 KB/block.  Replaces fa2_dv_bf16 + fa2_dk_bf16 (kept
// above for A/B).
// ---------------------------------------------------------------------------
#define FD_WAVES 4
#define FD_THREADS (FD_WAVES * 64)
#define FD_TILE (FD_WAVES * FB_OWN)  // 128 kv rows per block

extern "C" __global__ void __launch_bounds__(FD_THREADS, 1)
fa2_dvdk_bf16(const unsigned short* __restrict__ q,
              const unsigned short* __restrict__ k,
              const unsigned short* __restrict__ v,
              const unsigned short* __restrict__ dout,
              const float* __restrict__ lse,
              const float* __restrict__ delta,
              unsigned short* __restrict__ dv_part,
              unsigned short* __restrict__ dk_part,
              int B, int Hq, int Hkv, int S, float scale) {
  __shared__ unsigned short lq[FB_OTH * FB_D];    // Q q-tile (swz)
  __shared__ unsigned short ldo[FB_OTH * FB_D];   // dO q-tile (swz)
  __shared__ unsigned short lk[FD_TILE * FB_D];   // block's K kv rows (swz)
  __shared__ unsigned short lv[FD_TILE * FB_D];   // block's V kv rows (swz)

  // Open-coded rather than ff_prologue: through the helper this kernel's
  // registers are allocated differently, and it has none to spare.
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = tid >> 6;
  const int l31 = lane & 31;
  const int half = lane >> 5;

  int bx = blockIdx.x, by = blockIdx.y, bz = blockIdx.z;
  ff_xcd_remap(bx, by, bz);
  const int kt = bx;
  const int h = by;
  const int b = bz;
  const int hkv = h / (Hq / Hkv);
  const int64_t qbase = (((int64_t)b * Hq + h) * S) * FB_D;
  const int64_t kbase = (((int64_t)b * Hkv + hkv) * S) * FB_D;
  const int kvB = kt * FD_TILE;
  const int kv0w = kvB + wave * FB_OWN;
  const int my_kv = kv0w + l31;
  const int myrow = wave * FB_OWN + l31;  // my kv row within the block tile
  const float scale2 = scale * FF_LOG2E;

  // stage the block's K/V kv rows once (swizzled, block-cooperative)
  {
    const unsigned short* kg = k + kbase + (int64_t)kvB * FB_D;
    const unsigned short* vg = v + kbase + (int64_t)kvB * FB_D;
#pragma unroll
    for (int j = 0; j < FF_STAGE_CHUNKS(FD_TILE, FD_THREADS); ++j) {
      const int e = ff_chunk<FD_THREADS>(j, tid);
      ff_chunk_store(ff_chunk_load(kg, e), lk, e);
      ff_chunk_store(ff_chunk_load(vg, e), lv, e);
    }
  }

  ff_floatx16 dvacc[4], dkacc[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    dvacc[i] = (ff_floatx16)(0.f);
    dkacc[i] = (ff_floatx16)(0.f);
  }

  const int jq0 = kvB / FB_OTH;
  const int n_jq = S / FB_OTH;
  const float* lseg = lse + ((int64_t)b * Hq + h) * S;
  const float* dltg = delta + ((int64_t)b * Hq + h) * S;

  for (int jq = jq0; jq < n_jq; ++jq) {
    const int qt0 = jq * FB_OTH;
    const bool active = (qt0 + FB_OTH - 1 >= kv0w);
    const bool need_mask = (qt0 < kv0w + FB_OWN - 1);
    __syncthreads();  // previous tile readers done; first iter: K/V staged
    ff_stage<FB_OTH, FD_THREADS>(q + qbase + (int64_t)qt0 * FB_D, lq, tid);
    ff_stage<FB_OTH, FD_THREADS>(dout + qbase + (int64_t)qt0 * FB_D, ldo, tid);
    const float lse_reg = lseg[qt0 + lane] * FF_LOG2E;
    const float dlt_reg = dltg[qt0 + lane];
    __syncthreads();

    if (active) {
      // ST = Q.K^T and dP = dO.V^T in one pass — both D[q][kv], col = kv
      ff_floatx16 st[2], dp[2];
#pragma unroll
      for (int s2 = 0; s2 < 2; ++s2) {
        st[s2] = (ff_floatx16)(0.f);
        dp[s2] = (ff_floatx16)(0.f);
      }
#pragma unroll
      for (int s2 = 0; s2 < 2; ++s2)
#pragma unroll
        for (int ks = 0; ks < 8; ++ks) {
          ff_shortx8 kfr = ff_bfrag(lk, myrow, ks, half);
          ff_shortx8 qfr = ff_afrag(lq, s2, ks, l31, half);
          st[s2] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(qfr, kfr, st[s2], 0, 0, 0);
          ff_shortx8 vfr = ff_bfrag(lv, myrow, ks, half);
          ff_shortx8 dofr = ff_afrag(ldo, s2, ks, l31, half);
          dp[s2] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(dofr, vfr, dp[s2], 0, 0, 0);
        }
      // mask q < kv on the diagonal tiles only, as fa2_dv / fa2_dk do
      if (need_mask) ff_mask<false>(st, my_kv - qt0 - 4 * half);
      // P = exp2(st*scale2 - lse2[q row]) in place
#pragma unroll
      for (int s2 = 0; s2 < 2; ++s2)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          int qrow = ff_drow(s2 * 32, r, half);
          float l2 = __int_as_float(
              __builtin_amdgcn_ds_bpermute(qrow * 4, __float_as_int(lse_reg)));
          st[s2][r] = __builtin_amdgcn_exp2f(st[s2][r] * scale2 - l2);
        }
      // dV phase: dVacc[d][kv] += dO^T . P
      {
        ff_shortx8 pb[4];
        ff_relayout(st, pb);  // B-frags [kv][q-contraction]
#pragma unroll
        for (int ds = 0; ds < 4; ++ds) {
          ff_shortx4 t[4][2];
          ff_tr_read8(ldo, ds, tid, l31, half, t);
#pragma unroll
          for (int ks = 0; ks < 4; ++ks)
            dvacc[ds] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(
                ff_cat(t[ks][0], t[ks][1]), pb[ks], dvacc[ds], 0, 0, 0);
        }
      }
      // dS = P * (dP - delta[q row]) in place, then dK phase
#pragma unroll
      for (int s2 = 0; s2 < 2; ++s2)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          int qrow = ff_drow(s2 * 32, r, half);
          float dl = __int_as_float(
              __builtin_amdgcn_ds_bpermute(qrow * 4, __float_as_int(dlt_reg)));
          st[s2][r] = st[s2][r] * (dp[s2][r] - dl);
        }
      {
        ff_shortx8 pb[4];
        ff_relayout(st, pb);  // B-frags [kv][q-contraction]
        // dKacc[d][kv] += Q^T . dS
#pragma unroll
        for (int ds = 0; ds < 4; ++ds) {
          ff_shortx4 t[4][2];
          ff_tr_read8(lq, ds, tid, l31, half, t);
#pragma unroll
          for (int ks = 0; ks < 4; ++ks)
            dkacc[ds] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(
                ff_cat(t[ks][0], t[ks][1]), pb[ks], dkacc[ds], 0, 0, 0);
        }
      }
    }
  }

  // epilogues: dV[kv][d] = acc ; dK[kv][d] = scale * acc
  unsigned short* ogv = dv_part + qbase + (int64_t)my_kv * FB_D;
  unsigned short* ogk = dk_part + qbase + (int64_t)my_kv * FB_D;
#pragma unroll
  for (int ds = 0; ds < 4; ++ds)
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      ff_store_elem(ogv, ds, r, half, dvacc[ds][r]);
      ff_store_elem(ogk, ds, r, half, dkacc[ds][r] * scale);
    }
}
