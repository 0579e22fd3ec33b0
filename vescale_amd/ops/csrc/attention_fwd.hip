// Flash-attention FORWARD — CDNA4 MFMA (32x32x16), causal, GQA, D=128.
//
// Structure per /opt/skills/guides/cdna_hip_programming.md App. B (the
// 8-wave 32x32 ladder) using the probe-verified fragment layouts
// (tools/fa_fwd_check.py runs the layout probes on every check):
//   - 4 waves x QBLK=32 q-rows each = 128 q rows per block; 4-wave
//     blocks (not 8) so TWO independent blocks fit per CU and drift out
//     of phase — one block's MFMA overlaps the other's softmax VALU
//     (barriers phase-lock waves WITHIN a block only)
//   - swapped QK^T: ST = mfma(A=K, B=Q) -> D-layout col = q = lane&31, so
//     the online softmax (running m, l per q) is LANE-LOCAL up to one
//     permlane32_swap combining the half-wave kv clusters
//   - P -> PV B-operand relayout in-register: v_cvt_pk_bf16_f32 pairs +
//     permlane32_swap (guide T12: one swap fills both half-kv words; no
//     LDS round trip, no divergent branch)
//   - V staged EXACTLY like K (row-major + XOR swizzle, direct loads)
//     and the PV A-operand (V^T) read with ds_read_b64_tr_b16 (guide
//     T10): probe-measured semantics (tools/tr_probe_check.py) are a 4x4
//     transpose within each aligned 4-lane group — lane l elem j receives
//     the (l&3)-th element of the 64b read issued by lane (l&~3)+j — so
//     pointing lanes of a group at 4 consecutive kv rows (same d column
//     group) yields the transposed fragment for free; the row-XOR swizzle
//     (fa32_lds_map.h) sends the 4 rows to 4 different 64-byte column
//     bands, so these reads and the K row-fragment reads are both
//     bank-conflict-free
//   - K/V tiles DOUBLE-BUFFERED in LDS by direct global -> LDS loads
//     (ff_stage_async: no staging register, no ds_write): tile j+1's loads
//     issue before tile j's compute into the other buffer, ONE wait + ONE
//     barrier per tile, at its top
//   - O accumulates in D-layout (col = q), so the online rescale by
//     exp(m_old - m_new) is a lane-local scalar multiply
//   - outputs: O [B,H,S,D] (or, out_bshd, [B,S,H,D] — the layout the
//     output projection reads, so no transpose copy follows) bf16 and
//     logsumexp [B,H,S] fp32 (ln), matching
//     the stock flash convention so EITHER backward (ours or the
//     library's) can consume it.
//   - packed documents (fa_fwd_seg_bf16, template SEG): documents are runs of
//     equal segment ids; a pre-pass (fa_seg_bounds_i32) writes each position's
//     run start and end, a lane keeps ONE integer (its row's start), the block
//     starts at its first row's document (the prologue stages THAT tile) and
//     a wave computes and masks by two scalars.  fa_fwd_bf16 is the SEG=false
//     instantiation: the instructions it had before the template.
//   - no mask (fa_fwd_full_bf16, template FULL): every q row sees every key,
//     and q and k/v have lengths of their own (Sq rows of q, o and lse, Sk rows
//     of k and v): encoders, cross attention, the past blocks of ring
//     attention.  Every block walks all Sk/64 kv tiles and no wave is ever
//     inactive, so the activity test, the mask and its compare are compiled out.
// Capability parity: reference vescale relies on library flash attention;
// this is the MI355X-native forward for the train step's hot op.
#include "fa32_common.h"

#define FF_QBLK 32             // q rows per wave
#define FF_WAVES 4
#define FF_QTILE (FF_QBLK * FF_WAVES)  // 128 q rows per block
#define FF_KV 64               // kv tile
#define FF_THREADS (FF_WAVES * 64)

// SEG: the packed-document mask of fa32_common.h (bounds [B,2,S] from the
// pre-pass; null and never read when !SEG).
// FULL: no mask, S rows of q / o / lse and Sk rows of k / v (Sk is read in
// FULL only: the masked kernels are square).  Never combined with SEG.
template <int MODE, bool SEG = false, bool FULL = false>  // MODE: 0=whole kernel, 1=no-softmax, 2=no-PV, 3=no-ST, 4=no-gating, 5=exp-domain (bisect)
DEV void fa_fwd_t(const unsigned short* __restrict__ q,
            const unsigned short* __restrict__ k,
            const unsigned short* __restrict__ v,
            unsigned short* __restrict__ out,
            float* __restrict__ lse,
            int B, int Hq, int Hkv, int S, float scale, int out_bshd,
            const int* __restrict__ bounds = nullptr, int Sk = 0) {
  static_assert(!(SEG && FULL), "FULL has no mask at all");
  __shared__ unsigned short lk[2][FF_KV * FF_D];  // K, swizzled
  __shared__ unsigned short lv[2][FF_KV * FF_D];  // V, swizzled (same as K)

  const ff_ctx c = ff_prologue(Hq, Hkv, S, FULL ? Sk : S);
  const int tid = c.tid, lane = c.lane, l31 = c.l31, half = c.half;
  // q macro-tile, ascending.  (Walking a head's tiles heaviest first, as
  // fa2_dq does, was measured here too: 3.51 -> 3.42 ms per call, inside this
  // kernel's own call-to-call spread of 0.08-0.10 ms, so it was not kept.)
  const int qt = c.tile;
  const int q0 = qt * FF_QTILE + c.wave * FF_QBLK;   // wave's first q row
  const int my_q = q0 + l31;                         // this lane's q row
  const float scale2 = (MODE == 5) ? scale : scale * FF_LOG2E;

  // ---- Q fragments in registers: B-operand B[j=q][k=d] ----
  // lane holds Q[my_q][ (half*8 + e) + 16*ks ] for ks = 0..7
  ff_shortx8 qf[8];
  ff_row_frags(q + c.qbase + (int64_t)my_q * FF_D, qf, half);

  // ---- online-softmax state (per q = l31; replicated across halves) ----
  float m_run = -INFINITY;
  float l_run = 0.f;
  // O accumulator: 4 d-subtiles (32 d each) in D-layout:
  //   acc[ds] reg r holds O[d = ff_drow(ds*32, r, half)][q=l31]
  ff_floatx16 oacc[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) oacc[i] = (ff_floatx16)(0.f);

  // BLOCK-UNIFORM kv loop bound (all 4 waves hit the same barriers):
  // cover kv < (qt+1)*128, i.e. through the block's last causal tile.
  // FULL: every tile of k, the same for all blocks.
  const int n_kv = (qt + 1) * (FF_QTILE / FF_KV);
  const int last_kv = FULL ? Sk / FF_KV : min(n_kv, S / FF_KV);

  // SEG: one integer per lane, the first key of its row's document; the mask
  // is my_start <= kv <= my_q.  start is monotone, so the wave's first row
  // (lane 0) holds the wave's minimum, its last row (lane 31) the maximum, and
  // the block's first row the block's minimum: the block's first kv tile.  It
  // is block-uniform (all 4 waves stage and reach the same barriers) and held
  // to [0, last_kv - 1] whatever bounds contains.
  int my_start = 0, wstart_lo = 0, wstart_hi = 0, first_kv = 0;
  if constexpr (SEG) {
    const int* start = ff_seg_start(bounds, c.b, S);
    my_start = start[my_q];
    wstart_lo = __builtin_amdgcn_readfirstlane(my_start);
    wstart_hi = __builtin_amdgcn_readlane(my_start, 31);
    first_kv = ff_seg_tile(start[qt * FF_QTILE] / FF_KV, 0, last_kv - 1);
  }

  // the prologue stages the block's first tile (tile 0 without SEG) into the
  // buffer the loop reads it from (buf = jkv & 1)
  const unsigned short* kg = k + c.kbase;
  const unsigned short* vg = v + c.kbase;
  const unsigned short* kg0 = kg + (int64_t)first_kv * (FF_KV * FF_D);
  const unsigned short* vg0 = vg + (int64_t)first_kv * (FF_KV * FF_D);
  const int buf0 = first_kv & 1;
  // direct global -> LDS loads (ff_stage_async): no staging register, no
  // ds_write; the loop's first wait + barrier makes the tile readable.
  // Unguarded, unlike the backward kernels' prologues: last_kv >= 1 (S >= 64,
  // qt >= 0) and first_kv <= last_kv - 1 (ff_seg_tile above), so the tile
  // exists and the loop runs at least once.
  ff_stage_async<FF_KV, FF_THREADS>(kg0, FF_D, lk[buf0], tid);
  ff_stage_async<FF_KV, FF_THREADS>(vg0, FF_D, lv[buf0], tid);

  for (int jkv = first_kv; jkv < last_kv; ++jkv) {
    const int kv0 = jkv * FF_KV;
    const int buf = jkv & 1;
    const bool have_next = (jkv + 1 < last_kv);
    // wave-uniform activity: a wave whose whole q-range is above this kv
    // tile skips ALL compute (it still stages + hits the barrier). Active
    // tiles always satisfy kv0 <= q0 <= min(my_q), so no lane is ever
    // fully masked and no -inf/-inf NaN guards are needed.
    // SEG: the wave is also inactive while the tile lies before its first
    // row's document, and also masks while the tile begins before its last
    // row's document.  A wave that straddles a document boundary then HAS
    // lanes whose whole tile is masked (their document begins after it): the
    // dead-lane guard below is theirs.  Tiles inside one document stay on the
    // unmasked path.
    // FULL: every wave is active in every tile and nothing is masked: both
    // flags are compile-time constants, the branch on `active` and the masked
    // arm below are not compiled.  No guard is needed either: every lane sees
    // 64 keys in its first tile (Sk >= 64), so m_new and from then on m_run
    // are finite, the first corr is exp2(-inf - finite) = 0 and no
    // exp2(-inf - -inf) is ever evaluated.
    bool active = FULL || (MODE == 4) || (kv0 <= q0 + FF_QBLK - 1);
    // wave-uniform mask need: only diagonal tiles pay the per-element cmp
    bool need_mask = !FULL && ((MODE == 4) || (kv0 + FF_KV - 1 > q0));
    if constexpr (SEG) {
      active = active && (kv0 + FF_KV - 1 >= wstart_lo);
      need_mask = need_mask || (kv0 < wstart_hi);
    }
    // One barrier per tile.  ff_stage_wait: this wave's loads of tile jkv (and,
    // in the first iteration, its Q fragments) have landed; it also leaves the
    // compiler's scoreboard clean, so no counted vmcnt wait of the prologue's
    // loads is carried into the QK^T block of every iteration
    // (NOTES_FA32_LOOPS.md, C).  After the barrier tile jkv is visible to all
    // waves and every wave is done reading tile jkv - 1, whose buffer the loads
    // of tile jkv + 1 then fill while this tile is computed.  Every wave issues
    // them, active or not; have_next is block-uniform and the last iteration
    // forms no address.
    ff_stage_wait();
    __syncthreads();
    if (have_next) {
      ff_stage_async<FF_KV, FF_THREADS>(kg + (int64_t)(kv0 + FF_KV) * FF_D, FF_D, lk[buf ^ 1], tid);
      ff_stage_async<FF_KV, FF_THREADS>(vg + (int64_t)(kv0 + FF_KV) * FF_D, FF_D, lv[buf ^ 1], tid);
    }

    if (active) {
    // ---- ST = K . Q^T : 2 kv-subtiles of 32, contraction d (8 ksteps) ----
    ff_floatx16 st[2];
#pragma unroll
    for (int s2 = 0; s2 < 2; ++s2) st[s2] = (ff_floatx16)(MODE == 3 ? 1e-3f : 0.f);
    if constexpr (MODE != 3)
#pragma unroll
    for (int s2 = 0; s2 < 2; ++s2) {
#pragma unroll
      for (int ks = 0; ks < 8; ++ks) {
        // A-frag: K rows (s2*32 + l31), d = ks*16 + half*8 .. +8
        ff_shortx8 kf = ff_afrag(lk[buf], s2, ks, l31, half);
        st[s2] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(kf, qf[ks], st[s2], 0, 0, 0);
      }
    }

    if constexpr (MODE == 1 || MODE == 3) {
      // ablation: skip softmax; keep state plausible so loop carries on
      l_run += 1.f; m_run = 0.f;
    } else {
    // ---- causal mask + online softmax, exp2 domain (per q = l31) ----
    // lane holds ST[kv][q=l31] at kv = ff_drow(kv0 + s2*32, r, half).
    // Work in log2: x2 = s * scale*log2(e); p = exp2(x2 - m2) maps to a
    // bare v_exp_f32 (no hidden 1/ln2 multiply per element).
    float pmax = -INFINITY;
    if (need_mask) {
#pragma unroll
      for (int s2 = 0; s2 < 2; ++s2)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          int kv = ff_drow(kv0 + s2 * 32, r, half);
          const bool vis = SEG ? (kv <= my_q && kv >= my_start) : (kv <= my_q);
          float x = vis ? st[s2][r] * scale2 : -INFINITY;
          st[s2][r] = x;
          pmax = fmaxf(pmax, x);
        }
    } else {
#pragma unroll
      for (int s2 = 0; s2 < 2; ++s2)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          float x = st[s2][r] * scale2;
          st[s2][r] = x;
          pmax = fmaxf(pmax, x);
        }
    }
    // combine halves: each (q) lives in lanes l31 and l31+32
    pmax = fmaxf(pmax, __int_as_float(ff_swap_other(__float_as_int(pmax), half)));
    float m_new = fmaxf(m_run, pmax);  // finite: active tiles have kv0 <= my_q
    bool dead = false;
    if constexpr (MODE == 4) dead = (m_new == -INFINITY);
    // SEG dead lane: nothing seen yet and nothing in this tile (m_run = m_new =
    // -inf).  The exponentials below take 0 in place of m_new: corr =
    // exp2(-inf - 0) = 0 and is then set to 1, p = exp2(-inf - 0) = 0 for all
    // 32 elements with no select per element, and no exp2(-inf - -inf) is
    // evaluated.  m_run stays -inf, so the lane comes alive at its document's
    // first tile exactly like a lane at its first tile.
    bool seg_dead = false;
    float m_exp = m_new;
    if constexpr (SEG) {
      seg_dead = (m_new == -INFINITY);
      m_exp = seg_dead ? 0.f : m_new;
    }
    float corr;
    if constexpr (MODE == 5) corr = __expf(m_run - m_new);
    else corr = __builtin_amdgcn_exp2f(m_run - m_exp);  // m_run=-inf -> 0
    if (dead) { corr = 1.f; m_new = m_run; }
    if (seg_dead) corr = 1.f;
    float psum = 0.f;
#pragma unroll
    for (int s2 = 0; s2 < 2; ++s2)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        float p;
        if (dead) p = 0.f;
        else if constexpr (MODE == 5) p = (st[s2][r] == -INFINITY) ? 0.f : __expf(st[s2][r] - m_new);
        else p = __builtin_amdgcn_exp2f(st[s2][r] - m_exp);  // -inf -> 0
        st[s2][r] = p;
        psum += p;
      }
    psum += __int_as_float(ff_swap_other(__float_as_int(psum), half));
    l_run = l_run * corr + psum;
    m_run = m_new;

    // rescale O accumulator by corr (lane-local: every reg shares q=l31)
#pragma unroll
    for (int ds = 0; ds < 4; ++ds)
#pragma unroll
      for (int r = 0; r < 16; ++r) oacc[ds][r] *= corr;
    }  // end softmax (MODE != 1,3)

    if constexpr (MODE == 2) {
      // ablation: consume st into oacc so ST isn't dead-code-eliminated
#pragma unroll
      for (int r = 0; r < 16; ++r) oacc[0][r] += st[0][r] + st[1][r];
    } else {
    // ---- P relayout to PV B-operand (4 ksteps of 16 kv, KV=64) ----
    ff_shortx8 pb[4];
    ff_relayout(st, pb);
    // ---- PV: O[d][q] += V^T . P  (contraction kv; A-frag V^T rows
    // d = ds*32 + l31 via tr reads of the V tile) ----
#pragma unroll
    for (int ds = 0; ds < 4; ++ds) {
      ff_shortx4 t[4][2];
      ff_tr_read8(lv[buf], ds, lane, l31, half, t);
#pragma unroll
      for (int ks = 0; ks < 4; ++ks)
        oacc[ds] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(
            ff_cat(t[ks][0], t[ks][1]), pb[ks], oacc[ds], 0, 0, 0);
    }
    }  // end relayout+PV (MODE != 2)
    }  // end if (active)
  }

  // the rule of all four kernels: nothing pending when the wave ends (here the
  // loop's last wait already saw to it)
  ff_stage_wait();

  // ---- epilogue: O[q][d] = acc / l ; lse = m2*ln2 + ln(l) (m2 log2-dom) ----
  float inv_l = (l_run > 0.f) ? 1.0f / l_run : 0.f;
  // out rows in the caller's layout ([B,Hq,S,D] or [B,S,Hq,D]): a row is 128
  // contiguous elements in both, only its address differs.
  const ff_rows orow = ff_o_rows(c, Hq, S, out_bshd);
  ff_store_row(out + orow.base + (int64_t)my_q * orow.stride, oacc, inv_l, half);
  if (half == 0)
    lse[c.rbase + my_q] = m_run * (MODE == 5 ? 1.0f : FF_LN2) + __logf(l_run);
}

// instantiations: the real kernel + ablation variants for profiling
extern "C" __global__ void FF_NO_PK_F32 __launch_bounds__(FF_THREADS, 2)
fa_fwd_bf16(const unsigned short* q, const unsigned short* k,
            const unsigned short* v, unsigned short* out, float* lse,
            int B, int Hq, int Hkv, int S, float scale, int out_bshd) {
  fa_fwd_t<0>(q, k, v, out, lse, B, Hq, Hkv, S, scale, out_bshd);
}
extern "C" __global__ void FF_NO_PK_F32 __launch_bounds__(FF_THREADS, 2)
fa_fwd_bf16_ab1(const unsigned short* q, const unsigned short* k,
                const unsigned short* v, unsigned short* out, float* lse,
                int B, int Hq, int Hkv, int S, float scale, int out_bshd) {
  fa_fwd_t<1>(q, k, v, out, lse, B, Hq, Hkv, S, scale, out_bshd);
}
extern "C" __global__ void FF_NO_PK_F32 __launch_bounds__(FF_THREADS, 2)
fa_fwd_bf16_ab2(const unsigned short* q, const unsigned short* k,
                const unsigned short* v, unsigned short* out, float* lse,
                int B, int Hq, int Hkv, int S, float scale, int out_bshd) {
  fa_fwd_t<2>(q, k, v, out, lse, B, Hq, Hkv, S, scale, out_bshd);
}
extern "C" __global__ void FF_NO_PK_F32 __launch_bounds__(FF_THREADS, 2)
fa_fwd_bf16_ab3(const unsigned short* q, const unsigned short* k,
                const unsigned short* v, unsigned short* out, float* lse,
                int B, int Hq, int Hkv, int S, float scale, int out_bshd) {
  fa_fwd_t<3>(q, k, v, out, lse, B, Hq, Hkv, S, scale, out_bshd);
}
extern "C" __global__ void FF_NO_PK_F32 __launch_bounds__(FF_THREADS, 2)
fa_fwd_bf16_ab4(const unsigned short* q, const unsigned short* k,
                const unsigned short* v, unsigned short* out, float* lse,
                int B, int Hq, int Hkv, int S, float scale, int out_bshd) {
  fa_fwd_t<4>(q, k, v, out, lse, B, Hq, Hkv, S, scale, out_bshd);
}
extern "C" __global__ void FF_NO_PK_F32 __launch_bounds__(FF_THREADS, 2)
fa_fwd_bf16_ab5(const unsigned short* q, const unsigned short* k,
                const unsigned short* v, unsigned short* out, float* lse,
                int B, int Hq, int Hkv, int S, float scale, int out_bshd) {
  fa_fwd_t<5>(q, k, v, out, lse, B, Hq, Hkv, S, scale, out_bshd);
}

// ---- packed documents: the pre-pass and the SEG forward ----
// ids [B,S] -> bounds [B,2,S] (fa32_common.h); grid (ceil(S/256), B)
extern "C" __global__ void __launch_bounds__(FF_SEG_THREADS)
fa_seg_bounds_i32(const int* ids, int* bounds, int S) {
  ff_seg_bounds(ids, bounds, S);
}
// fa_fwd_bf16 without a mask, Sq rows of q against Sk rows of k / v; grid
// (Sq/128, Hq, B).  Resources (the extension's flags,
// -Rpass-analysis=kernel-resource-usage): 199 VGPRs, 0 AGPRs, 64 KiB LDS,
// scratch 0, no spills, 2 waves/SIMD.
extern "C" __global__ void FF_NO_PK_F32 __launch_bounds__(FF_THREADS, 2)
fa_fwd_full_bf16(const unsigned short* q, const unsigned short* k,
                 const unsigned short* v, unsigned short* out, float* lse,
                 int B, int Hq, int Hkv, int Sq, int Sk, float scale, int out_bshd) {
  fa_fwd_t<0, false, true>(q, k, v, out, lse, B, Hq, Hkv, Sq, scale, out_bshd, nullptr, Sk);
}
// fa_fwd_bf16 with the packed-document mask.  Resources (the extension's flags,
// -Rpass-analysis=kernel-resource-usage): 204 VGPRs, 0 AGPRs, 64 KiB LDS,
// scratch 0, no spills, 2 waves/SIMD (fa_fwd_bf16: 203, the rest equal); the
// pre-pass 18 VGPRs, 1 KiB LDS, 8 waves/SIMD.
extern "C" __global__ void FF_NO_PK_F32 __launch_bounds__(FF_THREADS, 2)
fa_fwd_seg_bf16(const unsigned short* q, const unsigned short* k,
                const unsigned short* v, unsigned short* out, float* lse,
                const int* bounds, int B, int Hq, int Hkv, int S, float scale,
                int out_bshd) {
  fa_fwd_t<0, true>(q, k, v, out, lse, B, Hq, Hkv, S, scale, out_bshd, bounds);
}
