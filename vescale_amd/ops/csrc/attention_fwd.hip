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
//   - V staged EXACTLY like K (row-major + XOR swizzle, vector stores)
//     and the PV A-operand (V^T) read with ds_read_b64_tr_b16 (guide
//     T10): probe-measured semantics (tools/tr_probe_check.py) are a 4x4
//     transpose within each aligned 4-lane group — lane l elem j receives
//     the (l&3)-th element of the 64b read issued by lane (l&~3)+j — so
//     pointing lanes of a group at 4 consecutive kv rows (same d column
//     group) yields the transposed fragment for free; the row-XOR swizzle
//     (fa32_lds_map.h) sends the 4 rows to 4 different 64-byte column
//     bands, so these reads and the K row-fragment reads are both
//     bank-conflict-free
//   - K/V tiles DOUBLE-BUFFERED in LDS: tile j+1's global loads issue
//     before tile j's compute, stores land in the other buffer, ONE
//     barrier per tile (guide T3/T4 phase overlap, structured form)
//   - O accumulates in D-layout (col = q), so the online rescale by
//     exp(m_old - m_new) is a lane-local scalar multiply
//   - outputs: O [B,H,S,D] (or, out_bshd, [B,S,H,D] — the layout the
//     output projection reads, so no transpose copy follows) bf16 and
//     logsumexp [B,H,S] fp32 (ln), matching
//     the stock flash convention so EITHER backward (ours or the
//     library's) can consume it.
// Capability parity: reference vescale relies on library flash attention;
// this is the MI355X-native forward for the train step's hot op.
#include "fa32_common.h"

#define FF_QBLK 32             // q rows per wave
#define FF_WAVES 4
#define FF_QTILE (FF_QBLK * FF_WAVES)  // 128 q rows per block
#define FF_KV 64               // kv tile
#define FF_THREADS (FF_WAVES * 64)
#define FF_CHUNKS FF_STAGE_CHUNKS(FF_KV, FF_THREADS)  // staging chunks per thread per tile

template <int MODE>  // 0=full, 1=no-softmax, 2=no-PV, 3=no-ST, 4=no-gating, 5=exp-domain (bisect)
DEV void fa_fwd_t(const unsigned short* __restrict__ q,
            const unsigned short* __restrict__ k,
            const unsigned short* __restrict__ v,
            unsigned short* __restrict__ out,
            float* __restrict__ lse,
            int B, int Hq, int Hkv, int S, float scale, int out_bshd) {
  __shared__ unsigned short lk[2][FF_KV * FF_D];  // K, swizzled
  __shared__ unsigned short lv[2][FF_KV * FF_D];  // V, swizzled (same as K)

  const ff_ctx c = ff_prologue(Hq, Hkv, S);
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
  const int n_kv = (qt + 1) * (FF_QTILE / FF_KV);
  const int last_kv = min(n_kv, S / FF_KV);

  const unsigned short* kg = k + c.kbase;
  const unsigned short* vg = v + c.kbase;
  // staging registers: tile elems / threads / 8 chunks per thread
  ff_shortx8 kreg[FF_CHUNKS], vreg[FF_CHUNKS];
#pragma unroll
  for (int j = 0; j < FF_CHUNKS; ++j) {
    const int e = ff_chunk<FF_THREADS>(j, tid);
    kreg[j] = ff_chunk_load(kg, e);
    vreg[j] = ff_chunk_load(vg, e);
  }
#pragma unroll
  for (int j = 0; j < FF_CHUNKS; ++j) {
    const int e = ff_chunk<FF_THREADS>(j, tid);
    ff_chunk_store(kreg[j], lk[0], e);
    ff_chunk_store(vreg[j], lv[0], e);
  }
  // Retire every vector load here (s_waitcnt vmcnt(0); expcnt and lgkmcnt
  // fields left at "no wait").  The compiler schedules the 8 Q-fragment loads
  // after the tile-0 K/V loads and waits only for the latter before this
  // barrier, so its scoreboard enters the loop with 8 loads pending and it
  // puts vmcnt(7)..vmcnt(0) in front of the QK^T MFMAs that read qf[0..7] in
  // EVERY iteration.  From the second tile on those counts no longer cover Q
  // but the 8 K/V prefetch loads issued just above them, and the wave stalls
  // on the prefetch that the double buffer exists to carry across softmax and
  // PV.  With the scoreboard clean the loop's only vmcnt wait is in front of
  // the staging stores after PV.  (A builtin, not inline asm: the wait-count
  // pass does not look inside an asm statement.)
  __builtin_amdgcn_s_waitcnt(0x0F70);
  __syncthreads();

  for (int jkv = 0; jkv < last_kv; ++jkv) {
    const int kv0 = jkv * FF_KV;
    const int buf = jkv & 1;
    const bool have_next = (jkv + 1 < last_kv);
    // wave-uniform activity: a wave whose whole q-range is above this kv
    // tile skips ALL compute (it still stages + hits the barrier). Active
    // tiles always satisfy kv0 <= q0 <= min(my_q), so no lane is ever
    // fully masked and no -inf/-inf NaN guards are needed.
    const bool active = (MODE == 4) || (kv0 <= q0 + FF_QBLK - 1);
    // wave-uniform mask need: only diagonal tiles pay the per-element cmp
    const bool need_mask = (MODE == 4) || (kv0 + FF_KV - 1 > q0);
    // issue next tile's global loads BEFORE compute (latency overlap)
    if (have_next) {
      const unsigned short* kn = kg + (int64_t)(kv0 + FF_KV) * FF_D;
      const unsigned short* vn = vg + (int64_t)(kv0 + FF_KV) * FF_D;
#pragma unroll
      for (int j = 0; j < FF_CHUNKS; ++j) {
        const int e = ff_chunk<FF_THREADS>(j, tid);
        kreg[j] = ff_chunk_load(kn, e);
        vreg[j] = ff_chunk_load(vn, e);
      }
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
          float x = (kv <= my_q) ? st[s2][r] * scale2 : -INFINITY;
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
    float corr;
    if constexpr (MODE == 5) corr = __expf(m_run - m_new);
    else corr = __builtin_amdgcn_exp2f(m_run - m_new);  // m_run=-inf -> 0
    if (dead) { corr = 1.f; m_new = m_run; }
    float psum = 0.f;
#pragma unroll
    for (int s2 = 0; s2 < 2; ++s2)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        float p;
        if (dead) p = 0.f;
        else if constexpr (MODE == 5) p = (st[s2][r] == -INFINITY) ? 0.f : __expf(st[s2][r] - m_new);
        else p = __builtin_amdgcn_exp2f(st[s2][r] - m_new);  // -inf -> 0
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

    // store next tile into the other buffer, then one barrier
    if (have_next) {
#pragma unroll
      for (int j = 0; j < FF_CHUNKS; ++j) {
        const int e = ff_chunk<FF_THREADS>(j, tid);
        ff_chunk_store(kreg[j], lk[buf ^ 1], e);
        ff_chunk_store(vreg[j], lv[buf ^ 1], e);
      }
    }
    __syncthreads();
  }

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
extern "C" __global__ void __launch_bounds__(FF_THREADS, 2)
fa_fwd_bf16(const unsigned short* q, const unsigned short* k,
            const unsigned short* v, unsigned short* out, float* lse,
            int B, int Hq, int Hkv, int S, float scale, int out_bshd) {
  fa_fwd_t<0>(q, k, v, out, lse, B, Hq, Hkv, S, scale, out_bshd);
}
extern "C" __global__ void __launch_bounds__(FF_THREADS, 2)
fa_fwd_bf16_ab1(const unsigned short* q, const unsigned short* k,
                const unsigned short* v, unsigned short* out, float* lse,
                int B, int Hq, int Hkv, int S, float scale, int out_bshd) {
  fa_fwd_t<1>(q, k, v, out, lse, B, Hq, Hkv, S, scale, out_bshd);
}
extern "C" __global__ void __launch_bounds__(FF_THREADS, 2)
fa_fwd_bf16_ab2(const unsigned short* q, const unsigned short* k,
                const unsigned short* v, unsigned short* out, float* lse,
                int B, int Hq, int Hkv, int S, float scale, int out_bshd) {
  fa_fwd_t<2>(q, k, v, out, lse, B, Hq, Hkv, S, scale, out_bshd);
}
extern "C" __global__ void __launch_bounds__(FF_THREADS, 2)
fa_fwd_bf16_ab3(const unsigned short* q, const unsigned short* k,
                const unsigned short* v, unsigned short* out, float* lse,
                int B, int Hq, int Hkv, int S, float scale, int out_bshd) {
  fa_fwd_t<3>(q, k, v, out, lse, B, Hq, Hkv, S, scale, out_bshd);
}
extern "C" __global__ void __launch_bounds__(FF_THREADS, 2)
fa_fwd_bf16_ab4(const unsigned short* q, const unsigned short* k,
                const unsigned short* v, unsigned short* out, float* lse,
                int B, int Hq, int Hkv, int S, float scale, int out_bshd) {
  fa_fwd_t<4>(q, k, v, out, lse, B, Hq, Hkv, S, scale, out_bshd);
}
extern "C" __global__ void __launch_bounds__(FF_THREADS, 2)
fa_fwd_bf16_ab5(const unsigned short* q, const unsigned short* k,
                const unsigned short* v, unsigned short* out, float* lse,
                int B, int Hq, int Hkv, int S, float scale, int out_bshd) {
  fa_fwd_t<5>(q, k, v, out, lse, B, Hq, Hkv, S, scale, out_bshd);
}
