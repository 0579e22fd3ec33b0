// General-shape flash attention, forward + backward, with a differentiable
// log-sum-exp output — the correctness-first companion of the tuned D=128
// kernels (attention_fwd.hip / attention_bwd2.hip).
//
// Written on fa16_common.h, which states the skeleton: 64-row tiles, 4 waves
// (wave w owns rows [16w, 16w+16) of the tile), mfma_f32_16x16x32_bf16 in TN
// form, __syncthreads-staged, +8-elem LDS row pad.  A tile whose transpose is
// needed later is staged as rows and kept in its staging registers; once the
// rows are consumed the same LDS buffer is rewritten transposed from them.
// Templated on D in {64, 128}; everything else is a runtime argument.
//
// Layouts: q,o,dO,dq [B,Hq,Sq,D]; k,v,dk,dv [B,Hkv,Sk,D], contiguous bf16,
// Hq % Hkv == 0.  lse [B,Hq,Sq] fp32, natural log.  Sq, Sk independent, any
// value >= 1.
//
// Mask: with `causal`, key j is visible to query i iff j <= i + shift
// (shift = 0, Sq == Sk: the usual triangle; shift = Sk - Sq: bottom-right
// alignment; |shift| >= S: fully visible / fully masked block).  The host
// clamps shift to [-Sq, Sk], which leaves the mask unchanged and keeps the
// index arithmetic inside int.  KV (resp. Q) tiles wholly outside the
// visible range are skipped.
//
// Segment mask (packed documents), the compile-time variant SEG of fwd, dkdv
// and dq (template <int D, bool SEG>; preprocess needs nothing): with
// q_seg [B,Sq] and kv_seg [B,Sk] (int32), key j is visible to query i iff
// kv_seg[b,j] == q_seg[b,i] AND the rule above holds.  Ids are compared for
// equality only: no value is special and they need not be sorted.  The test
// is written once, in fg_vis<SEG>.  fa_gen_seg_bounds_kernel writes the
// (min, max) id of every 64-row q and kv tile first; a (q tile, kv tile) pair
// whose ranges do not overlap holds no equal pair and its whole loop
// iteration is skipped — staging and barriers included, on block-uniform
// scalar facts, for all waves at once.  Conservative for unsorted ids (a
// pair that is not skipped is masked element by element as ever).  The
// SEG = false instantiations are the kernels without any of this: the ids
// and bounds are dead arguments (null), registers and results unchanged.
//
// Tails: rows >= Sq / >= Sk are never loaded (every global load is
// predicated on its row, segment ids included) and never stored; staging
// zero-fills them, and the mask gives their scores no weight.  A tile's
// (min, max) leaves its tail rows out.
//
// Dead rows (no visible key; with SEG also a query whose id no visible key
// carries): o = 0 and lse = -inf exactly; in backward they contribute
// exactly zero (their P and dS are selected to 0, never computed as
// exp(-inf - -inf) or 0/0), and dlse is taken as 0 on them.  With SEG as
// without, P and dS of a masked entry are selected to exact 0, so a key that
// no query sees gets dk = dv = 0 exactly.
//
// Backward is the standard split plus the LSE gradient:
//   fa_gen_preprocess: delta[row] = rowsum(dO*O) - dlse[row] (0 on dead rows)
//   fa_gen_dkdv:       per KV tile, loops the GQA group in-kernel (fp32
//                      accumulation across the group, no partial buffers)
//   fa_gen_dq:         per Q tile
// No atomics anywhere, the segment pre-pass included (one wave per tile, a
// shuffle reduction, one plain store): repeated calls are bitwise equal,
// with and without segment ids.
//
// Build report (hipcc -O3 --offload-arch=gfx950,
// -Rpass-analysis=kernel-resource-usage): no scratch (0 B/lane) and no
// SGPR/VGPR spills in any instantiation.
//   kernel       D    SEG  VGPRs  AGPRs  LDS B/block  waves/SIMD (compiler)
//   fa_gen_fwd   64   -    98     16     27648        4
//   fa_gen_fwd   128  -    154    32     45056        2
//   fa_gen_dq    64   -    112    32     27648        3
//   fa_gen_dq    128  -    144    56     45056        2
//   fa_gen_dkdv  64   -    146    52     37376        2
//   fa_gen_dkdv  128  -    201    80     55808        1
//   fa_gen_fwd   64   yes  118    20     27648        3
//   fa_gen_fwd   128  yes  159    48     45056        2
//   fa_gen_dq    64   yes  106    52     27648        3
//   fa_gen_dq    128  yes  174    36     45056        2
//   fa_gen_dkdv  64   yes  176    30     37376        2
//   fa_gen_dkdv  128  yes  248    40     55808        1
//   fa_gen_seg_bounds      8      0      0            8
// The segment variants hold 8 ids per lane (4 rows, 4 columns) and the tile
// ranges; only the forward at D=64 loses a wave per SIMD (4 -> 3) to them.
// The rows without SEG are those of the build before the segment mask.
// Occupancy is register-bound, not LDS-bound: at the stated waves/SIMD a CU
// holds 4 / 2 / 3 / 2 / 2 / 1 four-wave blocks, i.e. at most 110.6 KB
// (fwd D=64: 4 x 27648) of the 160 KB LDS.  dkdv at D=128 carries two
// [64, 128] fp32 accumulators plus the staging registers and runs at
// 1 wave/SIMD; trimming that is tuning, left to the follow-up.  A dkdv with a
// block per Q head writing bf16 partials, plus a reduce kernel over the GQA
// group, ran the whole backward in 46.5 ms where this in-kernel group loop
// takes 58.6 ms (B4 Hq32 Hkv8 S8192 D128 causal, profiles/fa16_helpers_ab.txt).
//
// Measured forward+backward on MI355X against
// F.scaled_dot_product_attention (profiles/fa_gen_vs_sdpa.txt; median of 30,
// min-max spread under 1% at the first shape):
//   B4 Hq32 Hkv8 S4160 D128 causal:  fa_gen 19.72 ms, SDPA 7.55 ms (2.61x slower)
//   B4 H12 S1000 D64 non-causal:     fa_gen 0.300 ms, SDPA 0.228 ms (1.32x slower)
// The general kernel loses at both: it buys shape coverage, the LSE output
// and O(S*D) saved state, not speed.
//
// Measured with segment ids (profiles/fa_gen_segments.txt; fa_gen_fwd +
// fa_gen_bwd, B4 Hq32 Hkv8 S8192 D128 causal, median of 12, three runs
// within 0.2%):
//   no ids 72.1 ms | ids that mask nothing 75.5 ms (+4.7%: the mask itself)
//   8 documents of 1024: 15.7 ms (0.218x; 0.132 of the tile pairs visible)
//   64 documents of 128: 3.08 ms (0.043x; 0.023 of the tile pairs visible)
// The time falls with the visible share, less than in proportion.  The
// cause was not isolated by measurement; the likely one is that a block
// with few tiles to visit no longer amortises its prologue and epilogue.
#include "fa16_common.h"

#include <climits>

// ---------------------------------------------------------------------------
// segment pre-pass   grid: (ceil(Sq/64) + ceil(Sk/64), B), one wave per tile
// bounds[b][tile] = (min, max) of the tile's segment ids, q tiles first
// (the layout fg_seg_bounds reads).  Tail rows are left out and never read;
// every tile has at least one row.
// ---------------------------------------------------------------------------
__global__ void __launch_bounds__(FG_BLK)
fa_gen_seg_bounds_kernel(const int* __restrict__ q_seg,
                         const int* __restrict__ kv_seg,
                         int* __restrict__ bounds, int Sq, int Sk) {
  const int nqt = fg_tiles(Sq);
  const int b = blockIdx.y;
  const bool is_q = (int)blockIdx.x < nqt;
  const int tile = is_q ? blockIdx.x : blockIdx.x - nqt;
  const int n = is_q ? Sq : Sk;
  const int* seg = is_q ? q_seg + (int64_t)b * Sq : kv_seg + (int64_t)b * Sk;
  const int row = tile * FG_BLK + threadIdx.x;
  int lo = INT_MAX, hi = INT_MIN;
  if (row < n) lo = hi = seg[row];
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) {
    lo = min(lo, __shfl_xor(lo, off, 64));
    hi = max(hi, __shfl_xor(hi, off, 64));
  }
  if (threadIdx.x == 0) {
    int* out = bounds + ((int64_t)b * gridDim.x + blockIdx.x) * 2;
    out[0] = lo;
    out[1] = hi;
  }
}

// ---------------------------------------------------------------------------
// forward   grid: (ceil(Sq/64), Hq, B)
// ---------------------------------------------------------------------------
template <int D, bool SEG>
__global__ void __launch_bounds__(FG_THREADS)
fa_gen_fwd_kernel(const unsigned short* __restrict__ q,
                  const unsigned short* __restrict__ k,
                  const unsigned short* __restrict__ v,
                  unsigned short* __restrict__ o,
                  float* __restrict__ lse,
                  int Hq, int Hkv, int Sq, int Sk, float scale_log2,
                  int causal, int shift,
                  const int* __restrict__ q_seg,
                  const int* __restrict__ kv_seg,
                  const int* __restrict__ seg_bounds) {
  constexpr int FG_LDD = D + FG_PAD;
  constexpr int KC = D / 32;    // contraction chunks over D
  constexpr int NF = D / 16;    // 16-col output blocks over D
  constexpr int NLD = D / 32;   // 8-elem chunks per thread per [64, D] tile
  __shared__ __attribute__((aligned(16))) unsigned short lk[FG_BLK * FG_LDD];     // K rows  [64][D+8]
  __shared__ __attribute__((aligned(16))) unsigned short lvt[D * FG_ROWS_N];      // V^T     [D][72]
  __shared__ __attribute__((aligned(16))) unsigned short lp[FG_BLK * FG_ROWS_N];  // P       [64][72]

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = tid >> 6;
  const int q0 = blockIdx.x * FG_BLK;
  const int h = blockIdx.y;
  const int b = blockIdx.z;
  const int hkv = h / (Hq / Hkv);

  const unsigned short* kh = k + ((int64_t)b * Hkv + hkv) * Sk * D;
  const unsigned short* vh = v + ((int64_t)b * Hkv + hkv) * Sk * D;

  fg_shortx8 qfrag[KC];
  fg_wave_frags<D>(qfrag, q + ((int64_t)b * Hq + h) * Sq * D, q0, Sq, wave, lane);

  fg_floatx4 acc[NF];
  fg_zero(acc);
  float m[4], l[4];   // running max (exp2 domain), per-lane partial row sum
#pragma unroll
  for (int r = 0; r < 4; ++r) { m[r] = -INFINITY; l[r] = 0.f; }

  const int trow = wave * 16 + 4 * (lane >> 4);   // tile row of acc[.][0]
  // SEG: ids of this lane's 4 query rows / 4 key columns, the q tile's id
  // range and this batch row's kv ids and kv tile ranges
  int qs[4] = {0, 0, 0, 0}, ks[4] = {0, 0, 0, 0};
  int qlo = 0, qhi = 0;
  const int* ksb = nullptr;
  const int* kb = nullptr;
  if constexpr (SEG) {
    const int* qb;
    fg_seg_bounds(seg_bounds, b, Sq, Sk, qb, kb);
    fg_seg_range(qb, blockIdx.x, qlo, qhi);
    ksb = kv_seg + (int64_t)b * Sk;
#pragma unroll
    for (int r = 0; r < 4; ++r) qs[r] = fg_seg(q_seg + (int64_t)b * Sq, q0 + trow + r, Sq);
  }
  const int n_tiles = fg_kv_tiles(q0, Sq, Sk, causal, shift);
  for (int jt = 0; jt < n_tiles; ++jt) {
    const int k0 = jt * FG_BLK;
    if constexpr (SEG) {
      // block-uniform: every wave skips the whole iteration, barriers included
      int klo, khi;
      fg_seg_range(kb, jt, klo, khi);
      if (!fg_seg_overlap(qlo, qhi, klo, khi)) continue;
#pragma unroll
      for (int f = 0; f < 4; ++f) ks[f] = fg_seg(ksb, k0 + f * 16 + (lane & 15), Sk);
    }
    fg_shortx8 regv[NLD];
    fg_stage<D>(kh, k0, Sk, lk, tid);
    fg_tile_load<D>(regv, vh, k0, Sk, tid);
    fg_tile_t<D>(regv, lvt, tid);
    __syncthreads();

    // S[q][kv] = Q . K^T
    fg_floatx4 s[4];
    fg_zero(s);
    fg_score<KC>(s, qfrag, lk, FG_LDD, lane);

    // mask + online softmax (exp2 domain)
    float mx[4] = {-INFINITY, -INFINITY, -INFINITY, -INFINITY};
#pragma unroll
    for (int f = 0; f < 4; ++f) {
      int col = k0 + f * 16 + (lane & 15);
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        float x = fg_vis<SEG>(q0 + trow + r, col, Sk, causal, shift, qs[r], ks[f])
                      ? s[f][r] * scale_log2 : -INFINITY;
        s[f][r] = x;
        mx[r] = fmaxf(mx[r], x);
      }
    }
    float alpha[4], ms[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
#pragma unroll
      for (int off = 8; off >= 1; off >>= 1)
        mx[r] = fmaxf(mx[r], __shfl_xor(mx[r], off, 64));
      float mn = fmaxf(m[r], mx[r]);
      ms[r] = (mn == -INFINITY) ? 0.f : mn;   // no (-inf) - (-inf)
      alpha[r] = exp2f(m[r] - ms[r]);
      m[r] = mn;
      l[r] *= alpha[r];
    }
#pragma unroll
    for (int f = 0; f < 4; ++f)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        float p = exp2f(s[f][r] - ms[r]);
        l[r] += p;
        lp[(trow + r) * FG_ROWS_N + f * 16 + (lane & 15)] = f32_to_bf16(p);
      }
#pragma unroll
    for (int f = 0; f < NF; ++f)
#pragma unroll
      for (int r = 0; r < 4; ++r) acc[f][r] *= alpha[r];
    __syncthreads();

    fg_accum<NF>(acc, lp, lvt, wave, lane);   // O += P . V
    __syncthreads();
  }

  float* lh = lse + ((int64_t)b * Hq + h) * Sq;
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    float lr = l[r];
#pragma unroll
    for (int off = 8; off >= 1; off >>= 1) lr += __shfl_xor(lr, off, 64);
    bool live = lr > 0.f;
    float inv = live ? 1.f / lr : 0.f;
#pragma unroll
    for (int f = 0; f < NF; ++f) acc[f][r] *= inv;
    int row = q0 + trow + r;
    if (row < Sq && (lane & 15) == 0)
      lh[row] = live ? (m[r] + log2f(lr)) * FG_LN2 : -INFINITY;
  }
  fg_store<D>(o + ((int64_t)b * Hq + h) * Sq * D, acc, q0 + trow, Sq, lane);
}

// ---------------------------------------------------------------------------
// backward 1) delta = rowsum(dO * O) - dlse   (dlse null: 0; dead row: delta 0)
// ---------------------------------------------------------------------------
template <int D>
__global__ void __launch_bounds__(256)
fa_gen_preprocess_kernel(const unsigned short* __restrict__ dout,
                         const unsigned short* __restrict__ o,
                         const float* __restrict__ lse,
                         const float* __restrict__ dlse,
                         float* __restrict__ delta, int64_t rows) {
  constexpr int LPR = D / 8;          // lanes per row, 8 elems each
  constexpr int RPB = 256 / LPR;      // rows per block per iteration
  const int sub = threadIdx.x % LPR;
  int64_t row = (int64_t)blockIdx.x * RPB + threadIdx.x / LPR;
  const int64_t stride = (int64_t)gridDim.x * RPB;
  for (; row < rows; row += stride) {
    fg_shortx8 a = *reinterpret_cast<const fg_shortx8*>(dout + row * D + sub * 8);
    fg_shortx8 c = *reinterpret_cast<const fg_shortx8*>(o + row * D + sub * 8);
    float s = 0.f;
#pragma unroll
    for (int j = 0; j < 8; ++j)
      s += bf16_to_f32((unsigned short)a[j]) * bf16_to_f32((unsigned short)c[j]);
#pragma unroll
    for (int off = LPR / 2; off >= 1; off >>= 1) s += __shfl_xor(s, off, 64);
    if (sub == 0) {
      // dead row: delta = 0 whatever dO and dlse hold there
      bool live = lse[row] > -INFINITY;
      float d = (live && dlse != nullptr) ? dlse[row] : 0.f;
      delta[row] = live ? s - d : 0.f;
    }
  }
}

// ---------------------------------------------------------------------------
// backward 2) dK/dV   grid: (ceil(Sk/64), Hkv, B); loops the GQA group
// ---------------------------------------------------------------------------
template <int D, bool SEG>
__global__ void __launch_bounds__(FG_THREADS)
fa_gen_dkdv_kernel(const unsigned short* __restrict__ q,
                   const unsigned short* __restrict__ k,
                   const unsigned short* __restrict__ v,
                   const unsigned short* __restrict__ dout,
                   const float* __restrict__ lse,
                   const float* __restrict__ delta,
                   unsigned short* __restrict__ dk,
                   unsigned short* __restrict__ dv,
                   int Hq, int Hkv, int Sq, int Sk, float scale,
                   int causal, int shift,
                   const int* __restrict__ q_seg,
                   const int* __restrict__ kv_seg,
                   const int* __restrict__ seg_bounds) {
  constexpr int FG_LDD = D + FG_PAD;
  constexpr int KC = D / 32;
  constexpr int NF = D / 16;
  constexpr int NLD = D / 32;
  // each q-tile buffer lives twice per iteration: rows [64][D+8] for the
  // S^T / dP^T GEMMs, then rewritten transposed [D][72] from the staging
  // registers for the dV / dK GEMMs
  constexpr int LQ = (D * FG_ROWS_N > FG_BLK * FG_LDD) ? D * FG_ROWS_N : FG_BLK * FG_LDD;
  __shared__ __attribute__((aligned(16))) unsigned short lq[LQ];
  __shared__ __attribute__((aligned(16))) unsigned short ldo[LQ];
  __shared__ __attribute__((aligned(16))) unsigned short lpt[FG_BLK * FG_ROWS_N];   // P^T  [64kv][72]
  __shared__ __attribute__((aligned(16))) unsigned short ldst[FG_BLK * FG_ROWS_N];  // dS^T [64kv][72]
  __shared__ float lse_s[FG_BLK];   // lse * log2e; +inf on dead / tail rows
  __shared__ float dlt_s[FG_BLK];

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = tid >> 6;
  const int k0 = blockIdx.x * FG_BLK;
  const int hkv = blockIdx.y;
  const int b = blockIdx.z;
  const int group = Hq / Hkv;
  const float scale_log2 = scale * FG_LOG2E;
  const int64_t kvoff = ((int64_t)b * Hkv + hkv) * Sk * D;

  fg_shortx8 kfrag[KC], vfrag[KC];
  fg_wave_frags<D>(kfrag, k + kvoff, k0, Sk, wave, lane);
  fg_wave_frags<D>(vfrag, v + kvoff, k0, Sk, wave, lane);

  fg_floatx4 accK[NF], accV[NF];
  fg_zero(accK);
  fg_zero(accV);

  const int trow = wave * 16 + 4 * (lane >> 4);   // kv tile row of acc[.][0]
  const int n_qtiles = (Sq + FG_BLK - 1) / FG_BLK;
  // first q row that sees key k0: i >= k0 - shift
  const int iq_start = (causal && k0 - shift > 0) ? (k0 - shift) / FG_BLK : 0;

  // SEG: ids of this lane's 4 key rows / 4 query columns, the kv tile's id
  // range and this batch row's q ids and q tile ranges
  int ks[4] = {0, 0, 0, 0}, qs[4] = {0, 0, 0, 0};
  int klo = 0, khi = 0;
  const int* qsb = nullptr;
  const int* qb = nullptr;
  if constexpr (SEG) {
    const int* kb;
    fg_seg_bounds(seg_bounds, b, Sq, Sk, qb, kb);
    fg_seg_range(kb, blockIdx.x, klo, khi);
    qsb = q_seg + (int64_t)b * Sq;
#pragma unroll
    for (int r = 0; r < 4; ++r) ks[r] = fg_seg(kv_seg + (int64_t)b * Sk, k0 + trow + r, Sk);
  }

  for (int g = 0; g < group; ++g) {
    const int h = hkv * group + g;
    const unsigned short* qh = q + ((int64_t)b * Hq + h) * Sq * D;
    const unsigned short* doh = dout + ((int64_t)b * Hq + h) * Sq * D;
    const float* lh = lse + ((int64_t)b * Hq + h) * Sq;
    const float* dh = delta + ((int64_t)b * Hq + h) * Sq;

    for (int iq = iq_start; iq < n_qtiles; ++iq) {
      const int q0 = iq * FG_BLK;
      if constexpr (SEG) {
        // block-uniform: every wave skips the whole iteration, barriers included
        int qlo, qhi;
        fg_seg_range(qb, iq, qlo, qhi);
        if (!fg_seg_overlap(qlo, qhi, klo, khi)) continue;
#pragma unroll
        for (int f = 0; f < 4; ++f) qs[f] = fg_seg(qsb, q0 + f * 16 + (lane & 15), Sq);
      }
      fg_shortx8 regq[NLD], regdo[NLD];
      fg_stage<D>(regq, qh, q0, Sq, lq, tid);
      fg_stage<D>(regdo, doh, q0, Sq, ldo, tid);
      if (tid < FG_BLK) fg_lse_delta(lh, dh, q0 + tid, Sq, lse_s[tid], dlt_s[tid]);
      __syncthreads();

      // ST[kv][q] = K . Q^T; dPT[kv][q] = V . dO^T
      fg_floatx4 st[4], dpt[4];
      fg_zero(st);
      fg_zero(dpt);
      fg_score<KC>(st, kfrag, lq, FG_LDD, lane);
      fg_score<KC>(dpt, vfrag, ldo, FG_LDD, lane);
      __syncthreads();   // row layouts consumed before the rewrite

      // P^T = exp2(ST*scale*log2e - lse*log2e); dS^T = P^T (dPT - delta) scale
#pragma unroll
      for (int f = 0; f < 4; ++f) {
        int qc = f * 16 + (lane & 15);
        float l2 = lse_s[qc];
        float dl = dlt_s[qc];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          bool vis = fg_vis<SEG>(q0 + qc, k0 + trow + r, Sk, causal, shift, qs[f], ks[r]);
          float p = fg_p(vis, st[f][r], scale_log2, l2);
          lpt[(trow + r) * FG_ROWS_N + qc] = f32_to_bf16(p);
          ldst[(trow + r) * FG_ROWS_N + qc] = f32_to_bf16(fg_ds(p, dpt[f][r], dl, scale));
        }
      }
      fg_tile_t<D>(regq, lq, tid);
      fg_tile_t<D>(regdo, ldo, tid);
      __syncthreads();

      fg_accum<NF>(accV, lpt, ldo, wave, lane);    // dV += P^T . dO
      fg_accum<NF>(accK, ldst, lq, wave, lane);    // dK += dS^T . Q
      __syncthreads();
    }
  }

  fg_store<D>(dk + kvoff, accK, k0 + trow, Sk, lane);
  fg_store<D>(dv + kvoff, accV, k0 + trow, Sk, lane);
}

// ---------------------------------------------------------------------------
// backward 3) dQ   grid: (ceil(Sq/64), Hq, B)
// ---------------------------------------------------------------------------
template <int D, bool SEG>
__global__ void __launch_bounds__(FG_THREADS)
fa_gen_dq_kernel(const unsigned short* __restrict__ q,
                 const unsigned short* __restrict__ k,
                 const unsigned short* __restrict__ v,
                 const unsigned short* __restrict__ dout,
                 const float* __restrict__ lse,
                 const float* __restrict__ delta,
                 unsigned short* __restrict__ dq,
                 int Hq, int Hkv, int Sq, int Sk, float scale,
                 int causal, int shift,
                 const int* __restrict__ q_seg,
                 const int* __restrict__ kv_seg,
                 const int* __restrict__ seg_bounds) {
  constexpr int FG_LDD = D + FG_PAD;
  constexpr int KC = D / 32;
  constexpr int NF = D / 16;
  constexpr int NLD = D / 32;
  constexpr int LK = (D * FG_ROWS_N > FG_BLK * FG_LDD) ? D * FG_ROWS_N : FG_BLK * FG_LDD;
  __shared__ __attribute__((aligned(16))) unsigned short lk[LK];                   // K rows -> K^T
  __shared__ __attribute__((aligned(16))) unsigned short lv[FG_BLK * FG_LDD];      // V rows [64][D+8]
  __shared__ __attribute__((aligned(16))) unsigned short lds_s[FG_BLK * FG_ROWS_N];// dS [64q][72]

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = tid >> 6;
  const int q0 = blockIdx.x * FG_BLK;
  const int h = blockIdx.y;
  const int b = blockIdx.z;
  const int hkv = h / (Hq / Hkv);
  const float scale_log2 = scale * FG_LOG2E;
  const int64_t loff = ((int64_t)b * Hq + h) * Sq;   // this head in lse / delta
  const int64_t qoff = loff * D;                     // ... and in q, dO, dq

  const unsigned short* kh = k + ((int64_t)b * Hkv + hkv) * Sk * D;
  const unsigned short* vh = v + ((int64_t)b * Hkv + hkv) * Sk * D;

  fg_shortx8 qfrag[KC], dofrag[KC];
  fg_wave_frags<D>(qfrag, q + qoff, q0, Sq, wave, lane);
  fg_wave_frags<D>(dofrag, dout + qoff, q0, Sq, wave, lane);
  const int trow = wave * 16 + 4 * (lane >> 4);
  float l2_r[4], dlt_r[4];   // lse * log2e (+inf on dead / tail rows), delta
#pragma unroll
  for (int r = 0; r < 4; ++r)
    fg_lse_delta(lse + loff, delta + loff, q0 + trow + r, Sq, l2_r[r], dlt_r[r]);

  fg_floatx4 accQ[NF];
  fg_zero(accQ);

  // SEG: as in the forward
  int qs[4] = {0, 0, 0, 0}, ks[4] = {0, 0, 0, 0};
  int qlo = 0, qhi = 0;
  const int* ksb = nullptr;
  const int* kb = nullptr;
  if constexpr (SEG) {
    const int* qb;
    fg_seg_bounds(seg_bounds, b, Sq, Sk, qb, kb);
    fg_seg_range(qb, blockIdx.x, qlo, qhi);
    ksb = kv_seg + (int64_t)b * Sk;
#pragma unroll
    for (int r = 0; r < 4; ++r) qs[r] = fg_seg(q_seg + (int64_t)b * Sq, q0 + trow + r, Sq);
  }
  const int n_tiles = fg_kv_tiles(q0, Sq, Sk, causal, shift);
  for (int jt = 0; jt < n_tiles; ++jt) {
    const int k0 = jt * FG_BLK;
    if constexpr (SEG) {
      // block-uniform: every wave skips the whole iteration, barriers included
      int klo, khi;
      fg_seg_range(kb, jt, klo, khi);
      if (!fg_seg_overlap(qlo, qhi, klo, khi)) continue;
#pragma unroll
      for (int f = 0; f < 4; ++f) ks[f] = fg_seg(ksb, k0 + f * 16 + (lane & 15), Sk);
    }
    fg_shortx8 regk[NLD];
    fg_stage<D>(regk, kh, k0, Sk, lk, tid);
    fg_stage<D>(vh, k0, Sk, lv, tid);
    __syncthreads();

    // S[q][kv] = Q . K^T; dP[q][kv] = dO . V^T
    fg_floatx4 s[4], dp[4];
    fg_zero(s);
    fg_zero(dp);
    fg_score<KC>(s, qfrag, lk, FG_LDD, lane);
    fg_score<KC>(dp, dofrag, lv, FG_LDD, lane);
    __syncthreads();   // K rows consumed; lk may be rewritten transposed

    // dS[q][kv] = P (dP - delta) scale
#pragma unroll
    for (int f = 0; f < 4; ++f) {
      int col = k0 + f * 16 + (lane & 15);
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        bool vis = fg_vis<SEG>(q0 + trow + r, col, Sk, causal, shift, qs[r], ks[f]);
        float p = fg_p(vis, s[f][r], scale_log2, l2_r[r]);
        lds_s[(trow + r) * FG_ROWS_N + f * 16 + (lane & 15)] =
            f32_to_bf16(fg_ds(p, dp[f][r], dlt_r[r], scale));
      }
    }
    fg_tile_t<D>(regk, lk, tid);
    __syncthreads();

    fg_accum<NF>(accQ, lds_s, lk, wave, lane);   // dQ += dS . K
    __syncthreads();
  }

  fg_store<D>(dq + qoff, accQ, q0 + trow, Sq, lane);
}
