// General-shape flash attention, forward + backward, with a differentiable
// log-sum-exp output — the correctness-first companion of the tuned D=128
// kernels (attention_fwd.hip / attention_bwd2.hip).
//
// Same skeleton as attention_bwd.hip: 64-row tiles, 4 waves (wave w owns
// rows [16w, 16w+16) of the tile), mfma_f32_16x16x32_bf16 in TN form
// (C[i][j] = sum_k X[i][k] * Y[j][k], operand fragment row = lane&15,
// k-chunk = lane>>4; D-layout col = lane&15, row = 4*(lane>>4)+r),
// __syncthreads-staged, +8-elem LDS row pad.  Templated on D in {64, 128};
// everything else is a runtime argument.
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
// Tails: rows >= Sq / >= Sk are never loaded (every global load is
// predicated on its row) and never stored; staging zero-fills them, and the
// mask gives their scores no weight.
//
// Dead rows (no visible key): o = 0 and lse = -inf exactly; in backward they
// contribute exactly zero (their P and dS are selected to 0, never computed
// as exp(-inf - -inf) or 0/0), and dlse is taken as 0 on them.
//
// Backward is the standard split plus the LSE gradient:
//   fa_gen_preprocess: delta[row] = rowsum(dO*O) - dlse[row] (0 on dead rows)
//   fa_gen_dkdv:       per KV tile, loops the GQA group in-kernel (fp32
//                      accumulation across the group, no partial buffers)
//   fa_gen_dq:         per Q tile
// No atomics anywhere: repeated calls are bitwise equal.
//
// Build report (hipcc -O3 --offload-arch=gfx950,
// -Rpass-analysis=kernel-resource-usage): no scratch (0 B/lane) and no
// SGPR/VGPR spills in any instantiation.
//   kernel       D    VGPRs  AGPRs  LDS B/block  waves/SIMD (compiler)
//   fa_gen_fwd   64   108    16     27648        4
//   fa_gen_fwd   128  154    32     45056        2
//   fa_gen_dq    64   106    36     27648        3
//   fa_gen_dq    128  150    64     45056        2
//   fa_gen_dkdv  64   137    52     37376        2
//   fa_gen_dkdv  128  221    96     55808        1
// Occupancy is register-bound, not LDS-bound: at the stated waves/SIMD a CU
// holds 4 / 2 / 3 / 2 / 2 / 1 four-wave blocks, i.e. at most 110.6 KB
// (fwd D=64: 4 x 27648) of the 160 KB LDS.  dkdv at D=128 carries two
// [64, 128] fp32 accumulators plus the staging registers and runs at
// 1 wave/SIMD; trimming that is tuning, left to the follow-up.
//
// Measured forward+backward on MI355X against
// F.scaled_dot_product_attention (profiles/fa_gen_vs_sdpa.txt; median of 30,
// min-max spread under 1% at the first shape):
//   B4 Hq32 Hkv8 S4160 D128 causal:  fa_gen 20.20 ms, SDPA 7.69 ms (2.63x slower)
//   B4 H12 S1000 D64 non-causal:     fa_gen 0.296 ms, SDPA 0.222 ms (1.33x slower)
// The general kernel loses at both: it buys shape coverage, the LSE output
// and O(S*D) saved state, not speed.
#include "common.h"

#define FG_BLK 64              // tile rows (q and kv tiles)
#define FG_THREADS 256         // 4 waves
#define FG_PAD 8               // LDS row pad (elems)
#define FG_ROWS_N (FG_BLK + FG_PAD)
#define FG_LOG2E 1.4426950408889634f
#define FG_LN2 0.6931471805599453f

typedef float fg_floatx4 __attribute__((ext_vector_type(4)));
typedef short fg_shortx8 __attribute__((ext_vector_type(8)));

// 8-elem chunk of row `row` of a [nrows, D] head; zero (and no load) past
// the end
template <int D>
DEV fg_shortx8 fg_ld8(const unsigned short* head, int row, int nrows, int col) {
  fg_shortx8 z = {0, 0, 0, 0, 0, 0, 0, 0};
  if (row < nrows)
    z = *reinterpret_cast<const fg_shortx8*>(head + (int64_t)row * D + col);
  return z;
}

// operand fragment read (row-major LDS tile, row stride `stride` elems;
// rf = 16-row block, kc = 32-elem contraction chunk)
DEV fg_shortx8 fg_frag(const unsigned short* t, int stride, int rf, int kc, int lane) {
  int row = rf * 16 + (lane & 15);
  int col = kc * 32 + (lane >> 4) * 8;
  return *reinterpret_cast<const fg_shortx8*>(t + row * stride + col);
}

// number of 64-row KV tiles a q tile starting at q0 has to visit
DEV int fg_kv_tiles(int q0, int Sq, int Sk, int causal, int shift) {
  int kv_end = Sk;
  if (causal) {
    int qmax = min(q0 + FG_BLK - 1, Sq - 1);
    kv_end = min(Sk, qmax + shift + 1);
  }
  return kv_end > 0 ? (kv_end + FG_BLK - 1) / FG_BLK : 0;
}

// ---------------------------------------------------------------------------
// forward   grid: (ceil(Sq/64), Hq, B)
// ---------------------------------------------------------------------------
template <int D>
__global__ void __launch_bounds__(FG_THREADS)
fa_gen_fwd_kernel(const unsigned short* __restrict__ q,
                  const unsigned short* __restrict__ k,
                  const unsigned short* __restrict__ v,
                  unsigned short* __restrict__ o,
                  float* __restrict__ lse,
                  int Hq, int Hkv, int Sq, int Sk, float scale_log2,
                  int causal, int shift) {
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

  const unsigned short* qh = q + ((int64_t)b * Hq + h) * Sq * D;
  const unsigned short* kh = k + ((int64_t)b * Hkv + hkv) * Sk * D;
  const unsigned short* vh = v + ((int64_t)b * Hkv + hkv) * Sk * D;

  fg_shortx8 qfrag[KC];
#pragma unroll
  for (int kc = 0; kc < KC; ++kc)
    qfrag[kc] = fg_ld8<D>(qh, q0 + wave * 16 + (lane & 15), Sq,
                          kc * 32 + (lane >> 4) * 8);

  fg_floatx4 acc[NF];
#pragma unroll
  for (int f = 0; f < NF; ++f) acc[f] = (fg_floatx4){0.f, 0.f, 0.f, 0.f};
  float m[4], l[4];   // running max (exp2 domain), per-lane partial row sum
#pragma unroll
  for (int r = 0; r < 4; ++r) { m[r] = -INFINITY; l[r] = 0.f; }

  const int trow = wave * 16 + 4 * (lane >> 4);   // tile row of acc[.][0]
  const int n_tiles = fg_kv_tiles(q0, Sq, Sk, causal, shift);
  for (int jt = 0; jt < n_tiles; ++jt) {
    const int k0 = jt * FG_BLK;
#pragma unroll
    for (int j = 0; j < NLD; ++j) {
      int e = (tid + j * FG_THREADS) * 8;
      int r = e / D, c = e % D;
      *reinterpret_cast<fg_shortx8*>(lk + r * FG_LDD + c) = fg_ld8<D>(kh, k0 + r, Sk, c);
      fg_shortx8 vv = fg_ld8<D>(vh, k0 + r, Sk, c);
#pragma unroll
      for (int x = 0; x < 8; ++x) lvt[(c + x) * FG_ROWS_N + r] = (unsigned short)vv[x];
    }
    __syncthreads();

    // S[q][kv] = Q . K^T
    fg_floatx4 s[4];
#pragma unroll
    for (int f = 0; f < 4; ++f) s[f] = (fg_floatx4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int kc = 0; kc < KC; ++kc)
#pragma unroll
      for (int f = 0; f < 4; ++f)
        s[f] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
            qfrag[kc], fg_frag(lk, FG_LDD, f, kc, lane), s[f], 0, 0, 0);

    // mask + online softmax (exp2 domain)
    float mx[4] = {-INFINITY, -INFINITY, -INFINITY, -INFINITY};
#pragma unroll
    for (int f = 0; f < 4; ++f) {
      int col = k0 + f * 16 + (lane & 15);
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        bool vis = col < Sk && (!causal || col <= q0 + trow + r + shift);
        float x = vis ? s[f][r] * scale_log2 : -INFINITY;
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

    // O += P . V   (Y = V^T)
#pragma unroll
    for (int kc = 0; kc < 2; ++kc) {
      fg_shortx8 xp = fg_frag(lp, FG_ROWS_N, wave, kc, lane);
#pragma unroll
      for (int f = 0; f < NF; ++f)
        acc[f] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
            xp, fg_frag(lvt, FG_ROWS_N, f, kc, lane), acc[f], 0, 0, 0);
    }
    __syncthreads();
  }

  unsigned short* oh = o + ((int64_t)b * Hq + h) * Sq * D;
  float* lh = lse + ((int64_t)b * Hq + h) * Sq;
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    float lr = l[r];
#pragma unroll
    for (int off = 8; off >= 1; off >>= 1) lr += __shfl_xor(lr, off, 64);
    int row = q0 + trow + r;
    if (row < Sq) {
      bool live = lr > 0.f;
      float inv = live ? 1.f / lr : 0.f;
#pragma unroll
      for (int f = 0; f < NF; ++f)
        oh[(int64_t)row * D + f * 16 + (lane & 15)] = f32_to_bf16(acc[f][r] * inv);
      if ((lane & 15) == 0)
        lh[row] = live ? (m[r] + log2f(lr)) * FG_LN2 : -INFINITY;
    }
  }
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
template <int D>
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
                   int causal, int shift) {
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

  const unsigned short* kh = k + ((int64_t)b * Hkv + hkv) * Sk * D;
  const unsigned short* vh = v + ((int64_t)b * Hkv + hkv) * Sk * D;

  fg_shortx8 kfrag[KC], vfrag[KC];
#pragma unroll
  for (int kc = 0; kc < KC; ++kc) {
    int row = k0 + wave * 16 + (lane & 15);
    int col = kc * 32 + (lane >> 4) * 8;
    kfrag[kc] = fg_ld8<D>(kh, row, Sk, col);
    vfrag[kc] = fg_ld8<D>(vh, row, Sk, col);
  }

  fg_floatx4 accK[NF], accV[NF];
#pragma unroll
  for (int f = 0; f < NF; ++f) {
    accK[f] = (fg_floatx4){0.f, 0.f, 0.f, 0.f};
    accV[f] = (fg_floatx4){0.f, 0.f, 0.f, 0.f};
  }

  const int trow = wave * 16 + 4 * (lane >> 4);   // kv tile row of acc[.][0]
  const int n_qtiles = (Sq + FG_BLK - 1) / FG_BLK;
  // first q row that sees key k0: i >= k0 - shift
  const int iq_start = (causal && k0 - shift > 0) ? (k0 - shift) / FG_BLK : 0;

  for (int g = 0; g < group; ++g) {
    const int h = hkv * group + g;
    const unsigned short* qh = q + ((int64_t)b * Hq + h) * Sq * D;
    const unsigned short* doh = dout + ((int64_t)b * Hq + h) * Sq * D;
    const float* lh = lse + ((int64_t)b * Hq + h) * Sq;
    const float* dh = delta + ((int64_t)b * Hq + h) * Sq;

    for (int iq = iq_start; iq < n_qtiles; ++iq) {
      const int q0 = iq * FG_BLK;
      fg_shortx8 regq[NLD], regdo[NLD];
#pragma unroll
      for (int j = 0; j < NLD; ++j) {
        int e = (tid + j * FG_THREADS) * 8;
        int r = e / D, c = e % D;
        regq[j] = fg_ld8<D>(qh, q0 + r, Sq, c);
        regdo[j] = fg_ld8<D>(doh, q0 + r, Sq, c);
        *reinterpret_cast<fg_shortx8*>(lq + r * FG_LDD + c) = regq[j];
        *reinterpret_cast<fg_shortx8*>(ldo + r * FG_LDD + c) = regdo[j];
      }
      if (tid < FG_BLK) {
        float l2 = INFINITY, dl = 0.f;
        if (q0 + tid < Sq) {
          float lv = lh[q0 + tid];
          if (lv > -INFINITY) l2 = lv * FG_LOG2E;
          dl = dh[q0 + tid];
        }
        lse_s[tid] = l2;
        dlt_s[tid] = dl;
      }
      __syncthreads();

      // ST[kv][q] = K . Q^T; dPT[kv][q] = V . dO^T
      fg_floatx4 st[4], dpt[4];
#pragma unroll
      for (int f = 0; f < 4; ++f) {
        st[f] = (fg_floatx4){0.f, 0.f, 0.f, 0.f};
        dpt[f] = (fg_floatx4){0.f, 0.f, 0.f, 0.f};
      }
#pragma unroll
      for (int kc = 0; kc < KC; ++kc)
#pragma unroll
        for (int f = 0; f < 4; ++f) {
          st[f] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
              kfrag[kc], fg_frag(lq, FG_LDD, f, kc, lane), st[f], 0, 0, 0);
          dpt[f] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
              vfrag[kc], fg_frag(ldo, FG_LDD, f, kc, lane), dpt[f], 0, 0, 0);
        }
      __syncthreads();   // row layouts consumed before the rewrite

      // P^T = exp2(ST*scale*log2e - lse*log2e); dS^T = P^T (dPT - delta) scale
#pragma unroll
      for (int f = 0; f < 4; ++f) {
        int qc = f * 16 + (lane & 15);
        float l2 = lse_s[qc];
        float dl = dlt_s[qc];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          int kvrow = k0 + trow + r;
          bool vis = kvrow < Sk && (!causal || kvrow <= q0 + qc + shift);
          float p = vis ? exp2f(st[f][r] * scale_log2 - l2) : 0.f;
          float ds = (p > 0.f) ? p * (dpt[f][r] - dl) * scale : 0.f;
          lpt[(trow + r) * FG_ROWS_N + qc] = f32_to_bf16(p);
          ldst[(trow + r) * FG_ROWS_N + qc] = f32_to_bf16(ds);
        }
      }
#pragma unroll
      for (int j = 0; j < NLD; ++j) {
        int e = (tid + j * FG_THREADS) * 8;
        int r = e / D, c = e % D;
#pragma unroll
        for (int x = 0; x < 8; ++x) {
          lq[(c + x) * FG_ROWS_N + r] = (unsigned short)regq[j][x];
          ldo[(c + x) * FG_ROWS_N + r] = (unsigned short)regdo[j][x];
        }
      }
      __syncthreads();

      // dV += P^T . dO (Y = dO^T); dK += dS^T . Q (Y = Q^T)
#pragma unroll
      for (int kc = 0; kc < 2; ++kc) {
        fg_shortx8 xp = fg_frag(lpt, FG_ROWS_N, wave, kc, lane);
        fg_shortx8 xs = fg_frag(ldst, FG_ROWS_N, wave, kc, lane);
#pragma unroll
        for (int f = 0; f < NF; ++f) {
          accV[f] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
              xp, fg_frag(ldo, FG_ROWS_N, f, kc, lane), accV[f], 0, 0, 0);
          accK[f] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
              xs, fg_frag(lq, FG_ROWS_N, f, kc, lane), accK[f], 0, 0, 0);
        }
      }
      __syncthreads();
    }
  }

  unsigned short* dkh = dk + ((int64_t)b * Hkv + hkv) * Sk * D;
  unsigned short* dvh = dv + ((int64_t)b * Hkv + hkv) * Sk * D;
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    int row = k0 + trow + r;
    if (row < Sk) {
#pragma unroll
      for (int f = 0; f < NF; ++f) {
        int col = f * 16 + (lane & 15);
        dkh[(int64_t)row * D + col] = f32_to_bf16(accK[f][r]);
        dvh[(int64_t)row * D + col] = f32_to_bf16(accV[f][r]);
      }
    }
  }
}

// ---------------------------------------------------------------------------
// backward 3) dQ   grid: (ceil(Sq/64), Hq, B)
// ---------------------------------------------------------------------------
template <int D>
__global__ void __launch_bounds__(FG_THREADS)
fa_gen_dq_kernel(const unsigned short* __restrict__ q,
                 const unsigned short* __restrict__ k,
                 const unsigned short* __restrict__ v,
                 const unsigned short* __restrict__ dout,
                 const float* __restrict__ lse,
                 const float* __restrict__ delta,
                 unsigned short* __restrict__ dq,
                 int Hq, int Hkv, int Sq, int Sk, float scale,
                 int causal, int shift) {
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

  const unsigned short* qh = q + ((int64_t)b * Hq + h) * Sq * D;
  const unsigned short* doh = dout + ((int64_t)b * Hq + h) * Sq * D;
  const unsigned short* kh = k + ((int64_t)b * Hkv + hkv) * Sk * D;
  const unsigned short* vh = v + ((int64_t)b * Hkv + hkv) * Sk * D;
  const float* lh = lse + ((int64_t)b * Hq + h) * Sq;
  const float* dh = delta + ((int64_t)b * Hq + h) * Sq;

  fg_shortx8 qfrag[KC], dofrag[KC];
#pragma unroll
  for (int kc = 0; kc < KC; ++kc) {
    int row = q0 + wave * 16 + (lane & 15);
    int col = kc * 32 + (lane >> 4) * 8;
    qfrag[kc] = fg_ld8<D>(qh, row, Sq, col);
    dofrag[kc] = fg_ld8<D>(doh, row, Sq, col);
  }
  const int trow = wave * 16 + 4 * (lane >> 4);
  float l2_r[4], dlt_r[4];   // lse * log2e (+inf on dead / tail rows), delta
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    int row = q0 + trow + r;
    l2_r[r] = INFINITY;
    dlt_r[r] = 0.f;
    if (row < Sq) {
      float lv_ = lh[row];
      if (lv_ > -INFINITY) l2_r[r] = lv_ * FG_LOG2E;
      dlt_r[r] = dh[row];
    }
  }

  fg_floatx4 accQ[NF];
#pragma unroll
  for (int f = 0; f < NF; ++f) accQ[f] = (fg_floatx4){0.f, 0.f, 0.f, 0.f};

  const int n_tiles = fg_kv_tiles(q0, Sq, Sk, causal, shift);
  for (int jt = 0; jt < n_tiles; ++jt) {
    const int k0 = jt * FG_BLK;
    fg_shortx8 regk[NLD];
#pragma unroll
    for (int j = 0; j < NLD; ++j) {
      int e = (tid + j * FG_THREADS) * 8;
      int r = e / D, c = e % D;
      regk[j] = fg_ld8<D>(kh, k0 + r, Sk, c);
      *reinterpret_cast<fg_shortx8*>(lk + r * FG_LDD + c) = regk[j];
      *reinterpret_cast<fg_shortx8*>(lv + r * FG_LDD + c) = fg_ld8<D>(vh, k0 + r, Sk, c);
    }
    __syncthreads();

    // S[q][kv] = Q . K^T; dP[q][kv] = dO . V^T
    fg_floatx4 s[4], dp[4];
#pragma unroll
    for (int f = 0; f < 4; ++f) {
      s[f] = (fg_floatx4){0.f, 0.f, 0.f, 0.f};
      dp[f] = (fg_floatx4){0.f, 0.f, 0.f, 0.f};
    }
#pragma unroll
    for (int kc = 0; kc < KC; ++kc)
#pragma unroll
      for (int f = 0; f < 4; ++f) {
        s[f] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
            qfrag[kc], fg_frag(lk, FG_LDD, f, kc, lane), s[f], 0, 0, 0);
        dp[f] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
            dofrag[kc], fg_frag(lv, FG_LDD, f, kc, lane), dp[f], 0, 0, 0);
      }
    __syncthreads();   // K rows consumed; lk may be rewritten transposed

    // dS[q][kv] = P (dP - delta) scale
#pragma unroll
    for (int f = 0; f < 4; ++f) {
      int col = k0 + f * 16 + (lane & 15);
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        bool vis = col < Sk && (!causal || col <= q0 + trow + r + shift);
        float p = vis ? exp2f(s[f][r] * scale_log2 - l2_r[r]) : 0.f;
        float ds = (p > 0.f) ? p * (dp[f][r] - dlt_r[r]) * scale : 0.f;
        lds_s[(trow + r) * FG_ROWS_N + f * 16 + (lane & 15)] = f32_to_bf16(ds);
      }
    }
#pragma unroll
    for (int j = 0; j < NLD; ++j) {
      int e = (tid + j * FG_THREADS) * 8;
      int r = e / D, c = e % D;
#pragma unroll
      for (int x = 0; x < 8; ++x) lk[(c + x) * FG_ROWS_N + r] = (unsigned short)regk[j][x];
    }
    __syncthreads();

    // dQ += dS . K (Y = K^T)
#pragma unroll
    for (int kc = 0; kc < 2; ++kc) {
      fg_shortx8 xs = fg_frag(lds_s, FG_ROWS_N, wave, kc, lane);
#pragma unroll
      for (int f = 0; f < NF; ++f)
        accQ[f] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
            xs, fg_frag(lk, FG_ROWS_N, f, kc, lane), accQ[f], 0, 0, 0);
    }
    __syncthreads();
  }

  unsigned short* dqh = dq + ((int64_t)b * Hq + h) * Sq * D;
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    int row = q0 + trow + r;
    if (row < Sq) {
#pragma unroll
      for (int f = 0; f < NF; ++f)
        dqh[(int64_t)row * D + f * 16 + (lane & 15)] = f32_to_bf16(accQ[f][r]);
    }
  }
}
