// Fused cross-entropy over a large vocab — CDNA4.
//
// Replaces log_softmax + nll (reference: vocab-parallel CE at
// legacy/vescale/model/patch/vp_cross_entropy.py:43-147 is the sharded
// variant; this is the dense fast path).  One 256-thread block per row,
// single pass max+sumexp (online), bf16x8 loads.  Backward recomputes
// softmax from the saved logsumexp and can write grads IN-PLACE over the
// logits buffer (a [tokens, 128k] bf16 tensor is GBs — avoid a second one).
// The sharded variant's kernels (ce_vp_fwd_bf16 / ce_vp_bwd_bf16) follow the
// dense pair below.
#include "common.h"

#define BLOCK 256

// a row of all -inf (or an idle thread) must not turn exp(-inf - -inf) into NaN
DEV float ce_finite_max(float m) { return m == -INFINITY ? 0.f : m; }

// logits: [N, V] bf16; target: [N] int64; loss/lse: [N] f32
extern "C" __global__ void __launch_bounds__(BLOCK)
ce_fwd_bf16(const unsigned short* __restrict__ logits,
            const int64_t* __restrict__ target,
            float* __restrict__ loss, float* __restrict__ lse_out,
            int64_t n_rows, int vocab, int64_t ignore_index) {
  __shared__ float lds[BLOCK / WAVE];
  const int vec = 8;
  const int iters = (vocab / vec + BLOCK - 1) / BLOCK;
  for (int64_t row = blockIdx.x; row < n_rows; row += gridDim.x) {
    const unsigned short* xr = logits + row * vocab;
    int64_t tgt = target[row];
    // online max + sumexp in one pass
    float mx = -INFINITY, sum = 0.f;
    for (int it = 0; it < iters; ++it) {
      int i = (it * BLOCK + threadIdx.x) * vec;
      if (i < vocab) {
        short8v v = *reinterpret_cast<const short8v*>(xr + i);
#pragma unroll
        for (int j = 0; j < vec; ++j) {
          int col = i + j;
          float f = (col < vocab) ? bf16_to_f32((unsigned short)v[j]) : -INFINITY;
          float m2 = fmaxf(mx, f);
          // -inf logits (masked classes) while mx is still -inf: shift by 0,
          // not by -inf (exp(-inf - -inf) is NaN); bitwise the same otherwise
          float ms = ce_finite_max(m2);
          sum = sum * __expf(mx - ms) + ((col < vocab) ? __expf(f - ms) : 0.f);
          mx = m2;
        }
      }
    }
    // block combine (max then rescaled sums)
    float gmax = block_reduce_max<BLOCK>(mx, lds);
    float gsum = block_reduce_sum<BLOCK>(sum * __expf(mx - ce_finite_max(gmax)), lds);
    float lse = gmax + __logf(gsum);
    if (threadIdx.x == 0) {
      if (tgt == ignore_index) {
        loss[row] = 0.f;
        lse_out[row] = lse;
      } else {
        float xt = bf16_to_f32(xr[tgt]);
        loss[row] = lse - xt;
        lse_out[row] = lse;
      }
    }
  }
}

// dlogits[r, c] = scale[r] * (softmax - onehot); scale[r] = dloss[r] (0 for
// ignored rows).  dlogits MAY alias logits.
extern "C" __global__ void __launch_bounds__(BLOCK)
ce_bwd_bf16(const unsigned short* __restrict__ logits,
            unsigned short* __restrict__ dlogits,
            const int64_t* __restrict__ target,
            const float* __restrict__ lse,
            const float* __restrict__ dloss,   // [N] upstream grad per row
            int64_t n_rows, int vocab, int64_t ignore_index) {
  const int vec = 8;
  const int iters = (vocab / vec + BLOCK - 1) / BLOCK;
  for (int64_t row = blockIdx.x; row < n_rows; row += gridDim.x) {
    const unsigned short* xr = logits + row * vocab;
    unsigned short* dr = dlogits + row * vocab;
    int64_t tgt = target[row];
    float l = lse[row];
    float sc = (tgt == ignore_index) ? 0.f : dloss[row];
    for (int it = 0; it < iters; ++it) {
      int i = (it * BLOCK + threadIdx.x) * vec;
      if (i < vocab) {
        short8v v = *reinterpret_cast<const short8v*>(xr + i);
        short8v o;
#pragma unroll
        for (int j = 0; j < vec; ++j) {
          int col = i + j;
          float f = bf16_to_f32((unsigned short)v[j]);
          float p = __expf(f - l);
          if (col == (int)tgt) p -= 1.f;
          o[j] = (short)f32_to_bf16(p * sc);
        }
        *reinterpret_cast<short8v*>(dr + i) = o;
      }
    }
  }
}

// ---------------------------------------------------------------------------
// Vocab-parallel (class-sharded) variant: this rank's logits hold columns
// [vocab_start, vocab_start + n) of a vocab_total-class row.  The forward
// gives the two per-row partials a rank owes the combine (local log-sum-exp,
// raw target logit if the target is a local column); the combine itself is
// two all-reduces on [N] fp32 fields in ops/functional.py.  The backward is
// the dense one with a column offset and the GLOBAL lse.
//
// Both kernels: one 256-thread block per row (rows grid-strided), a thread
// issues VP_UNROLL independent 16-byte loads before it touches any of them.
// A vector index past the row's end is clamped to the row's last vector, so
// the loads are unconditional and stay inside the row; what such a load
// brought is replaced by bf16 -inf (forward: adds exp(-inf) = 0) or not
// stored (backward), so no column predicate sits in the per-element code.
// Forward: ONE max over the thread's 32 values, one rescale of the running
// sum, then one __expf per element (33 per 32 elements; the dense kernel's
// online update spends 64).  The target column is read with an index only
// after it has been compared into [0, n); an out-of-range or ignored target
// reads nothing.  Requires n % 8 == 0 (16-byte rows for the short8v loads).
//
// hipcc -O3 --offload-arch=gfx950 (-Rpass-analysis=kernel-resource-usage):
//   ce_vp_fwd_bf16: 49 VGPRs, 16 B LDS, no scratch, 8 waves/SIMD
//   ce_vp_bwd_bf16: 42 VGPRs,  0 B LDS, no scratch, 8 waves/SIMD
// (dense pair, for comparison: 31 / 30 VGPRs, 8 waves/SIMD)
// ---------------------------------------------------------------------------
#define VP_UNROLL 4
#define BF16_NEG_INF ((short)0xFF80)

// logits: [N, n] bf16; target: [N] int64 (global ids); picked/lse_out: [N] f32
extern "C" __global__ void __launch_bounds__(BLOCK)
ce_vp_fwd_bf16(const unsigned short* __restrict__ logits,
               const int64_t* __restrict__ target,
               float* __restrict__ picked, float* __restrict__ lse_out,
               int64_t n_rows, int n, int64_t vocab_start, int64_t ignore_index) {
  __shared__ float lds[BLOCK / WAVE];
  const int nvec = n / 8;
  for (int64_t row = blockIdx.x; row < n_rows; row += gridDim.x) {
    const unsigned short* xr = logits + row * n;
    float mx = -INFINITY, sum = 0.f;
    for (int base = threadIdx.x; base < nvec; base += BLOCK * VP_UNROLL) {
      short8v v[VP_UNROLL];
#pragma unroll
      for (int u = 0; u < VP_UNROLL; ++u) {
        int idx = base + u * BLOCK;
        // branch-free: a vector past the end re-reads the row's last one
        short8v t = *reinterpret_cast<const short8v*>(xr + (int64_t)min(idx, nvec - 1) * 8);
        v[u] = idx < nvec ? t : (short8v)BF16_NEG_INF;
      }
      float f[VP_UNROLL][8];
      float vmax = -INFINITY;
#pragma unroll
      for (int u = 0; u < VP_UNROLL; ++u)
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          f[u][j] = bf16_to_f32((unsigned short)v[u][j]);
          vmax = fmaxf(vmax, f[u][j]);
        }
      float m2 = fmaxf(mx, vmax);
      float ms = ce_finite_max(m2);
      float part = 0.f;
#pragma unroll
      for (int u = 0; u < VP_UNROLL; ++u)
#pragma unroll
        for (int j = 0; j < 8; ++j) part += __expf(f[u][j] - ms);
      sum = sum * __expf(mx - ms) + part;
      mx = m2;
    }
    float gmax = block_reduce_max<BLOCK>(mx, lds);
    float gs = ce_finite_max(gmax);
    float gsum = block_reduce_sum<BLOCK>(sum * __expf(mx - gs), lds);
    if (threadIdx.x == 0) {
      int64_t tgt = target[row];
      bool local = tgt != ignore_index && tgt >= vocab_start && tgt < vocab_start + n;
      picked[row] = local ? bf16_to_f32(xr[tgt - vocab_start]) : 0.f;
      lse_out[row] = gmax + __logf(gsum);
    }
  }
}

// dlogits[r, c] = scale[r] * (exp(x[r, c] - lse[r]) - [c + vocab_start == target[r]]);
// scale[r] = dloss[r] (0 for ignored rows).  dlogits MAY alias logits: a
// thread writes only the vectors it has read, after it has read them.
extern "C" __global__ void __launch_bounds__(BLOCK)
ce_vp_bwd_bf16(const unsigned short* logits, unsigned short* dlogits,
               const int64_t* __restrict__ target,
               const float* __restrict__ lse,     // [N] global log-sum-exp
               const float* __restrict__ dloss,   // [N] upstream grad per row
               int64_t n_rows, int n, int64_t vocab_start, int64_t ignore_index) {
  const int nvec = n / 8;
  for (int64_t row = blockIdx.x; row < n_rows; row += gridDim.x) {
    const unsigned short* xr = logits + row * n;
    unsigned short* dr = dlogits + row * n;
    int64_t tgt = target[row];
    float l = lse[row];
    float sc = (tgt == ignore_index) ? 0.f : dloss[row];
    // local target column, -1 if the target is no column of this shard
    int lt = (tgt >= vocab_start && tgt < vocab_start + n) ? (int)(tgt - vocab_start) : -1;
    for (int base = threadIdx.x; base < nvec; base += BLOCK * VP_UNROLL) {
      short8v v[VP_UNROLL];
#pragma unroll
      for (int u = 0; u < VP_UNROLL; ++u) {
        int idx = base + u * BLOCK;
        // branch-free: a vector past the end re-reads the row's last one
        v[u] = *reinterpret_cast<const short8v*>(xr + (int64_t)min(idx, nvec - 1) * 8);
      }
#pragma unroll
      for (int u = 0; u < VP_UNROLL; ++u) {
        int idx = base + u * BLOCK;
        if (idx < nvec) {
          float p[8];
#pragma unroll
          for (int j = 0; j < 8; ++j) p[j] = __expf(bf16_to_f32((unsigned short)v[u][j]) - l);
          int d = lt - idx * 8;
          if (d >= 0 && d < 8) {
#pragma unroll
            for (int j = 0; j < 8; ++j) p[j] -= (j == d) ? 1.f : 0.f;
          }
          short8v o;
#pragma unroll
          for (int j = 0; j < 8; ++j) o[j] = (short)f32_to_bf16(p[j] * sc);
          *reinterpret_cast<short8v*>(dr + (int64_t)idx * 8) = o;
        }
      }
    }
  }
}
