// Grouped expert GEMM for the MoE layer: forward, dgrad and wgrad, each ONE
// launch over all experts, group boundaries read from device memory.
//
//   rows sorted by expert; offs int32 [E+1] on the device, expert e owns rows
//   offs[e]..offs[e+1]; W[e] [N,K] bf16 (nn.Linear); bf16 operands, fp32
//   accumulation, one rounding to bf16; no atomics, no split-K: every output
//   element is one MFMA chain in a fixed order, so results repeat to the bit.
//
//   fwd    Y[t,:]  = X[t,:]  . W[e(t)]^T    X  [T,K] -> [T,N]   contraction K
//   dgrad  dX[t,:] = dY[t,:] . W[e(t)]      dY [T,N] -> [T,K]   contraction N
//   wgrad  dW[e]   = dY[e]^T . X[e]         -> [E,N,K]          contraction rows(e)
//
// Work split.  fwd / dgrad: a block owns 128 rows x 128 output columns and
// walks the contraction 64 at a time.  A row tile never spans two experts:
// the grid has T/128 + E row tiles (>= sum ceil(n_e/128), sized on the host
// from T and E alone, no sync) and every block maps its tile index to
// (expert, first row) by a block-uniform walk over the offsets; surplus blocks
// return as whole blocks before the first barrier (README rule 3).  wgrad: one
// block per (expert, 128x128 tile of dW[e]) walks the group's rows 64 at a
// time; an empty group runs zero steps and stores its zero accumulators.
// 256 threads = 4 waves as 2x2, a wave owns 64x64 = 4x4 MFMA 16x16x32 tiles
// (operand fragment row = lane&15, k = 8*(lane>>4)..+8; the layout
// fa16_common.h runs and the probes verified): per 32 of contraction 8
// ds_read_b128 feed 16 MFMAs.  The product is formed as (B rows) x (A rows),
// so a lane's four accumulator values are four CONSECUTIVE output columns of
// one output row: the epilogue is one 8-byte store per MFMA tile.
//
// Offsets are untrusted device data (rule 5 for what the host cannot read):
// every bound is clamped to [0, T] and made monotone by a running maximum,
// b[0] = clamp(offs[0]), b[e+1] = max(b[e], clamp(offs[e+1])); expert e owns
// [b[e], b[e+1]).  For valid offsets that is offs itself; offs[e+1] < offs[e]
// is an empty group; groups never overlap (no output row has two writers) and
// sum to <= T (the grid bound holds); every row index that reaches an address
// is < T.  Rows outside [b[0], b[E]) are not written.
//
// Transposed operands.  dgrad's W and both wgrad operands are contraction-
// major in global memory.  They are staged TRANSPOSED INTO LDS (the
// fg_tile_t route, not ds_read_b64_tr_b16): a thread loads 4 consecutive
// contraction rows x 8 columns (four 16-byte loads, 256-byte coalesced per 16
// lanes), transposes 4x8 in registers (plain moves) and writes eight 8-byte
// LDS stores.  Why: after staging every operand of every form has ONE LDS
// image, [128 rows][64 k], so all three kernels share one fragment read, one
// MFMA loop and one epilogue, on the layout the 16x16 family already
// verified; the tr read returns 4x4-transposed 4-lane groups that feed the
// 32x32x16 operand layout of fa32_common.h and would need a second compute
// path (and its own probe) for two of the three forms.  The price is paid in
// LDS stores (8 ds_write_b64 instead of 4 ds_write_b128 per thread, operand
// and step), not in global memory: no transposed copy of a weight or an
// activation is ever made there.
//
// LDS image (by the bank rules fa32_lds_map.h models: 64 banks x 4 bytes, a
// ds_read_b128 served in four 16-lane groups {0-3,12-15,20-27},
// {4-11,16-19,28-31}, +32).  A tile row is 128 bytes = 8 slots of 16 bytes;
// row r stores slot s at  s ^ ((r >> 1) ^ (r >> 4)) & 7.  A fragment read
// takes 16 consecutive rows (16-aligned, so r >> 4 is a constant) at slot
// 4*kc + (lane >> 4); a served group holds all 16 rows, eight at slot q and
// eight (rows 4-11) at slot q ^ 1.  Two rows of equal parity share their 256-
// byte bank phase; (r >> 1) ^ [4 <= r <= 11] is a bijection on the 8 rows of a
// parity, so the 16 lanes land on 16 distinct slots = 64 distinct banks:
// 4 LDS cycles per ds_read_b128, the conflict-free cost.  Row-major staging
// stores (ds_write_b128, 8 lanes per row on 8 distinct slots) are conflict-
// free as well; the transposing ds_write_b64 is 2-way conflicted (the r >> 4
// term spreads its 16 column chunks over all 8 slots; without it, 16-way).
#pragma once
#include "common.h"

#define GG_BM 128        // tile rows
#define GG_BN 128        // tile output columns
#define GG_BK 64         // contraction step
#define GG_THREADS 256   // 4 waves, 2 x 2
#define GG_MAX_E 64      // experts per launch (the by-value pointer table)
#define GG_ROW_BYTES (GG_BK * 2)

typedef float gg_floatx4 __attribute__((ext_vector_type(4)));
typedef short gg_shortx8 __attribute__((ext_vector_type(8)));
typedef short gg_shortx4 __attribute__((ext_vector_type(4)));

// W[e] base pointers, passed by value in the kernel arguments
struct GGPtrs {
  const unsigned short* p[GG_MAX_E];
};

// byte offset of 16-byte slot `slot` of tile row `row` in the LDS image
DEV int gg_map(int row, int slot) {
  return row * GG_ROW_BYTES + ((slot ^ (((row >> 1) ^ (row >> 4)) & 7)) << 4);
}

// One operand of a tile product.  Row-major over the contraction (TR = false):
// tile row i is global row r0 + i (zero at and past r_end) and contraction
// index k is column c0 + k.  Contraction-major (TR = true): tile row i is
// global column c0 + i and contraction index k is global row r0 + k (zero at
// and past r_end).
struct gg_operand {
  const unsigned short* p;
  int64_t ld;  // row stride in elements
  int r0, r_end, c0;
};

// 8 elements at (row, col), or zeros WITHOUT a load when the row is out of
// the group: a select, so a NaN beyond the boundary never meets a zero
DEV gg_shortx8 gg_ld8(const gg_operand& o, int row, int col) {
  gg_shortx8 v = {0, 0, 0, 0, 0, 0, 0, 0};
  if (row < o.r_end) v = *reinterpret_cast<const gg_shortx8*>(o.p + (int64_t)row * o.ld + col);
  return v;
}

// global -> staging registers for contraction step [kk, kk + 64)
template <bool TR>
DEV void gg_load(gg_shortx8 (&reg)[4], const gg_operand& o, int kk, int tid) {
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    if constexpr (!TR) {
      const int i = tid + j * GG_THREADS;  // chunk: row i / 8, slot i % 8
      reg[j] = gg_ld8(o, o.r0 + (i >> 3), o.c0 + kk + (i & 7) * 8);
    } else {
      // contraction rows 4*(tid / 16) + j, columns 8*(tid % 16)..+8
      reg[j] = gg_ld8(o, o.r0 + kk + (tid >> 4) * 4 + j, o.c0 + (tid & 15) * 8);
    }
  }
}

// staging registers -> LDS image [128][64]
template <bool TR>
DEV void gg_store(const gg_shortx8 (&reg)[4], unsigned short* tile, int tid) {
  if constexpr (!TR) {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int i = tid + j * GG_THREADS;
      *reinterpret_cast<gg_shortx8*>((char*)tile + gg_map(i >> 3, i & 7)) = reg[j];
    }
  } else {
    const int ng = tid >> 4;  // contraction elements 4*ng..+4 = half (ng & 1) of slot ng / 2
#pragma unroll
    for (int x = 0; x < 8; ++x) {
      const int row = (tid & 15) * 8 + x;
      const gg_shortx4 v = {reg[0][x], reg[1][x], reg[2][x], reg[3][x]};
      *reinterpret_cast<gg_shortx4*>((char*)tile + gg_map(row, ng >> 1) + (ng & 1) * 8) = v;
    }
  }
}

// operand fragment: rows 16*rf + (lane & 15), contraction 32*kc + 8*(lane >> 4)..+8
DEV gg_shortx8 gg_frag(const unsigned short* tile, int rf, int kc, int lane) {
  return *reinterpret_cast<const gg_shortx8*>(
      (const char*)tile + gg_map(rf * 16 + (lane & 15), kc * 4 + (lane >> 4)));
}

// clamped offset e
DEV int gg_bound(const int* offs, int e, int T) { return min(max(offs[e], 0), T); }

// The block's 128 x 128 tile: out[orow0 + i][ocol0 + j] = sum_k A[i][k] B[j][k]
// over `nsteps` contraction steps of 64, rows at and past orow_end not stored.
// Every argument but tid is block-uniform, so the barriers are too.
template <bool AT, bool BT>
DEV void gg_tile_gemm(const gg_operand& A, const gg_operand& B, int nsteps,
                      unsigned short* out, int64_t ldo, int orow0, int orow_end, int ocol0,
                      unsigned short* As, unsigned short* Bs) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wi = wave >> 1, wj = wave & 1;
  gg_floatx4 acc[4][4];
#pragma unroll
  for (int fi = 0; fi < 4; ++fi)
#pragma unroll
    for (int fj = 0; fj < 4; ++fj) acc[fi][fj] = (gg_floatx4){0.f, 0.f, 0.f, 0.f};

  gg_shortx8 ra[4], rb[4];
  if (nsteps > 0) {
    gg_load<AT>(ra, A, 0, tid);
    gg_load<BT>(rb, B, 0, tid);
  }
  for (int s = 0; s < nsteps; ++s) {
    __syncthreads();  // the previous step's fragment reads are done
    gg_store<AT>(ra, As, tid);
    gg_store<BT>(rb, Bs, tid);
    __syncthreads();
    if (s + 1 < nsteps) {  // next step's global loads fly under this step's MFMAs
      gg_load<AT>(ra, A, (s + 1) * GG_BK, tid);
      gg_load<BT>(rb, B, (s + 1) * GG_BK, tid);
    }
#pragma unroll
    for (int kc = 0; kc < 2; ++kc) {
      gg_shortx8 af[4], bf[4];
#pragma unroll
      for (int f = 0; f < 4; ++f) {
        af[f] = gg_frag(As, wi * 4 + f, kc, lane);
        bf[f] = gg_frag(Bs, wj * 4 + f, kc, lane);
      }
#pragma unroll
      for (int fi = 0; fi < 4; ++fi)
#pragma unroll
        for (int fj = 0; fj < 4; ++fj)
          acc[fi][fj] =
              __builtin_amdgcn_mfma_f32_16x16x32_bf16(bf[fj], af[fi], acc[fi][fj], 0, 0, 0);
    }
  }

  // D layout of (B rows) x (A rows): lane holds output row (lane & 15) of the
  // MFMA tile and its columns 4*(lane >> 4) + 0..3
#pragma unroll
  for (int fi = 0; fi < 4; ++fi) {
    const int row = orow0 + wi * 64 + fi * 16 + (lane & 15);
    if (row < orow_end) {
      unsigned short* orow = out + (int64_t)row * ldo + ocol0 + wj * 64 + (lane >> 4) * 4;
#pragma unroll
      for (int fj = 0; fj < 4; ++fj) {
        gg_shortx4 v;
#pragma unroll
        for (int r = 0; r < 4; ++r) v[r] = (short)f32_to_bf16(acc[fi][fj][r]);
        *reinterpret_cast<gg_shortx4*>(orow + fj * 16) = v;
      }
    }
  }
}

// fwd (DGRAD = false): a = X [T,K], out = Y [T,N].  dgrad: a = dY [T,N], out =
// dX [T,K], W read contraction-major.  grid (T/128 + E, out columns / 128).
template <bool DGRAD>
__global__ __launch_bounds__(GG_THREADS) void gemm_grouped_rows_bf16(
    const unsigned short* __restrict__ a, GGPtrs w, const int* __restrict__ offs,
    unsigned short* __restrict__ out, int T, int E, int N, int K) {
  __shared__ __attribute__((aligned(16))) unsigned short As[GG_BM * GG_BK];
  __shared__ __attribute__((aligned(16))) unsigned short Bs[GG_BN * GG_BK];
  // row tile -> (expert, first row): a block-uniform walk over the offsets
  int rt = blockIdx.x, e = 0, lo = gg_bound(offs, 0, T), hi = lo;
  for (; e < E; ++e) {
    hi = max(lo, gg_bound(offs, e + 1, T));
    const int tiles = (hi - lo + GG_BM - 1) / GG_BM;
    if (rt < tiles) break;
    rt -= tiles;
    lo = hi;
  }
  if (e == E) return;  // a surplus block: all of it, before any barrier
  const int row0 = lo + rt * GG_BM, c0 = blockIdx.y * GG_BN;
  const int C = DGRAD ? N : K;  // contraction length
  const gg_operand A = {a, C, row0, hi, 0};
  const gg_operand B = DGRAD ? gg_operand{w.p[e], K, 0, N, c0} : gg_operand{w.p[e], K, c0, N, 0};
  gg_tile_gemm<false, DGRAD>(A, B, C / GG_BK, out, DGRAD ? K : N, row0, hi, c0, As, Bs);
}

// dW[e] = dY[rows of e]^T . X[rows of e]; grid (K/128, N/128, E)
__global__ __launch_bounds__(GG_THREADS) void gemm_grouped_wgrad_bf16(
    const unsigned short* __restrict__ dy, const unsigned short* __restrict__ x,
    const int* __restrict__ offs, unsigned short* __restrict__ dw, int T, int N, int K) {
  __shared__ __attribute__((aligned(16))) unsigned short As[GG_BM * GG_BK];
  __shared__ __attribute__((aligned(16))) unsigned short Bs[GG_BN * GG_BK];
  const int e = blockIdx.z;
  int lo = gg_bound(offs, 0, T), hi = lo;
  for (int g = 0; g <= e; ++g) {
    lo = hi;
    hi = max(lo, gg_bound(offs, g + 1, T));
  }
  const int n0 = blockIdx.y * GG_BM, k0 = blockIdx.x * GG_BN;
  const gg_operand A = {dy, N, lo, hi, n0};
  const gg_operand B = {x, K, lo, hi, k0};
  gg_tile_gemm<true, true>(A, B, (hi - lo + GG_BK - 1) / GG_BK, dw + (int64_t)e * N * K, K, n0,
                           N, k0, As, Bs);
}
