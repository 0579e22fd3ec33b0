// Shared device helpers of the 16x16x32-MFMA flash-attention family
// (attention_gen.hip).  Every idiom of the family lives HERE, once
// (csrc/README.md rule 7).
//
// 64-row tiles, 4 waves; wave w owns rows [16w, 16w+16) of its tile.  Every
// GEMM is TN, C[i][j] = sum_k X[i][k] * Y[j][k], both operands row-major over
// the contraction: operand fragment row = lane&15, k-chunk = lane>>4;
// D-layout col = lane&15, row = 4*(lane>>4)+r.  LDS tiles carry a +8-elem row
// pad: a staged tile is [64][D+8], its transpose [D][72], P / dS [64][72].
// A thread stages D/32 8-elem chunks of a tile; chunk j of thread tid is
// element (tid + 256*j) * 8 of the [64, D] tile.
//
// No helper holds a barrier (rule 3), and every loop over a register array
// is statically unrolled (runtime-indexed arrays spill).
#pragma once
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

// key `col` is visible to query `row`
DEV bool fg_vis(int row, int col, int Sk, int causal, int shift) {
  return col < Sk && (!causal || col <= row + shift);
}

// Segment (document) mask, a compile-time variant of the family: with SEG,
// key `col` is visible to query `row` iff the rule above holds AND the two
// rows carry the same segment id.  Ids are compared for equality only; no
// value is special and they need not be sorted.  Without SEG the ids are
// dead arguments and the test is the one above.
template <bool SEG>
DEV bool fg_vis(int row, int col, int Sk, int causal, int shift, int qs, int ks) {
  bool vis = fg_vis(row, col, Sk, causal, shift);
  if constexpr (SEG) vis = vis && qs == ks;
  return vis;
}

// segment id of row `row` of one batch row's [n] ids.  Rows past the end are
// not read; what stands in for them never matters (tail keys fail col < Sk,
// tail queries are never stored and carry l2 = +inf in backward).
DEV int fg_seg(const int* seg, int row, int n) { return row < n ? seg[row] : 0; }

// The tile bounds of a call, written by fa_gen_seg_bounds_kernel: per batch
// row, (min, max) pairs of its ceil(Sq/64) q tiles, then of its ceil(Sk/64)
// kv tiles.  qb / kb = the pairs of batch row b's q / kv tiles.
DEV int fg_tiles(int n) { return (n + FG_BLK - 1) / FG_BLK; }
DEV void fg_seg_bounds(const int* bounds, int b, int Sq, int Sk, const int*& qb,
                       const int*& kb) {
  qb = bounds + (int64_t)b * (fg_tiles(Sq) + fg_tiles(Sk)) * 2;
  kb = qb + 2 * fg_tiles(Sq);
}

// [min, max] of the segment ids of 64-row tile `tile`.  The index is
// block-uniform wherever this is called, so these are scalar loads.
DEV void fg_seg_range(const int* bounds, int tile, int& lo, int& hi) {
  lo = bounds[2 * tile];
  hi = bounds[2 * tile + 1];
}

// A (q tile, kv tile) pair can hold an equal pair of ids only if the two id
// ranges overlap: conservative for unsorted ids, exact for sorted ones.  A
// block-uniform fact: the caller skips the whole loop iteration on it,
// staging and barriers included, for all waves at once (rule 3).
DEV bool fg_seg_overlap(int qlo, int qhi, int klo, int khi) {
  return qlo <= khi && klo <= qhi;
}

template <int N>
DEV void fg_zero(fg_floatx4 (&acc)[N]) {
#pragma unroll
  for (int f = 0; f < N; ++f) acc[f] = (fg_floatx4){0.f, 0.f, 0.f, 0.f};
}

// this wave's operand fragments, straight from global: rows
// row0 + 16*wave + (lane&15) of a [nrows, D] head, zero past the end
template <int D>
DEV void fg_wave_frags(fg_shortx8 (&x)[D / 32], const unsigned short* head, int row0,
                       int nrows, int wave, int lane) {
#pragma unroll
  for (int kc = 0; kc < D / 32; ++kc)
    x[kc] = fg_ld8<D>(head, row0 + wave * 16 + (lane & 15), nrows, kc * 32 + (lane >> 4) * 8);
}

// rows [row0, row0 + 64) of a [nrows, D] head into staging registers (zero
// past the end) ...
template <int D>
DEV void fg_tile_load(fg_shortx8 (&reg)[D / 32], const unsigned short* head, int row0,
                      int nrows, int tid) {
#pragma unroll
  for (int j = 0; j < D / 32; ++j) {
    int e = (tid + j * FG_THREADS) * 8;
    reg[j] = fg_ld8<D>(head, row0 + e / D, nrows, e % D);
  }
}
// ... from there into LDS as rows [64][D+8] ...
template <int D>
DEV void fg_tile_rows(const fg_shortx8 (&reg)[D / 32], unsigned short* t, int tid) {
#pragma unroll
  for (int j = 0; j < D / 32; ++j) {
    int e = (tid + j * FG_THREADS) * 8;
    *reinterpret_cast<fg_shortx8*>(t + (e / D) * (D + FG_PAD) + e % D) = reg[j];
  }
}
// ... or transposed [D][72] (also the rewrite of a buffer whose rows have
// been consumed: the caller puts the barrier in between)
template <int D>
DEV void fg_tile_t(const fg_shortx8 (&reg)[D / 32], unsigned short* t, int tid) {
#pragma unroll
  for (int j = 0; j < D / 32; ++j) {
    int e = (tid + j * FG_THREADS) * 8;
    int r = e / D, c = e % D;
#pragma unroll
    for (int x = 0; x < 8; ++x) t[(c + x) * FG_ROWS_N + r] = (unsigned short)reg[j][x];
  }
}
// load + rows, keeping the staging registers for a later fg_tile_t
template <int D>
DEV void fg_stage(fg_shortx8 (&reg)[D / 32], const unsigned short* head, int row0,
                  int nrows, unsigned short* t, int tid) {
  fg_tile_load<D>(reg, head, row0, nrows, tid);
  fg_tile_rows<D>(reg, t, tid);
}
// the plain form, for a tile that is only ever read as rows
template <int D>
DEV void fg_stage(const unsigned short* head, int row0, int nrows, unsigned short* t, int tid) {
  fg_shortx8 reg[D / 32];
  fg_stage<D>(reg, head, row0, nrows, t, tid);
}

// score block: acc[f] += X . rows [16f, 16f+16) of Y; x = this wave's
// fragments over the contraction, y a row-major [64][stride] tile
template <int KC>
DEV void fg_score(fg_floatx4 (&acc)[4], const fg_shortx8 (&x)[KC], const unsigned short* y,
                  int stride, int lane) {
#pragma unroll
  for (int kc = 0; kc < KC; ++kc)
#pragma unroll
    for (int f = 0; f < 4; ++f)
      acc[f] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
          x[kc], fg_frag(y, stride, f, kc, lane), acc[f], 0, 0, 0);
}

// accumulate block: acc[f] += X[wave rows, 64] . Y with x a [64][72] tile
// (P or dS) and yt = Y^T, [16*NF][72]
template <int NF>
DEV void fg_accum(fg_floatx4 (&acc)[NF], const unsigned short* x, const unsigned short* yt,
                  int wave, int lane) {
#pragma unroll
  for (int kc = 0; kc < 2; ++kc) {
    fg_shortx8 xf = fg_frag(x, FG_ROWS_N, wave, kc, lane);
#pragma unroll
    for (int f = 0; f < NF; ++f)
      acc[f] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
          xf, fg_frag(yt, FG_ROWS_N, f, kc, lane), acc[f], 0, 0, 0);
  }
}

// backward's P from a raw score and l2 = lse * log2e, and dS from P; the
// selections keep masked entries and dead rows (l2 = +inf) at exactly 0
DEV float fg_p(bool vis, float s, float scale_log2, float l2) {
  return vis ? exp2f(s * scale_log2 - l2) : 0.f;
}
DEV float fg_ds(float p, float dp, float delta, float scale) {
  return (p > 0.f) ? p * (dp - delta) * scale : 0.f;
}

// l2 = lse * log2e and delta of query row `row`; +inf / 0 on dead or tail rows
DEV void fg_lse_delta(const float* lse, const float* delta, int row, int Sq, float& l2,
                      float& dl) {
  float l = INFINITY, d = 0.f;
  if (row < Sq) {
    float lv = lse[row];
    if (lv > -INFINITY) l = lv * FG_LOG2E;
    d = delta[row];
  }
  l2 = l;
  dl = d;
}

// D-layout store of acc to rows row0 + r (r < 4; row0 = the lane's first row)
// of a [nrows, D] head; rows past the end are not stored
template <int D>
DEV void fg_store(unsigned short* head, const fg_floatx4 (&acc)[D / 16], int row0, int nrows,
                  int lane) {
#pragma unroll
  for (int r = 0; r < 4; ++r)
    if (row0 + r < nrows) {
#pragma unroll
      for (int f = 0; f < D / 16; ++f)
        head[(int64_t)(row0 + r) * D + f * 16 + (lane & 15)] = f32_to_bf16(acc[f][r]);
    }
}
