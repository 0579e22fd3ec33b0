// Streaming transposing copy, bf16 [R,C] -> [C,R], through LDS — CDNA4
// memory-bound.  It prepares operands for the dense wgrad GEMMs (the library
// runs a product faster when both operands are contiguous along the
// contraction), so it has to cost a small fraction of a GEMM: 16-byte global
// loads and stores on both sides, one LDS round trip in between.
//
// A block moves one TT x TT tile.  The tile is stored ROW-MAJOR in LDS with
// ds_write_b128 and read back by COLUMNS, eight 2-byte reads per 16-byte
// output chunk.  The image is [TT rows][TT/8 slots of 16 bytes]; row r keeps
// its slot s at slot  s ^ ((r >> 3) & (TT/8 - 1)).  By the bank rules written
// down in fa32_lds_map.h (64 banks of 4 bytes):
//   - stores: 8 contiguous lanes write the 8 (or 8 of the 16) contiguous slots
//     of one row; XOR with a constant keeps them distinct mod 8, the
//     conflict-free ds_write_b128.
//   - column reads: a wave reads, per step i, one element each of rows
//     8*b + i for TT/8 consecutive b (the lanes of one output chunk row) and
//     64 / (TT/8) consecutive columns c of one aligned 8-column group, i.e.
//     of ONE slot s.  The rows differ only in r >> 3 = b, so the XOR sends
//     them to TT/8 distinct slots s ^ b; with TT = 64 a row is 128 bytes and
//     all rows 8*b + i have the same parity, so they also share the half of
//     the 64 banks that parity selects.  The wave thus touches 32 dwords (two
//     lanes per dword, one address: a broadcast, not a conflict) on 32
//     distinct banks: one pass.
// Partial tiles are predicated per 16-byte chunk (R % 8 == 0 and C % 8 == 0
// make a chunk all in or all out); no thread leaves before the barrier
// (rule 3 of README.md).  Chunks that were not loaded are never read: a valid
// output chunk (c, rows 8b..8b+7) reads only rows < R of column c < C.
// Indexing is 32-bit inside a tile and 64-bit for the tile bases.
#pragma once
#include "common.h"

#define TP_THREADS 256
// no packed fp32 VALU ops in the kernels built on this file (per kernel, as
// FF_NO_PK_F32 in fa32_common.h)
#define TP_NO_PK_F32 __attribute__((target("no-packed-fp32-ops")))

// byte offset of element (r, c) in the LDS image of a TT x TT tile
template <int TT>
DEV int tp_lds_byte(int r, int c) {
  return r * (TT * 2) + ((((c >> 3) ^ (r >> 3)) & (TT / 8 - 1)) << 4) + ((c & 7) << 1);
}

// Store chunk q (row q / (TT/8), 8 columns from 8 * (q % (TT/8))) row-major.
template <int TT>
DEV void tp_lds_put(unsigned char* lds, int q, short8v v) {
  const int r = q / (TT / 8), c = (q % (TT / 8)) * 8;
  *reinterpret_cast<short8v*>(lds + tp_lds_byte<TT>(r, c)) = v;
}

// Gather chunk q of the TRANSPOSED tile: column c = q / (TT/8) of the stored
// tile, rows 8*b .. 8*b + 7 with b = q % (TT/8).
template <int TT>
DEV short8v tp_lds_get_t(const unsigned char* lds, int q) {
  const int c = q / (TT / 8), b = q % (TT / 8);
  short8v v;
#pragma unroll
  for (int i = 0; i < 8; ++i)
    v[i] = *reinterpret_cast<const short*>(lds + tp_lds_byte<TT>(8 * b + i, c));
  return v;
}

// out[C,R] = in[R,C]^T.  grid = (ceil(R/TT), ceil(C/TT)): blockIdx.x walks the
// output's contiguous direction, so blocks that run together fill whole lines.
template <int TT>
DEV void transpose_body(const unsigned short* __restrict__ in,
                        unsigned short* __restrict__ out, int R, int C) {
  constexpr int CHUNKS = TT * TT / 8, PER = CHUNKS / TP_THREADS, CPR = TT / 8;
  static_assert(CHUNKS % TP_THREADS == 0, "whole chunks per thread");
  __shared__ __attribute__((aligned(16))) unsigned char lds[TT * TT * 2];
  const int r0 = blockIdx.x * TT, c0 = blockIdx.y * TT;
  const int rows = min(TT, R - r0), cols = min(TT, C - c0);  // valid extent, multiples of 8
  const unsigned short* src = in + ((int64_t)r0 * C + c0);
  unsigned short* dst = out + ((int64_t)c0 * R + r0);
  short8v v[PER] = {};
#pragma unroll
  for (int j = 0; j < PER; ++j) {
    const int q = threadIdx.x + j * TP_THREADS;
    const int r = q / CPR, c = (q % CPR) * 8;
    if (r < rows && c < cols) v[j] = *reinterpret_cast<const short8v*>(src + (r * C + c));
  }
#pragma unroll
  for (int j = 0; j < PER; ++j) tp_lds_put<TT>(lds, threadIdx.x + j * TP_THREADS, v[j]);
  __syncthreads();
#pragma unroll
  for (int j = 0; j < PER; ++j) {
    const int q = threadIdx.x + j * TP_THREADS;
    const int c = q / CPR, r = (q % CPR) * 8;
    const short8v t = tp_lds_get_t<TT>(lds, q);
    if (c < cols && r < rows) *reinterpret_cast<short8v*>(dst + (c * R + r)) = t;
  }
}

extern "C" __global__ void TP_NO_PK_F32 __launch_bounds__(TP_THREADS)
transpose_bf16(const unsigned short* __restrict__ in, unsigned short* __restrict__ out,
               int R, int C) {
  transpose_body<128>(in, out, R, C);
}

extern "C" __global__ void TP_NO_PK_F32 __launch_bounds__(TP_THREADS)
transpose_t64_bf16(const unsigned short* __restrict__ in, unsigned short* __restrict__ out,
                   int R, int C) {
  transpose_body<64>(in, out, R, C);
}
