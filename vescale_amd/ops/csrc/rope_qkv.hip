// Fused QKV-split + RoPE — CDNA4.
//
// Consumes the packed output of the fused wqkv GEMM [B, S, (Hq+2*Hkv)*D]
// and emits contiguous q/k/v in [B, H, S, D] layout (the attention
// kernels' native layout — saves three transpose-copies per layer) with
// RoPE applied to q and k — one read + one write instead of (3
// slice-copies + 2 rope passes + 3 transposes).  Backward packs dq/dk/dv
// back (inverse rotation on dq/dk).
//
// Two forms of each direction: the v8 kernels (16-byte vectors, D % 16 == 0)
// and the scalar kernels, which take any even D.  The binding selects.
#include "common.h"

#include <type_traits>

#define BLOCK 256

// forward: qkv [T, (Hq+2Hkv)*D] -> q [B,Hq,S,D] (roped), k [B,Hkv,S,D]
// (roped), v [B,Hkv,S,D].  T = B*S tokens; table [S, D/2, 2].
extern "C" __global__ void __launch_bounds__(BLOCK)
rope_qkv_fwd_bf16(const unsigned short* __restrict__ qkv,
                  unsigned short* __restrict__ q,
                  unsigned short* __restrict__ k,
                  unsigned short* __restrict__ v,
                  const float* __restrict__ table,
                  int64_t n_tokens, int seq, int Hq, int Hkv, int D,
                  int pos_offset) {
  const int rot = D / 2;
  const int row_in = (Hq + 2 * Hkv) * D;
  // one (token, head) pair handles D/2 rotation pairs; v heads copied raw.
  const int heads_total = Hq + 2 * Hkv;
  int64_t total = n_tokens * heads_total * rot;
  int64_t i0 = blockIdx.x * BLOCK + threadIdx.x;
  int64_t stride = (int64_t)gridDim.x * BLOCK;
  for (int64_t t = i0; t < total; t += stride) {
    int d = (int)(t % rot);
    int64_t th = t / rot;
    int h = (int)(th % heads_total);
    int64_t tok = th / heads_total;
    int64_t s = tok % seq;
    int64_t b = tok / seq;
    const unsigned short* src = qkv + tok * row_in + (int64_t)h * D;
    float x0 = bf16_to_f32(src[d]);
    float x1 = bf16_to_f32(src[d + rot]);
    unsigned short* dst;
    bool do_rope = true;
    if (h < Hq) {
      dst = q + (((b * Hq + h) * seq) + s) * D;
    } else if (h < Hq + Hkv) {
      dst = k + (((b * Hkv + (h - Hq)) * seq) + s) * D;
    } else {
      dst = v + (((b * Hkv + (h - Hq - Hkv)) * seq) + s) * D;
      do_rope = false;
    }
    if (do_rope) {
      const float* tb = table + ((s + pos_offset) * (int64_t)rot + d) * 2;
      float c = tb[0], sn = tb[1];
      dst[d] = f32_to_bf16(x0 * c - x1 * sn);
      dst[d + rot] = f32_to_bf16(x1 * c + x0 * sn);
    } else {
      dst[d] = f32_to_bf16(x0);
      dst[d + rot] = f32_to_bf16(x1);
    }
  }
}

// backward: dq/dk/dv -> dqkv packed; inverse rotation (negated sin) on dq,dk
extern "C" __global__ void __launch_bounds__(BLOCK)
rope_qkv_bwd_bf16(const unsigned short* __restrict__ dq,
                  const unsigned short* __restrict__ dk,
                  const unsigned short* __restrict__ dv,
                  unsigned short* __restrict__ dqkv,
                  const float* __restrict__ table,
                  int64_t n_tokens, int seq, int Hq, int Hkv, int D,
                  int pos_offset) {
  const int rot = D / 2;
  const int row_out = (Hq + 2 * Hkv) * D;
  const int heads_total = Hq + 2 * Hkv;
  int64_t total = n_tokens * heads_total * rot;
  int64_t i0 = blockIdx.x * BLOCK + threadIdx.x;
  int64_t stride = (int64_t)gridDim.x * BLOCK;
  for (int64_t t = i0; t < total; t += stride) {
    int d = (int)(t % rot);
    int64_t th = t / rot;
    int h = (int)(th % heads_total);
    int64_t tok = th / heads_total;
    int64_t s = tok % seq;
    int64_t b = tok / seq;
    const unsigned short* src;
    bool do_rope = true;
    if (h < Hq) {
      src = dq + (((b * Hq + h) * seq) + s) * D;
    } else if (h < Hq + Hkv) {
      src = dk + (((b * Hkv + (h - Hq)) * seq) + s) * D;
    } else {
      src = dv + (((b * Hkv + (h - Hq - Hkv)) * seq) + s) * D;
      do_rope = false;
    }
    float x0 = bf16_to_f32(src[d]);
    float x1 = bf16_to_f32(src[d + rot]);
    unsigned short* dst = dqkv + tok * row_out + (int64_t)h * D;
    if (do_rope) {
      const float* tb = table + ((s + pos_offset) * (int64_t)rot + d) * 2;
      float c = tb[0], sn = -tb[1];
      dst[d] = f32_to_bf16(x0 * c - x1 * sn);
      dst[d + rot] = f32_to_bf16(x1 * c + x0 * sn);
    } else {
      dst[d] = f32_to_bf16(x0);
      dst[d + rot] = f32_to_bf16(x1);
    }
  }
}

// ---------------------------------------------------------------------------
// 16-byte form, D % 16 == 0 and D / 16 <= 64.  One WAVE per token: the wave's
// lanes are (head slot, unit) with unit = lane % (D/16); a lane moves the 8
// elements [8*unit, 8*unit + 8) of the low half and the matching 8 of the
// high half of one head per pass and walks the token's heads slot by slot.
// Its 8 (cos, sin) pairs depend on the token and the unit only, so they are
// read once per token (4 float4s) and serve every roped head the lane visits.
// A V head is the same two 16-byte moves without the rotation.  All offsets
// inside a token are 32-bit; the token's bases are computed once per token.
// BWD swaps source and destination and negates sin.
// ---------------------------------------------------------------------------
template <bool BWD>
DEV void rope_qkv_v8_t(
    std::conditional_t<BWD, unsigned short, const unsigned short>* __restrict__ packed,
    std::conditional_t<BWD, const unsigned short, unsigned short>* __restrict__ q,
    std::conditional_t<BWD, const unsigned short, unsigned short>* __restrict__ k,
    std::conditional_t<BWD, const unsigned short, unsigned short>* __restrict__ v,
    const float* __restrict__ table, int64_t n_tokens, int seq, int Hq, int Hkv, int D,
    int pos_offset) {
  const int rot = D / 2;
  const int upd = D / 16;           // 16-element units per head
  const int slots = WAVE / upd;     // heads per pass
  const int lane = threadIdx.x & (WAVE - 1);
  const int slot = lane / upd;
  const int d0 = (lane - slot * upd) * 8;
  const int heads_total = Hq + 2 * Hkv;
  const int row = heads_total * D;
  const int64_t head_stride = (int64_t)seq * D;  // between heads of q / k / v
  const int waves = BLOCK / WAVE;
  if (slot >= slots) return;  // D/16 does not divide 64: the tail lanes idle
  for (int64_t tok = (int64_t)blockIdx.x * waves + (threadIdx.x / WAVE); tok < n_tokens;
       tok += (int64_t)gridDim.x * waves) {
    const int64_t b = tok / seq;
    const int s = (int)(tok - b * seq);
    const float4v* tb = reinterpret_cast<const float4v*>(
        table + ((int64_t)(s + pos_offset) * rot + d0) * 2);
    float cs[16];  // c0 s0 c1 s1 ...
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      float4v t = tb[j];
#pragma unroll
      for (int e = 0; e < 4; ++e) cs[j * 4 + e] = t[e];
    }
    auto* pk = packed + tok * row + d0;
    const int64_t in_head = (int64_t)s * D + d0;
    auto* qt = q + b * Hq * head_stride + in_head;
    auto* kt = k + b * Hkv * head_stride + in_head;
    auto* vt = v + b * Hkv * head_stride + in_head;
#pragma unroll 2
    for (int h = slot; h < heads_total; h += slots) {
      const bool roped = h < Hq + Hkv;
      auto* hp = h < Hq ? qt + h * head_stride
                        : (roped ? kt + (h - Hq) * head_stride
                                 : vt + (h - Hq - Hkv) * head_stride);
      auto* pp = pk + h * D;
      short8v lo, hi;
      if constexpr (BWD) {
        lo = *reinterpret_cast<const short8v*>(hp);
        hi = *reinterpret_cast<const short8v*>(hp + rot);
      } else {
        lo = *reinterpret_cast<const short8v*>(pp);
        hi = *reinterpret_cast<const short8v*>(pp + rot);
      }
      if (roped) {
#pragma unroll
        for (int e = 0; e < 8; ++e) {
          float x0 = bf16_to_f32((unsigned short)lo[e]);
          float x1 = bf16_to_f32((unsigned short)hi[e]);
          const float c = cs[2 * e], sn = cs[2 * e + 1];
          // The scalar kernels' x0*c - x1*sn and x1*c + x0*sn (sn negated in
          // the backward) compile to one rounded product and one fma each: a
          // difference fuses its first product, a sum its second.  Spelled
          // out here, because left to the compiler this unrolled body fuses
          // some elements and not others, and the two forms of the kernel
          // (and a model's results) would differ in the last bf16 bit.
          if constexpr (BWD) {
            lo[e] = (short)f32_to_bf16(__builtin_fmaf(x1, sn, x0 * c));
            hi[e] = (short)f32_to_bf16(__builtin_fmaf(x1, c, -(x0 * sn)));
          } else {
            lo[e] = (short)f32_to_bf16(__builtin_fmaf(x0, c, -(x1 * sn)));
            hi[e] = (short)f32_to_bf16(__builtin_fmaf(x0, sn, x1 * c));
          }
        }
      }
      if constexpr (BWD) {
        *reinterpret_cast<short8v*>(pp) = lo;
        *reinterpret_cast<short8v*>(pp + rot) = hi;
      } else {
        *reinterpret_cast<short8v*>(hp) = lo;
        *reinterpret_cast<short8v*>(hp + rot) = hi;
      }
    }
  }
}

extern "C" __global__ void __launch_bounds__(BLOCK)
rope_qkv_fwd_v8_bf16(const unsigned short* __restrict__ qkv,
                     unsigned short* __restrict__ q,
                     unsigned short* __restrict__ k,
                     unsigned short* __restrict__ v,
                     const float* __restrict__ table,
                     int64_t n_tokens, int seq, int Hq, int Hkv, int D,
                     int pos_offset) {
  rope_qkv_v8_t<false>(qkv, q, k, v, table, n_tokens, seq, Hq, Hkv, D, pos_offset);
}

extern "C" __global__ void __launch_bounds__(BLOCK)
rope_qkv_bwd_v8_bf16(const unsigned short* __restrict__ dq,
                     const unsigned short* __restrict__ dk,
                     const unsigned short* __restrict__ dv,
                     unsigned short* __restrict__ dqkv,
                     const float* __restrict__ table,
                     int64_t n_tokens, int seq, int Hq, int Hkv, int D,
                     int pos_offset) {
  rope_qkv_v8_t<true>(dqkv, dq, dk, dv, table, n_tokens, seq, Hq, Hkv, D, pos_offset);
}
