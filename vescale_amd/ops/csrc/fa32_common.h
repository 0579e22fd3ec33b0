// Shared device helpers of the 32x32x16-MFMA flash-attention family
// (attention_fwd.hip, attention_bwd2.hip, the tr probe in probes.hip):
// causal, GQA, D=128, bf16 tiles staged row-major + XOR swizzle in LDS (the
// map itself, and why it is bank-conflict-free, is fa32_lds_map.h).
// Every idiom of the family lives HERE, once; the kernels and the probe
// call it, so the probe exercises the exact code the kernels run
// (csrc/README.md rule 6).
#pragma once
#include "common.h"
#include "fa32_lds_map.h"

#define FF_D 128
#define FF_LOG2E 1.44269504088896340736f
#define FF_LN2 0.69314718055994530942f

typedef float ff_floatx16 __attribute__((ext_vector_type(16)));
typedef short ff_shortx4 __attribute__((ext_vector_type(4)));
typedef short ff_shortx8 __attribute__((ext_vector_type(8)));
typedef int ff_intx4 __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(3))) const unsigned short* ff_lds_p;

// partner-half exchange: returns the value this VGPR holds in lane l^32.
// permlane32_swap(a,b) returns the post-swap pair: r0 = [a:0-31 | b:0-31],
// r1 = [a:32-63 | b:32-63] (probe-verified: tools/fa_fwd_check.py — lane 0
// sees partner in r1, lane 32 sees partner in r0).
DEV int ff_swap_other(int x, int half) {
  auto r = __builtin_amdgcn_permlane32_swap(x, x, false, false);
  return half ? r[0] : r[1];
}

// XCD-aware block remap (guide T1): the 8 XCDs have private L2s and the
// HW round-robins consecutive workgroups across them; remapping so each
// XCD owns a CONTIGUOUS chunk of the flat grid keeps all q-tiles of the
// same (batch, head) — which stream the same K/V — on one XCD's L2.
// Bijective when nwg % 8 == 0 (else identity).
DEV void ff_xcd_remap(int& bx, int& by, int& bz) {
  int gx = gridDim.x, gy = gridDim.y;
  int nwg = gx * gy * (int)gridDim.z;
  if ((nwg & 7) != 0) return;
  int f = bx + gx * (by + gy * bz);
  f = (f & 7) * (nwg >> 3) + (f >> 3);
  bx = f % gx; f /= gx;
  by = f % gy;
  bz = f / gy;
}

// Kernel prologue: lane facts, the XCD-remapped block coordinates of a
// (tile, head, batch) grid and the head's base offsets.
struct ff_ctx {
  int tid, lane, wave;
  int l31, half;         // lane & 31, lane >> 5
  int tile, h, b;        // remapped blockIdx.x / .y / .z
  int64_t rbase;         // ((b*Hq + h) * S): row base into lse / delta
  int64_t qbase, kbase;  // element base of this head in q-shaped / k-shaped tensors
};
DEV ff_ctx ff_prologue(int Hq, int Hkv, int S) {
  ff_ctx c;
  c.tid = threadIdx.x;
  c.lane = c.tid & 63;
  c.wave = c.tid >> 6;
  c.l31 = c.lane & 31;
  c.half = c.lane >> 5;
  int bx = blockIdx.x, by = blockIdx.y, bz = blockIdx.z;
  ff_xcd_remap(bx, by, bz);
  c.tile = bx;
  c.h = by;
  c.b = bz;
  const int hkv = c.h / (Hq / Hkv);
  c.rbase = ((int64_t)c.b * Hq + c.h) * S;
  c.qbase = c.rbase * FF_D;
  c.kbase = (((int64_t)c.b * Hkv + hkv) * S) * FF_D;
  return c;
}

// D-layout row of accumulator register r (32x32 MFMA result; col = l31) in
// the 32-row subtile that starts at `base`.  A macro, not a function: the sum
// then keeps the association and no-overflow facts of the written-out
// formula, which the address folding of the row stores depends on.
#define ff_drow(base, r, half) ((base) + ((r) & 3) + 8 * ((r) >> 2) + 4 * (half))

// Tile LDS swizzle (guide G4): XOR the 16-byte slot (byte bits 4-7) with
// g(row) = ((row & 3) << 2) | ((row >> 2) & 3) — fa32_lds_map.h
DEV int ff_kswz(int byte_off) { return ff_map_swz(byte_off); }

// Block-cooperative staging of a [ROWS][128] bf16 tile, row-major + ff_kswz,
// by THREADS threads.  Thread tid moves chunk j = the 8 elements at
// e = ff_chunk<THREADS>(j, tid): ff_chunk_load (global -> register) and
// ff_chunk_store (register -> swizzled LDS).  ff_stage does both, chunk by
// chunk, for one tile.  A kernel that stages K and V interleaved, or puts
// compute between the loads and the stores (the forward's double buffer),
// loops over the two halves itself and keeps its staging registers in plain
// local arrays: handed to a helper by reference they are promoted to
// registers in a later pass and the kernel schedules differently.
#define FF_STAGE_CHUNKS(ROWS, THREADS) ((ROWS) * FF_D / ((THREADS) * 8))
template <int THREADS>
DEV int ff_chunk(int j, int tid) { return ff_map_chunk(j, tid, THREADS); }
DEV ff_shortx8 ff_chunk_load(const unsigned short* g, int e) {
  return *reinterpret_cast<const ff_shortx8*>(g + e);
}
DEV void ff_chunk_store(ff_shortx8 v, unsigned short* l, int e) {
  *reinterpret_cast<ff_shortx8*>((char*)l + ff_map_chunk_byte(e)) = v;
}
template <int ROWS, int THREADS>
DEV void ff_stage(const unsigned short* __restrict__ g, unsigned short* l, int tid) {
#pragma unroll
  for (int j = 0; j < FF_STAGE_CHUNKS(ROWS, THREADS); ++j) {
    const int e = ff_chunk<THREADS>(j, tid);
    ff_chunk_store(ff_chunk_load(g, e), l, e);
  }
}

// Rows of one head of an o-shaped tensor (o, dout) in either layout: row r of
// head (b, h) starts at element base + r * stride.  [B,Hq,S,D]: the head's
// rows are D apart; [B,S,Hq,D]: they are Hq*D apart and the head picks a
// 128-element column band.  Block-uniform, so it lives in scalar registers.
struct ff_rows {
  int64_t base;
  int stride;
};
DEV ff_rows ff_o_rows(const ff_ctx& c, int Hq, int S, int bshd) {
  ff_rows r;
  r.stride = bshd ? Hq * FF_D : FF_D;
  r.base = bshd ? ((int64_t)c.b * S * Hq + c.h) * FF_D : c.qbase;
  return r;
}

// ff_stage's strided sibling: the tile's row i starts at g + i * stride
// (stride = FF_D is ff_stage itself).  LDS image identical to ff_stage's.
template <int ROWS, int THREADS>
DEV void ff_stage_rows(const unsigned short* __restrict__ g, int stride, unsigned short* l,
                       int tid) {
#pragma unroll
  for (int j = 0; j < FF_STAGE_CHUNKS(ROWS, THREADS); ++j) {
    const int e = ff_chunk<THREADS>(j, tid);
    const int ge = (e / FF_D) * stride + (e % FF_D);
    ff_chunk_store(ff_chunk_load(g, ge), l, e);
  }
}

// A-operand fragment: rows s2*32 + l31 of a swizzled [*x128] LDS tile,
// k = ks*16 + half*8 + e
DEV ff_shortx8 ff_afrag(const unsigned short* l, int s2, int ks, int l31, int half) {
  return *reinterpret_cast<const ff_shortx8*>((const char*)l +
                                              ff_map_frag(s2 * 32 + l31, ks, half));
}

// B-operand fragment of row `row` from a swizzled LDS tile:
// B[j=row][k = ks*16 + half*8 + e] (row index may exceed 64; swizzle is
// row-periodic mod 16 so any multiple of 16 rows works)
DEV ff_shortx8 ff_bfrag(const unsigned short* l, int row, int ks, int half) {
  return *reinterpret_cast<const ff_shortx8*>((const char*)l + ff_map_frag(row, ks, half));
}

// B-operand fragments of one row straight from global memory (the
// register-resident operand of a wave's own rows): row[ks*16 + half*8 + e]
DEV ff_shortx8 ff_row_frag(const unsigned short* __restrict__ row, int ks, int half) {
  return *reinterpret_cast<const ff_shortx8*>(row + ks * 16 + half * 8);
}
DEV void ff_row_frags(const unsigned short* __restrict__ row, ff_shortx8 (&f)[8], int half) {
#pragma unroll
  for (int ks = 0; ks < 8; ++ks) f[ks] = ff_row_frag(row, ks, half);
}

// Relayout a D-layout [rows][cols=l31] fp32 register block (2 subtiles of 32
// rows) into 4 B-operand fragments with lane-dim = former cols and
// contraction = former rows, in-register: v_cvt_pk_bf16_f32 pairs +
// two-operand permlane32_swap (guide T12: one swap fills both half-row words;
// no LDS round trip, no select, no divergent branch).
// Derivation (regs r: row_local = ff_drow(0, r, half)):
//   group g (16 rows): own regs g*8+0..3 -> row g*16 + (0..3)+4*half ("LO")
//                      own regs g*8+4..7 -> row g*16 + (8..11)+4*half ("HI")
//   B-frag wants row = g*16 + half*8 + e:
//     half=0: e0-3 = own LO, e4-7 = partner LO (their +4..7)
//     half=1: e0-3 = partner HI (their 8..11), e4-7 = own HI (12..15)
//   permlane32_swap(LO, HI) (result layout: ff_swap_other's comment) hands
//     half=0: r0 = own LO,     r1 = partner LO
//     half=1: r0 = partner HI, r1 = own HI
//   so the fragment is {r0 of word 0, r0 of word 1, r1 of word 0, r1 of
//   word 1} in BOTH halves: 2 swaps per 16-row group, 8 per tile.
// ff_cvt_pk is the packed convert alone, so the relayout probe's reference
// formulation (probes.hip) starts from the same words.
DEV unsigned ff_cvt_pk(float a, float b) {
  unsigned w;
  asm volatile("v_cvt_pk_bf16_f32 %0, %1, %2" : "=v"(w) : "v"(a), "v"(b));
  return w;
}
DEV void ff_relayout(const ff_floatx16 st[2], ff_shortx8 pb[4]) {
#pragma unroll
  for (int s2 = 0; s2 < 2; ++s2) {
#pragma unroll
    for (int g = 0; g < 2; ++g) {
      const unsigned lo0 = ff_cvt_pk(st[s2][g * 8 + 0], st[s2][g * 8 + 1]);
      const unsigned lo1 = ff_cvt_pk(st[s2][g * 8 + 2], st[s2][g * 8 + 3]);
      const unsigned hi0 = ff_cvt_pk(st[s2][g * 8 + 4], st[s2][g * 8 + 5]);
      const unsigned hi1 = ff_cvt_pk(st[s2][g * 8 + 6], st[s2][g * 8 + 7]);
      auto w0 = __builtin_amdgcn_permlane32_swap(lo0, hi0, false, false);
      auto w1 = __builtin_amdgcn_permlane32_swap(lo1, hi1, false, false);
      ff_intx4 frag = (ff_intx4){(int)w0[0], (int)w1[0], (int)w0[1], (int)w1[1]};
      pb[s2 * 2 + g] = *reinterpret_cast<ff_shortx8*>(&frag);
    }
  }
}

// Causal mask of a D-layout 64-row tile, applied by the backward kernels on
// their diagonal tiles only (a wave-uniform branch), as a pre-pass over the
// raw scores: the masked registers of st become -inf, and the one exp2 / dS
// body that every tile runs turns them into P = 0, dS = 0.
// row = the element's tile row LESS this lane's 4*half, a compile-time
// constant per register, so the mask is one compare of a constant against a
// per-lane limit and no index arithmetic.
//   ABOVE: rows > lim are masked (fa2_dq: kv > q);
//   else : rows < lim are masked (fa2_dv / fa2_dk: q < kv).
// Why -inf BEFORE the fma gives the bits that "x = -inf after it" gave: the
// body computes x = fma(st, scale2, -lse2) with scale2 = scale * log2(e) > 0
// (the fa_bwd2 binding refuses a scale that is not positive and finite; the
// forward masks after scaling and takes any), so -inf * scale2 = -inf, and
// lse2 is finite: an
// active row always holds its own diagonal element, so its logsumexp is the
// log of a positive sum, never -inf, and +inf or a finite value leaves
// -inf - lse2 = -inf.  Then exp2(-inf) = +0 exactly as before.  (Only a NaN
// lse, with which the row's gradients are NaN already, would differ.)
template <bool ABOVE>
DEV void ff_mask(ff_floatx16 (&st)[2], int lim) {
#pragma unroll
  for (int s2 = 0; s2 < 2; ++s2)
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int row = ff_drow(s2 * 32, r, 0);
      if (ABOVE ? row > lim : row < lim) st[s2][r] = -INFINITY;
    }
}

// 8 tr reads (4 ks x 2) of a TRANSPOSED A-operand from a swizzled 64x128
// tile: fragment[lane-dim = ds*32 + l31][k = ks*16 + half*8 + e] is
// ff_cat(t[ks][0], t[ks][1]).  Probe-measured ds_read_b64_tr_b16 semantics
// (tools/tr_probe_check.py, which runs THIS function): a 4x4 transpose
// within each aligned 4-lane group,
//   OUT[l&15][j] = IN[4j + ((l&15)>>2)][l&3]   per 16-lane group,
// so lane y reads tile row rbase + ((y&15)>>2) at byte column
// cbase + (y&3)*4 elems, and the HW hands lane l the column ds*32 + l31 of
// rows rbase..rbase+3. Two reads (rbase, rbase+4) fill the 8 k elems; ks
// walks rows in +16 steps = +4096 bytes, which commutes with the bits-4..7
// row swizzle (it reads row & 15 only); rbase+4 changes it, hence the second
// address register.  The addresses are ff_map_tr (fa32_lds_map.h).
// `l15` is the lane id mod 16: only its bits 0-3 are read (bit 4 comes in
// through l31, bit 5 through half), so lane or tid may be passed unmasked.
DEV void ff_tr_read8(const unsigned short* tile, int ds, int l15, int l31, int half,
                     ff_shortx4 (&t)[4][2]) {
  static_assert(FF_MAP_KS_BYTES == 4096, "the offset: immediates below step 16 rows");
  const int a0 = ff_map_tr(ds, l15, l31, half, 0);  // tile rows half*8 + 0..3
  const int a1 = ff_map_tr(ds, l15, l31, half, 1);  // tile rows half*8 + 4..7
  ff_lds_p b0 = (ff_lds_p)((const char*)tile + a0);
  ff_lds_p b1 = (ff_lds_p)((const char*)tile + a1);
  // ONE asm statement for all 8 reads + the drain: with separate
  // statements the compiler may interpose copies of t between a read
  // and the waitcnt, capturing the register BEFORE the LDS data lands
  // (observed as run-to-run nondeterminism in O). Earlyclobber outputs
  // keep the async dsts from aliasing the address registers.
  asm volatile(
      "ds_read_b64_tr_b16 %0, %8 offset:0\n\t"
      "ds_read_b64_tr_b16 %1, %9 offset:0\n\t"
      "ds_read_b64_tr_b16 %2, %8 offset:4096\n\t"
      "ds_read_b64_tr_b16 %3, %9 offset:4096\n\t"
      "ds_read_b64_tr_b16 %4, %8 offset:8192\n\t"
      "ds_read_b64_tr_b16 %5, %9 offset:8192\n\t"
      "ds_read_b64_tr_b16 %6, %8 offset:12288\n\t"
      "ds_read_b64_tr_b16 %7, %9 offset:12288\n\t"
      "s_waitcnt lgkmcnt(0)"
      : "=&v"(t[0][0]), "=&v"(t[0][1]), "=&v"(t[1][0]), "=&v"(t[1][1]),
        "=&v"(t[2][0]), "=&v"(t[2][1]), "=&v"(t[3][0]), "=&v"(t[3][1])
      : "v"(b0), "v"(b1));
}

DEV ff_shortx8 ff_cat(const ff_shortx4 a, const ff_shortx4 b) {
  ff_shortx8 r;
#pragma unroll
  for (int x = 0; x < 4; ++x) { r[x] = a[x]; r[4 + x] = b[x]; }
  return r;
}

// Epilogue: a 4 x floatx16 D-layout accumulator (rows = d, col = this
// lane's output row) stored as one bf16 row: row[d] = acc[d] (* mul).
DEV void ff_store_elem(unsigned short* __restrict__ row, int ds, int r, int half, float x) {
  row[ff_drow(ds * 32, r, half)] = f32_to_bf16(x);
}
// SCALE = false stores acc unscaled (mul unused).
template <bool SCALE = true>
DEV void ff_store_row(unsigned short* __restrict__ row, const ff_floatx16 (&acc)[4],
                      float mul, int half) {
#pragma unroll
  for (int ds = 0; ds < 4; ++ds)
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      if constexpr (SCALE) ff_store_elem(row, ds, r, half, acc[ds][r] * mul);
      else ff_store_elem(row, ds, r, half, acc[ds][r]);
    }
}
