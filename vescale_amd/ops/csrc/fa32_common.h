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
// Attribute of the kernels built on the direct staging below (forward, fa2_dq,
// fa2_dv / fa2_dk, the staging probe): compiled without the packed fp32 VALU
// ops (v_pk_{add,mul,fma}_f32); the scalar forms give the same bits.  Per
// kernel, not a build flag: every other kernel of the extension is compiled as
// before.  NOTES_FA32_STAGING.md has each kernel's time with and without it.
#define FF_NO_PK_F32 __attribute__((target("no-packed-fp32-ops")))
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
  int64_t rbase;         // ((b*Hq + h) * Sq): row base into lse / delta
  int64_t qbase, kbase;  // element base of this head in q-shaped / k-shaped tensors
};
// Sq rows per head in q, o, dout, lse, delta and dq, Sk in k and v.  The causal
// kernels are square and pass their S twice; only the FULL instantiations have
// two lengths.
DEV ff_ctx ff_prologue(int Hq, int Hkv, int Sq, int Sk) {
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
  c.rbase = ((int64_t)c.b * Hq + c.h) * Sq;
  c.qbase = c.rbase * FF_D;
  c.kbase = (((int64_t)c.b * Hkv + hkv) * Sk) * FF_D;
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

// The direct sibling of ff_stage_rows: the same tile, the same LDS image byte
// for byte, moved by global_load_lds_dwordx4 (16 bytes per lane, global -> LDS
// with no destination VGPR and no ds_write).  The LDS side of that load is
// linear (M0 = wave-uniform base, lane l lands at base + 16*l), so the swizzle
// sits on the source address: fa32_lds_map.h, "the SOURCE side".
// ASYNCHRONOUS: the call only issues the FF_ASYNC_LOADS(ROWS, THREADS) loads of
// this thread.  A tile is readable once every wave has passed ff_stage_wait()
// (its own loads have landed in LDS) and then a __syncthreads() of the
// kernel's (the other waves' have): the order gemm8.hip keeps, drain then
// barrier.  No barrier in here (README rule 3), and the caller keeps every wave
// of the block issuing, active or not: a wave that skips the call leaves its
// pieces of the tile stale.
// Inline asm, where gemm8.hip uses __builtin_amdgcn_global_load_lds: behind the
// builtin the compiler's wait-count pass treats every later LDS read as a
// reader of the pending load (it cannot tell the two buffers apart) and puts
// s_waitcnt vmcnt(0) in front of the first ds_read of the tile being computed,
// which is the wait the prefetch exists to avoid.  The asm keeps the load out
// of that scoreboard; ff_stage_wait is then the ONLY thing that orders it (rule
// 2's concern, with LDS as the destination: nothing may read the buffer before
// the wait and the barrier, and the "memory" clobbers keep the compiler from
// moving an LDS access across either statement).  The compiler's own counted
// vmcnt waits stay correct: the counter retires in order, so an unknown load
// in flight can only make one of them wait longer.  s_nop: one wait state
// between the SALU write of M0 and the load that reads it (at issue, so M0 is
// restored right behind it).
// One source offset per thread: the row of load i is (tid >> 4) + i *
// THREADS/16, THREADS/16 is a multiple of 16, the period of the swizzle, so
// load i reads ff_map_async_step further on.  The instruction offset stays 0
// (it would move the LDS side as well).
#define FF_ASYNC_LOADS(ROWS, THREADS) ((ROWS) * FF_MAP_ROW_BYTES / ((THREADS) * 16))
template <int ROWS, int THREADS>
DEV void ff_stage_async(const unsigned short* __restrict__ g, int stride, unsigned short* l,
                        int tid) {
  static_assert(THREADS % 256 == 0 && (ROWS * FF_MAP_ROW_BYTES) % (THREADS * 16) == 0,
                "whole 1 KiB pieces per wave, rows of later loads a multiple of 16 further");
  const int voff0 = ff_map_async_src(0, tid, THREADS, stride) * 2;  // bytes, >= 0
  const unsigned lbase = (unsigned)(uintptr_t)(__attribute__((address_space(3))) char*)l;
#pragma unroll
  for (int i = 0; i < FF_ASYNC_LOADS(ROWS, THREADS); ++i) {
    // the step goes into the 32-bit lane offset (one v_add), not into a scalar
    // base per load: 8 more 64-bit bases live across the forward's loop spill
    // SGPRs
    const int voff = voff0 + i * ff_map_async_step(THREADS, stride) * 2;
    const unsigned m0 =
        __builtin_amdgcn_readfirstlane(lbase + ff_map_async_base(i, tid, THREADS));
    unsigned keep;  // M0 is the compiler's: handed back as found
    asm volatile(
        "s_mov_b32 %0, m0\n\t"
        "s_mov_b32 m0, %3\n\t"
        "s_nop 0\n\t"
        "global_load_lds_dwordx4 %1, %2\n\t"
        "s_mov_b32 m0, %0"
        : "=&s"(keep)
        : "v"(voff), "s"(g), "s"(m0)
        : "memory");
  }
}
// Every direct load (and every other vector load) of this wave has landed:
// s_waitcnt vmcnt(0), expcnt and lgkmcnt left at "no wait".  The builtin also
// tells the compiler's wait-count pass that its own scoreboard is clean here;
// the empty asm keeps LDS accesses on their side of the wait.
DEV void ff_stage_wait() {
  __builtin_amdgcn_s_waitcnt(0x0F70);
  asm volatile("" ::: "memory");
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

// ---------------------------------------------------------------------------
// Packed-document ("contiguous segments") mask of the SEG instantiations.
// The documents of a batch row are the maximal runs of equal segment ids; the
// pre-pass below turns ids [B,S] into bounds [B,2,S]:
//   start[b][i] = first position of i's run, end[b][i] = one past its last.
// Key j is visible to query i iff start[i] <= j <= i, which is the same as
// j <= i < end[j].  Both rows are monotone non-decreasing in i, so the bound of
// a block's (or wave's) FIRST row is the minimum over its rows and that of its
// LAST row the maximum: tile skipping needs one scalar per block and two per
// wave, and the mask one integer per lane (its own row's start or end).
// ---------------------------------------------------------------------------
#define FF_SEG_THREADS 256
#define FF_SEG_NONE 0x7fffffff  // "no LAST seen yet" of the end scan

DEV const int* ff_seg_start(const int* __restrict__ bounds, int b, int S) {
  return bounds + (int64_t)b * 2 * S;
}
DEV const int* ff_seg_end(const int* __restrict__ bounds, int b, int S) {
  return bounds + ((int64_t)b * 2 + 1) * S;
}
// A tile index derived from the CONTENT of bounds, held to [lo, hi]: whatever
// the tensor holds, no address is formed from it outside the tiles the kernel
// without a mask would touch.
DEV int ff_seg_tile(int t, int lo, int hi) { return max(lo, min(t, hi)); }

// Inclusive block scan over FF_SEG_THREADS values in LDS (Hillis-Steele):
// MAX ? running maximum towards higher t : running minimum towards lower t.
template <bool MAX>
DEV int ff_seg_scan(int* l, int t, int x) {
  l[t] = x;
  __syncthreads();
#pragma unroll
  for (int off = 1; off < FF_SEG_THREADS; off <<= 1) {
    const int o = MAX ? t - off : t + off;
    const bool in = MAX ? o >= 0 : o < FF_SEG_THREADS;
    const int y = in ? l[o] : x;
    __syncthreads();
    x = MAX ? max(x, y) : min(x, y);
    l[t] = x;
    __syncthreads();
  }
  return x;
}

// The pre-pass.  grid (ceil(S / 256), B), 256 threads, one position each.
// A position is a run START when it is 0 or its id differs from the one
// before, and a run's LAST when it is S - 1 or the id after differs.  start is
// the running maximum of the START positions, end the running minimum (from
// the right) of LAST + 1.  A block first scans its own 256 positions; where
// its chunk holds no START at or before a position (no LAST at or after), the
// whole block walks the chunks before (after) it, 256 positions at a time,
// until one holds a flag: position 0 is always a START and S - 1 a LAST, so
// both walks end.  The walks are block-uniform (every thread reaches every
// barrier), read-only, and their length is the run's, in chunks.  No atomics:
// every output word is written once, by its own thread, from values that do
// not depend on the order blocks run in.
DEV void ff_seg_bounds(const int* __restrict__ ids, int* __restrict__ bounds, int S) {
  __shared__ int l[FF_SEG_THREADS];
  const int t = threadIdx.x, b = blockIdx.y;
  const int p0 = blockIdx.x * FF_SEG_THREADS;
  const int* row = ids + (int64_t)b * S;
  // is position i (0 <= i < S) a START / a LAST?
  auto is_start = [&](int i) { return i == 0 || row[i] != row[i - 1]; };
  auto is_last = [&](int i) { return i == S - 1 || row[i] != row[i + 1]; };

  const int i = p0 + t;
  const bool in = i < S;
  int st = ff_seg_scan<true>(l, t, (in && is_start(i)) ? i : -1);
  // l[0] after the scan is thread 0's own value: -1 iff p0 is no START, and
  // then every position up to the chunk's first START needs the walk
  int carry = -1;
  if (l[0] < 0) {
    // p0 > 0 here (position 0 is a START), so c >= 0 throughout
    for (int c = p0 - FF_SEG_THREADS; carry < 0; c -= FF_SEG_THREADS) {
      __syncthreads();
      ff_seg_scan<true>(l, t, is_start(c + t) ? c + t : -1);
      carry = l[FF_SEG_THREADS - 1];  // the chunk's last START, -1 if none
    }
  }
  st = max(st, carry);
  __syncthreads();

  int en = ff_seg_scan<false>(l, t, (in && is_last(i)) ? i + 1 : FF_SEG_NONE);
  // the chunk's last valid position holds FF_SEG_NONE iff it is no LAST, and then
  // it (and what precedes it back to the chunk's last LAST) needs the walk
  const int tail = min(FF_SEG_THREADS, S - p0) - 1;
  int ecarry = FF_SEG_NONE;
  if (l[tail] == FF_SEG_NONE) {
    // the tail is no LAST, so it is not S - 1 and the next chunk exists
    for (int c = p0 + FF_SEG_THREADS; ecarry == FF_SEG_NONE; c += FF_SEG_THREADS) {
      __syncthreads();
      const int j = c + t;
      ff_seg_scan<false>(l, t, (j < S && is_last(j)) ? j + 1 : FF_SEG_NONE);
      ecarry = l[0];  // the chunk's first LAST + 1, FF_SEG_NONE if none
    }
  }
  en = min(en, ecarry);
  if (in) {
    int* out = bounds + (int64_t)b * 2 * S;
    out[i] = st;
    out[S + i] = en;
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
