// FP8 dense TN GEMM for gfx950 and the quantiser kernels that feed it.
//
//   C[M,N] (bf16) = (A[M,K] . B[N,K]^T) * scale_a * scale_b
//
// A is e4m3 or e5m2 (template parameter AFMT: 0 / 1, the format selector of
// the matrix instruction), B is e4m3, both row-major with K innermost, fp32
// accumulation, the two per-tensor scales read from device memory in the
// epilogue (no host sync: the launch is capturable).  Requires M % 256 == 0,
// N % 256 == 0, K % 128 == 0.
//
// Geometry.  256 x 256 C tile, K-tiles of 128 fp8 = 128 BYTES per row, 8 waves
// (2 along M x 4 along N), per-wave C = 128 x 64.  A K-tile row has the byte
// length of gemm8.hip's (64 bf16), so the staging is that file's: half-tiles
// of 128 rows x 128 B = 16 KiB, two global_load_lds (16 B) per thread per
// half, two buffers per operand = 128 KiB of LDS, the LDS side linear and the
// swizzle applied to the global source address.  The schedule is gemm8's
// region rotation ("rot", four phases per K-tile, counted vmcnt waits, per-
// phase barrier pairs) and its slot / wait tables are the ones of
// gemm8_sched.h, which tests/gemm8_wait_model.cpp walks: the regions, their
// loads per thread and their lifetimes are the same (below).  The pipeline is
// two K-tiles deep: tile 0 is drained by the prologue, tile 1 meets the first
// counted wait, tile 2 the first steady one.
//
// Matrix instruction: v_mfma_f32_16x16x128_f8f6f4, 8 per phase and wave where
// gemm8 issues 16 of 16x16x32 bf16: the same bytes, twice the products.  Its
// block-scale arguments are 0, 0: the compiler then emits the unscaled form,
// whose block scale is the neutral 2^0.  The product is computed TRANSPOSED:
// the instruction's first operand is the B fragment (16 rows of B = 16 columns
// of C), its second the A fragment, so a lane's four results
//   acc[r],  lane = (g = lane >> 4, m = lane & 15):  C row m, B-fragment row 4g + r
// lie along a row of C.  B-fragment f (0..3 of the wave's 64 columns) reads
// its 16 rows from tile rows
//   brow(f, i) = 32 (f >> 1) + 8 (i >> 2) + 4 (f & 1) + (i & 3),   i = lane & 15
// so the results of fragments 2p and 2p + 1 in one lane are the 8 consecutive
// columns 32p + 8g .. + 7 of one C row: one 16-byte store of 8 bf16, each
// scaled in fp32 and rounded once.
//
// Phases of K-tile kt, p = 2 * mh + pair:  A fragments 4 mh .. 4 mh + 3 (rows
// 64 mh .. + 63 of the wave's 128) x B fragments 2 pair, 2 pair + 1.  So
//   A q0 (rows 0-63 of both halves)   last read p1
//   A q1 (rows 64-127)                last read p3
//   B h0 / h1 (the 128-row halves)    last read p3
// which are the lifetimes gemm8_sched.h's rot tables assume.
//
// K ordering.  Every instruction contracts over all 128 bytes of a row.  A
// lane (kg = lane >> 4) supplies 32 of them per operand, and any assignment of
// the row's eight 16-byte chunks to (kg, first / second half of the register
// operand) is correct as long as A and B use the same one.  Used here:
//   chunk(kg, h) = 4 (kg >> 1) + (kg & 1) + 2 h          h = 0, 1
// i.e. kg 0..3 read chunks {0,2}, {1,3}, {4,6}, {5,7}: two ds_read_b128 each.
//
// LDS image and banks (64 banks of 4 B; rules as written in fa32_lds_map.h).
// Byte offset of (row, chunk c) in a half-tile:
//   row * 128 + ((c ^ s(row)) << 4),   s(row) = ((row >> 1) & 7) ^ (((row >> 4) & 1) << 1)
// (f8_swz: byte bits 4-6 ^= bits 8-10, bit 5 ^= bit 11).  Two rows are 256 B =
// all 64 banks, so a 16-byte slot's banks are fixed by u(row, c) =
// 8 (row & 1) + (c ^ s(row)), 16 values; a ds_read_b128 is served in groups of
// 16 lanes and is conflict-free when a group's 16 u are distinct.
//   - A fragment: lane i reads row 16 f + i.  Over i = 0..15 (row & 1, s) takes
//     all 16 values (the bit-4 term is one constant), so 16 lanes that read one
//     chunk c are conflict-free.
//   - B fragment: rows brow(f, i) = {0-3, 8-11, 16-19, 24-27} + 4 (f & 1) +
//     32 (f >> 1).  Without the bit-4 term rows 16 apart would share s; with it
//     row >> 1 = {0,1, 4,5, 8,9, 12,13} maps to s = {0,1, 4,5, 2,3, 6,7}:
//     again all 16 (row & 1, s).
//   - the hardware's groups are not lanes 0-15 but {0-3, 12-15, 20-27},
//     {4-11, 16-19, 28-31} and both + 32: 8 lanes of one kg and 8 of kg ^ 1.
//     Lanes i in {0-3, 12-15} carry one set S of four s values and lanes 4-11
//     the complement (A: S = {0,1,6,7} or {2,3,4,5}; B the same two sets), and
//     both are closed under ^ 1.  kg and kg ^ 1 read chunks c and c ^ 1 (that
//     is what the K ordering above is chosen for), so the group's slots are
//     c ^ S and (c ^ 1) ^ ~S = c ^ ~S: disjoint.  Conflict-free under either
//     grouping; with the natural order chunk = 2 kg + h the two sets would
//     meet (c ^ 2 maps S onto ~S) and every read would take two passes.
//   - staging: the LDS side of global_load_lds is linear (lane * 16 B).
// The swizzle permutes 16-byte chunks inside a 128-byte row, so the global
// side still reads whole rows.
//
// Resources (-Rpass-analysis=kernel-resource-usage, gfx950), no scratch in any
// kernel of this file:
//   gemm_fp8_tn_e4m3 / _e5m2   250 VGPRs, 0 AGPRs, 32 SGPRs, 131072 B LDS
//   fp8_amax_bf16               14 VGPRs, 20 SGPRs, 16 B LDS
//   fp8_quantize_e4m3 / _e5m2   64 VGPRs, 34 SGPRs, 4352 B LDS
#pragma once
#include "common.h"
#include "gemm8_sched.h"

#define F8_BM 256
#define F8_BN 256
#define F8_BK 128                 // fp8 elements = bytes of a tile's K row
#define F8_THREADS 512
#define F8_HALF (128 * F8_BK)     // bytes of a 128-row half-tile
#define F8_E4M3_MAX 448.f
#define F8_E5M2_MAX 57344.f

typedef float f8_floatx4 __attribute__((ext_vector_type(4)));
typedef int f8_intx4 __attribute__((ext_vector_type(4)));
typedef int f8_intx8 __attribute__((ext_vector_type(8)));

DEV int f8_swz(int byte) {
  return byte ^ (((byte >> 8) & 7) << 4) ^ (((byte >> 11) & 1) << 5);
}

// stage `n` 8 KiB quarters (64 rows x 128 B each, from quarter q0) of one
// half-tile: one global_load_lds per thread and quarter.  Each lane loads the
// 16 bytes that belong at its linear LDS slot under the swizzle.
DEV void f8_stage(const unsigned char* g, int ld, unsigned char* lds_half, int q0, int n,
                  int tid) {
  const int wave = tid >> 6;
#pragma unroll
  for (int q = q0; q < q0 + n; ++q) {
    const int e = f8_swz((tid + q * F8_THREADS) * 16);  // the byte living at this slot
    unsigned char* lb = lds_half + (wave * 64 + q * F8_THREADS) * 16;  // wave base
    __builtin_amdgcn_global_load_lds(
        (const __attribute__((address_space(1))) void*)(g + (int64_t)(e >> 7) * ld + (e & 127)),
        (__attribute__((address_space(3))) void*)lb, 16, 0, 0);
  }
}

// one slot of gemm8_sched.h: the regions of K-tile s.tile into the buffers
// lAt / lBt ([half][16 KiB]) that tile lives in.  No __restrict__ on Ag, Bg,
// as in gemm8.hip's g8_issue.
DEV void f8_issue(G8Slot s, const unsigned char* Ag, const unsigned char* Bg, int K,
                  unsigned char (*lAt)[F8_HALF], unsigned char (*lBt)[F8_HALF], int tid) {
  if (s.tile < 0) return;
  const unsigned char* At = Ag + (int64_t)s.tile * F8_BK;
  const unsigned char* Bt = Bg + (int64_t)s.tile * F8_BK;
  if (s.regions & G8S_BH0) f8_stage(Bt, K, lBt[0], 0, 2, tid);
  if (s.regions & G8S_BH1) f8_stage(Bt + (int64_t)128 * K, K, lBt[1], 0, 2, tid);
#pragma unroll
  for (int q = 0; q < 2; ++q)
    if (s.regions & (q ? G8S_AQ1 : G8S_AQ0)) {
      f8_stage(At, K, lAt[0], q, 1, tid);
      f8_stage(At + (int64_t)128 * K, K, lAt[1], q, 1, tid);
    }
}

#define F8_VMCNT(n) asm volatile("s_waitcnt vmcnt(" #n ")")
DEV void f8_wait(int n) {  // the counts gemm8_sched.h's rot table produces
  if (n < 0) return;
  if (n >= 8) { F8_VMCNT(8); }
  else if (n >= 4) { F8_VMCNT(4); }
  else if (n >= 2) { F8_VMCNT(2); }
  else { F8_VMCNT(0); }
}

// operand fragment: 32 K bytes of `row` for lane group kg (K ordering above)
DEV f8_intx8 f8_frag(const unsigned char* half, int row, int kg) {
  const int b0 = row * F8_BK + ((((kg >> 1) << 2) | (kg & 1)) << 4);
  const f8_intx4 lo = *reinterpret_cast<const f8_intx4*>(half + f8_swz(b0));
  const f8_intx4 hi = *reinterpret_cast<const f8_intx4*>(half + f8_swz(b0 + 32));
  return __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7);
}

template <int AFMT>
DEV void f8_gemm_body(const unsigned char* A, const unsigned char* B,
                      unsigned short* __restrict__ C, const float* __restrict__ scale_a,
                      const float* __restrict__ scale_b, int M, int N, int K) {
  __shared__ __attribute__((aligned(16))) unsigned char lA[2][2][F8_HALF];  // [buf][m half]
  __shared__ __attribute__((aligned(16))) unsigned char lB[2][2][F8_HALF];  // [buf][n half]

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = tid >> 6;
  const int wm = wave >> 2;   // A half: C rows wm*128 .. +128
  const int wn = wave & 3;    // C cols wn*64 .. +64
  const int bh = wn >> 1;     // B half this wave reads
  const int li = lane & 15;
  const int kg = lane >> 4;

  // bijective XCD remap, as gemm8.hip
  int gx = gridDim.x, nwg = gx * (int)gridDim.y;
  int f = blockIdx.x + gx * blockIdx.y;
  {
    int q = nwg >> 3, r = nwg & 7;
    int xcd = f & 7, off = f >> 3;
    f = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + off;
  }
  const int bm = (f % gx) * F8_BM;
  const int bn = (f / gx) * F8_BN;
  const unsigned char* Ag = A + (int64_t)bm * K;
  const unsigned char* Bg = B + (int64_t)bn * K;

  // rows of this lane's fragments inside the half-tiles
  const int arow = li;                                            // + 16 * fragment
  const int brow = (wn & 1) * 64 + 8 * (li >> 2) + (li & 3);      // + 32 * pair + 4 * odd

  f8_floatx4 acc[8][4];
#pragma unroll
  for (int i = 0; i < 8; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = (f8_floatx4)(0.f);

  const int ntile = K / F8_BK;

  // prologue: tile 0 staged and drained; tile 1 issued in slot order, undrained
  f8_stage(Ag, K, lA[0][0], 0, 2, tid);
  f8_stage(Ag + (int64_t)128 * K, K, lA[0][1], 0, 2, tid);
  f8_stage(Bg, K, lB[0][0], 0, 2, tid);
  f8_stage(Bg + (int64_t)128 * K, K, lB[0][1], 0, 2, tid);
  asm volatile("s_waitcnt vmcnt(0)");
  __builtin_amdgcn_s_barrier();
#pragma unroll
  for (int i = 0; i < 3; ++i)
    f8_issue(g8s_rot_prologue_slot(i, ntile), Ag, Bg, K, lA[1], lB[1], tid);

  for (int kt = 0; kt < ntile; ++kt) {
    const int buf = kt & 1;
#pragma unroll
    for (int p = 0; p < 4; ++p) {
      const int mh = p >> 1, pair = p & 1;
      asm volatile("" ::: "memory");

      // (a) this phase's fragments: 12 ds_read_b128
      f8_intx8 af[4], bf[2];
#pragma unroll
      for (int i = 0; i < 4; ++i) af[i] = f8_frag(lA[buf][wm], (mh * 4 + i) * 16 + arow, kg);
#pragma unroll
      for (int j = 0; j < 2; ++j) bf[j] = f8_frag(lB[buf][bh], brow + 32 * pair + 4 * j, kg);

      // (b) this phase's prefetch slot (gemm8_sched.h): p0 B(kt+1) -> buf^1,
      // p1 A(kt+1) q1 -> buf^1, p2 A(kt+2) q0 -> buf (A(kt) q0 died at p1)
      f8_issue(g8s_rot_slot(p, kt, ntile), Ag, Bg, K, lA[p == 2 ? buf : buf ^ 1], lB[buf ^ 1],
               tid);

      // (c) lockstep barrier pair around the MFMA burst: no wave issues a
      // prefetch into a region while another wave's reads of it are pending
      __builtin_amdgcn_s_barrier();
      asm volatile("s_waitcnt lgkmcnt(0)");
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
          acc[mh * 4 + i][pair * 2 + j] = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(
              bf[j], af[i], acc[mh * 4 + i][pair * 2 + j], /*B: e4m3*/ 0, AFMT, 0, 0, 0, 0);

      // (d) the counted wait that gates the NEXT phase's reads, published to
      // the other waves by the closing barrier (a wave's wait covers only its
      // own loads, and all eight waves fill every region)
      const int nkt = kt + (p == 3 ? 1 : 0);
      if (nkt < ntile) f8_wait(g8s_rot_wait(false, (p + 1) & 3, nkt, ntile));
      asm volatile("" ::: "memory");
      __builtin_amdgcn_s_barrier();
    }
  }

  // epilogue: scale in fp32, round once, 8 bf16 = 16 bytes per store
  const float s = scale_a[0] * scale_b[0];
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const int row = bm + wm * 128 + i * 16 + li;
#pragma unroll
    for (int pr = 0; pr < 2; ++pr) {
      short8v v;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        v[r] = (short)f32_to_bf16(acc[i][2 * pr][r] * s);
        v[4 + r] = (short)f32_to_bf16(acc[i][2 * pr + 1][r] * s);
      }
      const int col = bn + wn * 64 + 32 * pr + 8 * kg;
      *reinterpret_cast<short8v*>(C + (int64_t)row * N + col) = v;
    }
  }
}

extern "C" __global__ void __launch_bounds__(F8_THREADS, 1)
gemm_fp8_tn_e4m3(const unsigned char* A, const unsigned char* B, unsigned short* C,
                 const float* scale_a, const float* scale_b, int M, int N, int K) {
  f8_gemm_body<0>(A, B, C, scale_a, scale_b, M, N, K);
}
extern "C" __global__ void __launch_bounds__(F8_THREADS, 1)
gemm_fp8_tn_e5m2(const unsigned char* A, const unsigned char* B, unsigned short* C,
                 const float* scale_a, const float* scale_b, int M, int N, int K) {
  f8_gemm_body<1>(A, B, C, scale_a, scale_b, M, N, K);
}

// ---------------------------------------------------------------------------
// amax: out[0] = max |x| over a bf16 tensor of n elements (n % 8 == 0), finite
// inputs.  One streaming pass of 16-byte loads.  |x| of a bf16 is its bit
// pattern without the sign, and for finite non-negative floats the order of
// the values is the order of the patterns as unsigned integers, so the whole
// reduction runs on integers and the blocks combine with one vector atomic
// max per block on the fp32 pattern, into a cell that fp8_amax_clear zeroed
// (a kernel, not a memset, so that the pair can be captured into a graph).
// ---------------------------------------------------------------------------
#define F8Q_AMAX_THREADS 256

extern "C" __global__ void fp8_amax_clear(unsigned int* out) { out[0] = 0u; }

extern "C" __global__ void __launch_bounds__(F8Q_AMAX_THREADS)
fp8_amax_bf16(const unsigned short* __restrict__ x, unsigned int* out, int64_t n8) {
  __shared__ unsigned int part[F8Q_AMAX_THREADS / WAVE];
  unsigned int m = 0u;
  const int64_t stride = (int64_t)gridDim.x * F8Q_AMAX_THREADS;
  for (int64_t i = (int64_t)blockIdx.x * F8Q_AMAX_THREADS + threadIdx.x; i < n8; i += stride) {
    const f8_intx4 v = reinterpret_cast<const f8_intx4*>(x)[i];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const unsigned int w = (unsigned int)v[j];
      m = max(m, max(w & 0x7fffu, (w >> 16) & 0x7fffu));
    }
  }
#pragma unroll
  for (int off = WAVE / 2; off > 0; off >>= 1) m = max(m, (unsigned int)__shfl_xor((int)m, off, WAVE));
  if ((threadIdx.x & (WAVE - 1)) == 0) part[threadIdx.x / WAVE] = m;
  __syncthreads();
  if (threadIdx.x == 0) {
#pragma unroll
    for (int w = 1; w < F8Q_AMAX_THREADS / WAVE; ++w) m = max(m, part[w]);
    if (m) atomicMax(out, m << 16);
  }
}

// ---------------------------------------------------------------------------
// cast with optional transpose: q[R,C] and / or qt[C,R] (fp8, FMT 0 = e4m3,
// 1 = e5m2) from ONE read of x[R,C] (bf16):
//   q = cast_rne(clamp(float(x) / scale, -fmt_max, fmt_max))
// a true fp32 division and an explicit clamp in front of the convert.
// R % 64 == 0, C % 64 == 0.
//
// One wave moves one 64 x 64 tile.  Lane t owns rows 4 rb .. + 3 (rb = t >> 2)
// x columns 16 cb .. + 15 (cb = t & 3): eight 16-byte loads (four lanes read
// the 128 bytes of a tile row), 64 converts, and for q four 16-byte stores.
// For qt the lane packs, per column, its four rows' bytes into one dword and
// writes the 16 dwords into the transposed LDS image T[col][row]:
//   dword index of (col, rb) = 16 col + 16 (col >> 4) + rb
// rows of 64 B plus one extra 64-byte step per 16 columns.  At step i the 64
// lanes write columns 16 cb + i: without the step the four cb would fall on
// the same 16 banks (16 columns = 256 dwords = 0 mod 64), with it they take
// the four bank quarters: 64 dwords on 64 banks.  The image is then read back
// by rows in 16-byte chunks (lane t: column (t >> 2) + 16 j, rows 16 (t & 3)
// .. + 15), 256 contiguous dwords per instruction, and stored in 16-byte
// chunks to qt.
// ---------------------------------------------------------------------------
#define F8Q_T_DWORDS (64 * 16 + 4 * 16)

template <int FMT>
DEV unsigned int f8q_pack4(float a, float b, float c, float d) {
  int v = 0;
  if constexpr (FMT == 0) {
    v = __builtin_amdgcn_cvt_pk_fp8_f32(a, b, v, false);
    v = __builtin_amdgcn_cvt_pk_fp8_f32(c, d, v, true);
  } else {
    v = __builtin_amdgcn_cvt_pk_bf8_f32(a, b, v, false);
    v = __builtin_amdgcn_cvt_pk_bf8_f32(c, d, v, true);
  }
  return (unsigned int)v;
}

template <int FMT>
DEV void f8q_body(const unsigned short* __restrict__ x, const float* __restrict__ scale,
                  unsigned char* __restrict__ q, unsigned char* __restrict__ qt, int R, int C) {
  __shared__ __attribute__((aligned(16))) unsigned int T[F8Q_T_DWORDS];
  constexpr float FMAX = FMT == 0 ? F8_E4M3_MAX : F8_E5M2_MAX;
  const int t = threadIdx.x, rb = t >> 2, cb = t & 3;
  const int r0 = blockIdx.y * 64, c0 = blockIdx.x * 64;
  const float sc = scale[0];

  unsigned int w[4][4];  // [row][4 columns each]
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const unsigned short* src = x + ((int64_t)(r0 + 4 * rb + r) * C + c0 + 16 * cb);
    float v[16];
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const short8v in = *reinterpret_cast<const short8v*>(src + 8 * h);
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const float y = bf16_to_f32((unsigned short)in[e]) / sc;
        v[8 * h + e] = fminf(fmaxf(y, -FMAX), FMAX);
      }
    }
#pragma unroll
    for (int k = 0; k < 4; ++k)
      w[r][k] = f8q_pack4<FMT>(v[4 * k], v[4 * k + 1], v[4 * k + 2], v[4 * k + 3]);
    if (q) {
      f8_intx4 o = {(int)w[r][0], (int)w[r][1], (int)w[r][2], (int)w[r][3]};
      *reinterpret_cast<f8_intx4*>(q + ((int64_t)(r0 + 4 * rb + r) * C + c0 + 16 * cb)) = o;
    }
  }
  if (!qt) return;  // uniform over the block

#pragma unroll
  for (int i = 0; i < 16; ++i) {
    const int sh = 8 * (i & 3);
    const unsigned int d = ((w[0][i >> 2] >> sh) & 0xffu) | (((w[1][i >> 2] >> sh) & 0xffu) << 8) |
                           (((w[2][i >> 2] >> sh) & 0xffu) << 16) |
                           (((w[3][i >> 2] >> sh) & 0xffu) << 24);
    T[16 * (16 * cb + i) + 16 * cb + rb] = d;
  }
  __syncthreads();
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int col = (t >> 2) + 16 * j, seg = t & 3;
    const f8_intx4 o = *reinterpret_cast<const f8_intx4*>(&T[16 * col + 16 * j + 4 * seg]);
    *reinterpret_cast<f8_intx4*>(qt + ((int64_t)(c0 + col) * R + r0 + 16 * seg)) = o;
  }
}

extern "C" __global__ void __launch_bounds__(WAVE)
fp8_quantize_e4m3(const unsigned short* x, const float* scale, unsigned char* q,
                  unsigned char* qt, int R, int C) {
  f8q_body<0>(x, scale, q, qt, R, C);
}
extern "C" __global__ void __launch_bounds__(WAVE)
fp8_quantize_e5m2(const unsigned short* x, const float* scale, unsigned char* q,
                  unsigned char* qt, int R, int C) {
  f8q_body<1>(x, scale, q, qt, R, C);
}
