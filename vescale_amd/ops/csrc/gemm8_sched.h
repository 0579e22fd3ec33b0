// Issue slots and counted vector-memory waits of the gemm8 region-rotation
// schedules (gemm8.hip: rot, its read-ahead form RA, rot8, rot9), as plain
// C++: the kernels call these functions, and tests/gemm8_wait_model.cpp
// includes the same header and walks one wave's queue of outstanding loads on
// the host.
//
// A K-tile t is staged in four regions per operand buffer:
//   A q0 / A q1   rows 0-63 / 64-127 of both 128-row A halves
//   B h0 / B h1   the two 128-row B halves
// and every region takes 2 global_load_lds per thread.  Tile t lives in A
// buffer g8s_abuf(t) and in B buffer g8s_bbuf(rot9, t).  During tile t (4
// phases p = 0..3) phases 0,1 read A q0, phases 2,3 read A q1 and every phase
// reads B (waves with bh = 0 read h0, the others h1).  RA issues the reads of
// a phase one phase early (after the previous phase's MFMA burst).
//
// vmcnt counts a wave's outstanding loads and retires them in issue order, so
// a wait vmcnt(n) guarantees everything but the n youngest loads has landed.
// The steady-state counts below are the ones derived in gemm8.hip.  They
// assume that the slots younger than the region being waited for were all
// issued.  Near the end of K they were not (there is no tile ntile to
// prefetch), the queue is shorter, and the same count would let the needed
// region stay in flight.  The TAIL RULE: wherever a slot that the steady
// count allows to stay outstanding was not issued, the count drops by that
// slot's loads.  Every function takes ntile so that the rule is part of the
// table and not of the kernels.
#pragma once

#if defined(__HIPCC__) || defined(__CUDACC__)
#define G8S_FN __host__ __device__ constexpr
#else
#define G8S_FN constexpr
#endif

enum G8Sched { G8S_ROT = 0, G8S_RA = 1, G8S_ROT8 = 2, G8S_ROT9 = 3 };

enum G8Region { G8S_AQ0 = 1, G8S_AQ1 = 2, G8S_BH0 = 4, G8S_BH1 = 8 };
#define G8S_LOADS_PER_REGION 2

// One issue slot: the regions (G8Region bits) of K-tile `tile` it loads, in
// the order B h0, B h1, A q0, A q1.  tile < 0: the slot stays empty.
struct G8Slot {
  int tile;
  int regions;
};

G8S_FN int g8s_abuf(int tile) { return tile & 1; }
G8S_FN int g8s_bbuf(bool rot9, int tile) { return rot9 ? tile % 3 : tile & 1; }

// K-tile counts the host guards of gemm_tn8 let through
G8S_FN bool g8s_ntile_ok(G8Sched s, bool u2, int ntile) {
  if (s == G8S_ROT8 || s == G8S_ROT9) return ntile >= 4 && ntile % 2 == 0;
  return ntile >= 1 && (!u2 || ntile % 2 == 0);
}

// Tiles the prologue stages whole and drains (vmcnt(0) + barrier) before the
// loop: tile 0 for rot/RA, tiles 0 and 1 for rot8/rot9.
G8S_FN int g8s_prologue_drained(G8Sched s) { return s == G8S_ROT8 || s == G8S_ROT9 ? 2 : 1; }

// ---- rot and RA: 4 phases per tile -----------------------------------------
// After the drained tile 0 the prologue issues tile 1 as slots i = 0..2,
// undrained: B h0+h1, A q0, A q1.
G8S_FN G8Slot g8s_rot_prologue_slot(int i, int ntile) {
  if (ntile <= 1) return {-1, 0};
  return {1, i == 0 ? (G8S_BH0 | G8S_BH1) : (i == 1 ? G8S_AQ0 : G8S_AQ1)};
}

// Slot of phase p of tile kt (the same for rot and RA):
//   p0: B(kt+1) h0+h1   p1: A(kt+1) q1   p2: A(kt+2) q0   p3: nothing
// kt = 0 issues no tile 1 (the prologue did).
G8S_FN G8Slot g8s_rot_slot(int p, int kt, int ntile) {
  if (p == 0 && kt >= 1 && kt + 1 < ntile) return {kt + 1, G8S_BH0 | G8S_BH1};
  if (p == 1 && kt >= 1 && kt + 1 < ntile) return {kt + 1, G8S_AQ1};
  if (p == 2 && kt + 2 < ntile) return {kt + 2, G8S_AQ0};
  return {-1, 0};
}

// Count of the wait that gates the reads of phase p of tile kt; < 0: no wait.
// A wave's wait covers its own loads, and all eight waves fill every region,
// so the kernels put a barrier between the wait and those reads: rot executes
// it at the end of the phase before, in front of that phase's closing barrier
// (the queue does not change in between, so the counts are those of the
// phase's start); RA executes it at the start of phase p and reads ahead after
// the phase's first barrier.
//   rot, steady:  p0 vmcnt(4)  youngest allowed: A(kt)q1, A(kt+1)q0
//                 p2 vmcnt(8)  youngest: A(kt+1)q0, B(kt+1) x2, A(kt+1)q1
//        last tile (kt + 1 == ntile): A(kt+1)q0 was never issued and p0, p1
//        issue nothing:  p0 vmcnt(2) (only A(kt)q1 may stay),  p2 vmcnt(0)
//   RA,  steady:  p1 vmcnt(6)  gates the read-ahead of A(kt)q1;  youngest:
//                              A(kt+1)q0, B(kt+1) x2
//                 p3 vmcnt(4)  gates the read-ahead of A(kt+1)q0 and B(kt+1);
//                              youngest: A(kt+1)q1, A(kt+2)q0
//        p3 before the last tile (kt + 2 == ntile): no A(kt+2)q0: vmcnt(2)
//        p1 of the last tile: nothing younger than A(kt)q1:       vmcnt(0)
G8S_FN int g8s_rot_wait(bool ra, int p, int kt, int ntile) {
  if (!ra) {
    if (kt < 1) return -1;
    const bool last = kt + 1 == ntile;
    if (p == 0) return last ? 2 : 4;
    if (p == 2) return last ? 0 : 8;
    return -1;
  }
  if (p == 1 && kt >= 1) return kt + 1 == ntile ? 0 : 6;
  if (p == 3) return kt + 2 == ntile ? 2 : 4;
  return -1;
}

// ---- rot8 and rot9: 8 phases gp = 0..7 per pair of tiles (T, T+1), T even --
// rot8:  gp0 A(T+1)q1  gp1 B(T+1)h0  gp2 B(T+1)h1  gp3 A(T+2)q0
//        gp4 A(T+2)q1  gp5 B(T+2)h0  gp6 B(T+2)h1  gp7 A(T+3)q0
// rot9 (B in three buffers) stages B one tile further ahead:
//        gp1 B(T+2)h0  gp2 B(T+2)h1  gp5 B(T+3)h0  gp6 B(T+3)h1
// T = 0 issues no tile 1 (the prologue did).
G8S_FN G8Slot g8s_rot89_slot(bool rot9, int gp, int T, int ntile) {
  const int bstep = rot9 ? 1 : 0;
  int tile = -1, regions = 0;
  switch (gp) {
    case 0: tile = T >= 2 ? T + 1 : -1; regions = G8S_AQ1; break;
    case 1: tile = rot9 || T >= 2 ? T + 1 + bstep : -1; regions = G8S_BH0; break;
    case 2: tile = rot9 || T >= 2 ? T + 1 + bstep : -1; regions = G8S_BH1; break;
    case 3: tile = T + 2; regions = G8S_AQ0; break;
    case 4: tile = T + 2; regions = G8S_AQ1; break;
    case 5: tile = T + 2 + bstep; regions = G8S_BH0; break;
    case 6: tile = T + 2 + bstep; regions = G8S_BH1; break;
    case 7: tile = T + 3; regions = G8S_AQ0; break;
    default: break;
  }
  if (tile < 0 || tile >= ntile) return {-1, 0};
  return {tile, regions};
}

// Waits gate the reads of gp0 and gp4 of every pair but the first (tiles 0 and
// 1 were drained by the prologue); executed, like rot's, in front of the
// closing barrier of the phase before.
//   rot8, steady: vmcnt(2): only the slot of the phase before may stay.
//   rot9, steady: vmcnt(6): the three slots before may stay; the A quarters
//         needed are the fourth and fifth youngest, B is older still.
//   last pair (T + 2 == ntile): gp1..gp3 (rot9), gp3 (rot8) issue nothing, so
//         at gp4 the youngest loads ARE the ones tile T+1 is read from:
//         vmcnt(0).  gp0 keeps its count: the slots it lets stay (gp7 for
//         rot8; gp5..gp7 for rot9) were issued by the pair before.
G8S_FN int g8s_rot89_wait(bool rot9, int gp, int T, int ntile) {
  if (T < 2 || (gp != 0 && gp != 4)) return -1;
  if (gp == 4 && T + 2 >= ntile) return 0;
  return rot9 ? 6 : 2;
}
