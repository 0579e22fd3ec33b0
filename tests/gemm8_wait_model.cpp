// Host model of the counted vector-memory waits of the gemm8 region-rotation
// schedules (built and run by tests/test_gemm8_wait_model.py).  Includes the
// table the kernels are built on, csrc/gemm8_sched.h, and walks ONE wave's
// queue of outstanding global_load_lds for every schedule and every K-tile
// count the host guards allow in 1..12:
//   - an issue slot pushes 2 loads per region it stages;
//   - a wait vmcnt(n) retires the oldest loads until at most n remain; what a
//     wave has retired is in LDS, but the other seven waves' shares of the
//     region are only known to be there once they have passed the same wait,
//     that is after the next barrier;
//   - every phase has a barrier before its MFMA burst and one closing it.  The
//     read-ahead form waits at the start of a phase and reads after the first
//     barrier; the others wait for the next phase's reads in front of the
//     closing barrier;
//   - a phase reads A q0 (phases 0,1) or A q1 (phases 2,3) and both B halves
//     of its K-tile; the read-ahead form performs the reads of a phase at the
//     end of the phase before (the prologue reads tile 0, phase 0).
// Conditions:
//   (a) a region read for tile kt holds tile kt, has no load in flight, and a
//       barrier lies between the wait that retired its loads and the read;
//   (b) a slot issues into a region only after the last phase that reads its
//       previous occupant: at least one phase later (the closing barrier of
//       the reading phase orders it), two for read-ahead, whose ds_reads are
//       drained by the lgkmcnt(0) of the phase after the one that issued them;
//       and never while loads of the previous occupant are still in flight.
// Every wave issues the same loads in the same order, so one queue stands for
// all eight.
//
// Two negative controls, each of which must report reads and exit 1:
//   --steady-only           the waits are taken from the table as if the end
//                           of K were far away (the steady loop's counts on
//                           every tile): the reads of the last tiles;
//   --waits-open-the-phase  every wait sits at the start of the phase whose
//                           reads it gates, with no barrier in between: every
//                           read that follows a counted wait.
// Exit status 0 = all hold; every failure prints a line.
#include <cstdio>
#include <cstring>
#include <deque>

#include "gemm8_sched.h"

namespace {

int failures = 0;
bool steady_only = false, waits_open = false;

struct Region {
  int tile = -1;         // K-tile whose data the region holds or is being sent
  int in_flight = 0;     // its loads not yet retired
  int unpublished = 0;   // retired by this wave, no barrier since
};

struct Sched {
  const char* name;
  G8Sched kind;
  bool u2;
};
const Sched SCHEDS[] = {{"rot", G8S_ROT, false},   // modes 2, 3, 4
                        {"rot-u2", G8S_ROT, true}, // mode 5
                        {"rot-ra", G8S_RA, false}, // mode 6
                        {"rot8", G8S_ROT8, false}, // mode 7
                        {"rot9", G8S_ROT9, false}};  // mode 8

const int KINDS[4] = {G8S_BH0, G8S_BH1, G8S_AQ0, G8S_AQ1};  // issue order in a slot
const char* kind_name(int k) {
  return k == G8S_AQ0 ? "A q0" : k == G8S_AQ1 ? "A q1" : k == G8S_BH0 ? "B h0" : "B h1";
}
// the one read table: does phase p of a tile read region kind k
bool phase_reads(int k, int p) { return k == G8S_AQ0 ? p < 2 : k == G8S_AQ1 ? p >= 2 : true; }

struct Walk {
  const Sched& s;
  int ntile;
  bool ra, rot9;
  Region regs[3][4];     // [buffer][index into KINDS]
  std::deque<Region*> fifo;
  int last_wait = -1, max_in_flight = 0;
  int fails = 0;

  Walk(const Sched& sc, int nt) : s(sc), ntile(nt), ra(sc.kind == G8S_RA), rot9(sc.kind == G8S_ROT9) {}

  Region& reg(int kind_idx, int tile) {
    const bool is_b = KINDS[kind_idx] == G8S_BH0 || KINDS[kind_idx] == G8S_BH1;
    return regs[is_b ? g8s_bbuf(rot9, tile) : g8s_abuf(tile)][kind_idx];
  }

  void fail(const char* what) {
    ++fails;
    ++failures;
    std::printf("FAIL %s ntile %d: %s\n", s.name, ntile, what);
  }

  void wait(int n) {
    if (n < 0) return;
    last_wait = n;
    while ((int)fifo.size() > n) {
      --fifo.front()->in_flight;
      ++fifo.front()->unpublished;
      fifo.pop_front();
    }
  }

  void barrier() {
    for (auto& buf : regs)
      for (Region& r : buf) r.unpublished = 0;
  }

  // phase g (global index; tile g / 4, phase g % 4) of the walk performs the
  // reads of logical phase lg
  void read(int lg) {
    const int kt = lg / 4, p = lg % 4;
    char buf[160];
    for (int k = 0; k < 4; ++k) {
      if (!phase_reads(KINDS[k], p)) continue;
      const Region& r = reg(k, kt);
      if (r.tile != kt) {
        std::snprintf(buf, sizeof buf, "tile %d p%d reads %s, which holds tile %d", kt, p,
                      kind_name(KINDS[k]), r.tile);
        fail(buf);
      } else if (r.in_flight) {
        std::snprintf(buf, sizeof buf, "tile %d p%d reads %s with %d loads in flight (last wait vmcnt(%d))",
                      kt, p, kind_name(KINDS[k]), r.in_flight, last_wait);
        fail(buf);
      } else if (r.unpublished) {
        std::snprintf(buf, sizeof buf,
                      "tile %d p%d reads %s straight after the wait vmcnt(%d) that retired it, no barrier between",
                      kt, p, kind_name(KINDS[k]), last_wait);
        fail(buf);
      }
    }
  }

  // last phase (global index) at which the walk reads region kind k of tile t
  int last_read_phase(int k, int t) const {
    int p = 3;
    while (!phase_reads(k, p)) --p;
    return 4 * t + p - (ra ? 1 : 0);
  }

  void issue(G8Slot slot, int g) {
    if (slot.tile < 0) return;
    char buf[200];
    if (slot.tile >= ntile) {
      std::snprintf(buf, sizeof buf, "phase %d issues tile %d, past the end of K", g, slot.tile);
      fail(buf);
      return;
    }
    for (int k = 0; k < 4; ++k) {
      if (!(slot.regions & KINDS[k])) continue;
      Region& r = reg(k, slot.tile);
      if (r.in_flight) {
        std::snprintf(buf, sizeof buf, "phase %d issues %s of tile %d over tile %d, still in flight", g,
                      kind_name(KINDS[k]), slot.tile, r.tile);
        fail(buf);
      }
      const int lag = ra ? 2 : 1;
      if (r.tile >= 0 && last_read_phase(KINDS[k], r.tile) + lag > g) {
        std::snprintf(buf, sizeof buf,
                      "phase %d issues %s of tile %d over tile %d, read until phase %d (needs %d phases)", g,
                      kind_name(KINDS[k]), slot.tile, r.tile, last_read_phase(KINDS[k], r.tile), lag);
        fail(buf);
      }
      r.tile = slot.tile;
      r.in_flight = G8S_LOADS_PER_REGION;
      for (int i = 0; i < G8S_LOADS_PER_REGION; ++i) fifo.push_back(&r);
    }
    if ((int)fifo.size() > max_in_flight) max_in_flight = (int)fifo.size();
  }

  void run() {
    const bool pair = s.kind == G8S_ROT8 || s.kind == G8S_ROT9;
    const int wait_ntile = steady_only ? 1 << 20 : ntile;
    for (int t = 0; t < g8s_prologue_drained(s.kind) && t < ntile; ++t)
      for (int k = 0; k < 4; ++k) reg(k, t).tile = t;
    if (!pair)
      for (int i = 0; i < 3; ++i) issue(g8s_rot_prologue_slot(i, ntile), -1);
    if (ra) read(0);
    for (int g = 0; g < 4 * ntile; ++g) {
      const int kt = g / 4, p = g % 4;
      const int T = kt & ~1, gp = g - 4 * T;
      auto table_wait = [&](int gg) {  // the wait that gates the reads of phase gg
        const int k2 = gg / 4, T2 = k2 & ~1;
        return pair ? g8s_rot89_wait(rot9, gg - 4 * T2, T2, wait_ntile)
                    : g8s_rot_wait(ra, gg % 4, k2, wait_ntile);
      };
      if (ra || waits_open) wait(table_wait(g));
      if (!ra) read(g);
      issue(pair ? g8s_rot89_slot(rot9, gp, T, ntile) : g8s_rot_slot(p, kt, ntile), g);
      barrier();
      if (ra && g + 1 < 4 * ntile) read(g + 1);
      if (!ra && !waits_open && g + 1 < 4 * ntile) wait(table_wait(g + 1));
      barrier();
    }
    if (!fails)
      std::printf("%s ntile %d: ok, at most %d loads in flight\n", s.name, ntile, max_in_flight);
  }
};

}  // namespace

int main(int argc, char** argv) {
  steady_only = argc > 1 && !std::strcmp(argv[1], "--steady-only");
  waits_open = argc > 1 && !std::strcmp(argv[1], "--waits-open-the-phase");
  for (const Sched& s : SCHEDS)
    for (int ntile = 1; ntile <= 12; ++ntile)
      if (g8s_ntile_ok(s.kind, s.u2, ntile)) Walk(s, ntile).run();
  if (failures) {
    std::printf("%d failures\n", failures);
    return 1;
  }
  std::printf("all checks passed\n");
  return 0;
}
