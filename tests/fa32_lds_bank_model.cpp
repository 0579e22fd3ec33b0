// Host check of the 32x32 flash family's LDS tile map (built and run by
// tests/test_fa32_lds_map.py).  Includes the address header the kernels are
// built on, enumerates the lane addresses of every LDS access pattern of the
// family and applies the CDNA4 bank rules:
//   ds_read_b128       4 groups of 16 lanes {0-3,12-15,20-27}, {4-11,16-19,28-31},
//                      the same two + 32; bank = dword address mod 64
//   ds_read_b64_tr_b16 2 groups of 32 lanes; bank = dword address mod 64
//   ds_write_b128      8 groups of 8 contiguous lanes; bank = dword address mod 32
// One LDS cycle per group when conflict-free; each further distinct dword
// address on a busy bank within a group adds one cycle; equal addresses
// broadcast.
// Conditions (not measurements): 4 cycles per ds_read_b128, 2 per
// ds_read_b64_tr_b16, store array cycles no worse than the previous map's
// (and 8, the conflict-free figure), and the map is a bijection of the tile.
// Exit status 0 = all hold; every failure prints a line.
#include <cstdio>
#include <set>
#include <vector>

#include "fa32_lds_map.h"

namespace {

int failures = 0;
#define CHECK(cond, ...)                 \
  do {                                   \
    if (!(cond)) {                       \
      ++failures;                        \
      std::printf("FAIL: " __VA_ARGS__); \
      std::printf("\n");                 \
    }                                    \
  } while (0)

typedef std::vector<std::vector<int>> groups_t;

groups_t groups_b128() {
  const std::vector<int> g0 = {0, 1, 2, 3, 12, 13, 14, 15, 20, 21, 22, 23, 24, 25, 26, 27};
  const std::vector<int> g1 = {4, 5, 6, 7, 8, 9, 10, 11, 16, 17, 18, 19, 28, 29, 30, 31};
  groups_t g = {g0, g1, g0, g1};
  for (int i = 2; i < 4; ++i)
    for (int& l : g[i]) l += 32;
  return g;
}
groups_t groups_contig(int n) {
  groups_t g;
  for (int b = 0; b < 64; b += n) {
    g.emplace_back();
    for (int l = b; l < b + n; ++l) g.back().push_back(l);
  }
  return g;
}

// LDS-array cycles of one wave-instruction: lane l accesses `ndw` dwords at
// byte address addr[l]
int cycles(const int (&addr)[64], int ndw, const groups_t& groups, int nbanks) {
  int total = 0;
  for (const auto& g : groups) {
    std::vector<std::set<int>> bank(nbanks);
    for (int l : g)
      for (int d = 0; d < ndw; ++d) {
        const int a = addr[l] / 4 + d;
        bank[a % nbanks].insert(a);
      }
    size_t worst = 0;
    for (const auto& s : bank) worst = s.size() > worst ? s.size() : worst;
    total += (int)worst;
  }
  return total;
}

// the map this one replaces (slot ^ (row & 7) on byte bits 4-6): the model
// must reproduce its measured 8 + 8 conflict figures, and it is the "today"
// of the store condition
int old_swz(int byte_off) { return byte_off ^ (((byte_off >> 8) & 7) << 4); }

}  // namespace

int main() {
  const groups_t G128 = groups_b128(), G32 = groups_contig(32), G8 = groups_contig(8);
  int addr[64];

  // ---- ds_read_b128 row fragments: ff_afrag (s2, ks) of a 64-row tile and
  // ff_bfrag for rows 0-255 (a wave reads rows wave*32 + l31) ----
  int rmin = 1 << 30, rmax = 0, old_rmax = 0;
  for (int blk = 0; blk < 8; ++blk)  // blk 0-1 = ff_afrag's s2; 0-7 = ff_bfrag's wave
    for (int ks = 0; ks < 8; ++ks) {
      int old_addr[64];
      for (int l = 0; l < 64; ++l) {
        const int row = blk * 32 + (l & 31), half = l >> 5;
        addr[l] = ff_map_frag(row, ks, half);
        old_addr[l] = old_swz((row * FF_MAP_D + ks * 16 + half * 8) * 2);
        CHECK(addr[l] % 16 == 0, "fragment address %d not 16-byte aligned", addr[l]);
        CHECK(addr[l] / FF_MAP_ROW_BYTES == row, "fragment of row %d leaves its row", row);
      }
      const int c = cycles(addr, 4, G128, 64);
      CHECK(c == 4, "ds_read_b128 rows %d.. ks %d: %d cycles, want 4", blk * 32, ks, c);
      rmin = c < rmin ? c : rmin;
      rmax = c > rmax ? c : rmax;
      const int oc = cycles(old_addr, 4, G128, 64);
      old_rmax = oc > old_rmax ? oc : old_rmax;
    }
  std::printf("ds_read_b128 fragments: %d..%d cycles (previous map: %d)\n", rmin, rmax, old_rmax);
  CHECK(old_rmax == 8, "model gives %d cycles for the previous map's fragments, counters say 8",
        old_rmax);

  // ---- ds_read_b64_tr_b16: every (ds, read jj, ks) of ff_tr_read8 ----
  int tmin = 1 << 30, tmax = 0, old_tmax = 0;
  for (int ds = 0; ds < 4; ++ds)
    for (int jj = 0; jj < 2; ++jj)
      for (int ks = 0; ks < 4; ++ks) {
        int old_addr[64];
        for (int l = 0; l < 64; ++l) {
          const int l15 = l & 15, l31 = l & 31, half = l >> 5;
          addr[l] = ff_map_tr(ds, l15, l31, half, jj) + ks * FF_MAP_KS_BYTES;
          // the element this lane must fetch: 4 elements of tile row
          // ks*16 + half*8 + jj*4 + (l15 >> 2) at column ds*32 + (l31 & 16) + (l15 & 3)*4
          const int row = ks * 16 + half * 8 + jj * 4 + (l15 >> 2);
          const int lin = (row * FF_MAP_D + ds * 32 + (l31 & 16) + (l15 & 3) * 4) * 2;
          CHECK(addr[l] == ff_map_swz(lin),
                "tr read ds %d jj %d ks %d lane %d: address %d is not the image of %d", ds, jj, ks,
                l, addr[l], lin);
          CHECK(addr[l] >= 0 && addr[l] + 8 <= 64 * FF_MAP_ROW_BYTES,
                "tr read address %d outside the 64-row tile", addr[l]);
          old_addr[l] = old_swz(lin);
        }
        const int c = cycles(addr, 2, G32, 64);
        CHECK(c == 2, "ds_read_b64_tr_b16 ds %d jj %d ks %d: %d cycles, want 2", ds, jj, ks, c);
        tmin = c < tmin ? c : tmin;
        tmax = c > tmax ? c : tmax;
        const int oc = cycles(old_addr, 2, G32, 64);
        old_tmax = oc > old_tmax ? oc : old_tmax;
      }
  std::printf("ds_read_b64_tr_b16: %d..%d cycles (previous map: %d)\n", tmin, tmax, old_tmax);
  CHECK(old_tmax == 8, "model gives %d cycles for the previous map's tr reads, counters say 8",
        old_tmax);

  // ---- ds_write_b128 staging stores, 128-, 256- and 512-thread blocks, up to
  // a 256-row tile (the largest the family stages) ----
  for (int threads : {128, 256, 512}) {
    int wmax = 0, old_wmax = 0;
    const int chunks = 256 * FF_MAP_D / (threads * 8);
    for (int j = 0; j < chunks; ++j)
      for (int wave = 0; wave < threads / 64; ++wave) {
        int old_addr[64];
        for (int l = 0; l < 64; ++l) {
          const int e = ff_map_chunk(j, wave * 64 + l, threads);
          addr[l] = ff_map_chunk_byte(e);
          old_addr[l] = old_swz(e * 2);
        }
        const int c = cycles(addr, 4, G8, 32), oc = cycles(old_addr, 4, G8, 32);
        CHECK(c <= oc, "ds_write_b128 threads %d chunk %d wave %d: %d array cycles, previous map %d",
              threads, j, wave, c, oc);
        CHECK(c == 8, "ds_write_b128 threads %d chunk %d wave %d: %d array cycles, want 8", threads,
              j, wave, c);
        wmax = c > wmax ? c : wmax;
        old_wmax = oc > old_wmax ? oc : old_wmax;
      }
    std::printf("ds_write_b128, %d threads: %d array cycles (previous map: %d)\n", threads, wmax,
                old_wmax);
  }

  // ---- bijection: every 16-byte slot of a tile of 64, 128 or 256 rows is
  // the image of exactly one slot of the same tile, and the staging chunks
  // cover the tile ----
  for (int rows : {64, 128, 256}) {
    const int bytes = rows * FF_MAP_ROW_BYTES;
    std::set<int> image;
    for (int b = 0; b < bytes; b += 16) {
      const int s = ff_map_swz(b);
      CHECK(s >= 0 && s < bytes && s % 16 == 0, "slot %d maps to %d, outside the %d-row tile", b, s,
            rows);
      CHECK(s / FF_MAP_ROW_BYTES == b / FF_MAP_ROW_BYTES, "slot %d changes row", b);
      image.insert(s);
      for (int i = 1; i < 16; ++i)
        CHECK(ff_map_swz(b + i) == s + i, "byte %d of slot %d is not kept in order", i, b);
    }
    CHECK((int)image.size() == rows * 16, "%d-row tile: %d distinct images of %d slots", rows,
          (int)image.size(), rows * 16);
    for (int threads : {64, 128, 256, 512}) {
      std::set<int> stored;
      for (int j = 0; j < rows * FF_MAP_D / (threads * 8); ++j)
        for (int tid = 0; tid < threads; ++tid)
          stored.insert(ff_map_chunk_byte(ff_map_chunk(j, tid, threads)));
      CHECK(stored == image, "%d-row tile staged by %d threads does not cover the image", rows,
            threads);
    }
  }
  // the swizzle reads row & 15 only: the tr reads' +16-row immediates commute
  for (int row = 0; row < 256; ++row)
    CHECK(ff_map_g(row) == ff_map_g(row & 15) && ff_map_g(row) >= 0 && ff_map_g(row) < 16,
          "g(%d) is not a function of row & 15 in 0..15", row);
  std::printf("bijection: ok\n");

  std::printf(failures ? "%d checks failed\n" : "all checks passed\n", failures);
  return failures ? 1 : 0;
}
