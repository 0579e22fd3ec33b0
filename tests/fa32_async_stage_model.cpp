// Host check of the SOURCE side of the 32x32 flash family's LDS tile image
// (built and run by tests/test_fa32_async_stage.py): the direct global -> LDS
// staging of ff_stage_async (fa32_common.h) against the register staging of
// ff_stage / ff_stage_rows.  Includes the address header the kernels are built
// on and walks the helper's own arithmetic: load i of thread tid lands at LDS
// byte ff_map_async_base(i, tid, threads) + 16 * (tid & 63) and reads the 16
// bytes at element ff_map_async_src(0, tid, threads, stride) + i *
// ff_map_async_step(threads, stride) of the tile in global memory.
// Conditions, for tiles of 64 and 256 rows staged by 256 and 512 threads,
// contiguous (stride 128) and with a [B,S,H,D] row stride of Hq*128:
//   1. every 16-byte position of the image is assigned exactly once, and a
//      wave's load covers 1 KiB of linear LDS (4 whole rows);
//   2. the chunk put there is the one ff_map_chunk_byte puts there: the
//      register path stores chunk e (8 elements) at byte ff_map_chunk_byte(e);
//   3. the closed form the helper uses equals ff_map_async_src(i, ...);
//   4. the 16 lanes of a quarter-wave read one whole 256-byte row (coalesced);
//   5. every global element offset formed lies inside [0, ROWS * stride), and
//      the 8 elements read stay inside the row's 128.
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

void check(int rows, int threads, int stride) {
  const int tile_bytes = rows * FF_MAP_ROW_BYTES;
  const int loads = tile_bytes / (threads * 16);
  CHECK(loads * threads * 16 == tile_bytes, "rows %d threads %d: no whole number of loads", rows,
        threads);
  // image byte -> global element offset the direct path puts there (-1: none)
  std::vector<int> direct(tile_bytes / 16, -1);
  for (int i = 0; i < loads; ++i)
    for (int w = 0; w < threads / 64; ++w) {
      std::set<int> rows_of_quarter[4];
      for (int l = 0; l < 64; ++l) {
        const int tid = w * 64 + l;
        const int base = ff_map_async_base(i, tid, threads);
        CHECK(base == ff_map_async_base(i, w * 64, threads) && base % FF_MAP_PIECE_BYTES == 0,
              "rows %d threads %d: LDS base of load %d not wave-uniform at tid %d", rows, threads,
              i, tid);
        const int lds = base + 16 * l;
        CHECK(lds >= 0 && lds + 16 <= tile_bytes, "rows %d threads %d: LDS byte %d outside the tile",
              rows, threads, lds);
        CHECK(lds == 16 * ff_map_async_pos(i, tid, threads),
              "rows %d threads %d: position of load %d tid %d", rows, threads, i, tid);
        const int src = ff_map_async_src(0, tid, threads, stride) +
                        i * ff_map_async_step(threads, stride);
        CHECK(src == ff_map_async_src(i, tid, threads, stride),
              "rows %d threads %d stride %d: closed form differs at load %d tid %d", rows, threads,
              stride, i, tid);
        CHECK(src >= 0 && src + 8 <= rows * stride && src % stride + 8 <= FF_MAP_D && src % 8 == 0,
              "rows %d threads %d stride %d: source element %d out of range", rows, threads, stride,
              src);
        if (lds >= 0 && lds + 16 <= tile_bytes) {
          CHECK(direct[lds / 16] == -1, "rows %d threads %d: position %d assigned twice", rows,
                threads, lds / 16);
          direct[lds / 16] = src;
        }
        rows_of_quarter[l / 16].insert(src / stride);
      }
      for (int qw = 0; qw < 4; ++qw)
        CHECK(rows_of_quarter[qw].size() == 1,
              "rows %d threads %d: a quarter-wave reads %d rows", rows, threads,
              (int)rows_of_quarter[qw].size());
      // one row per quarter, 16 distinct slots: the whole 256-byte row
      for (int qw = 0; qw < 4; ++qw) {
        std::set<int> cols;
        for (int l = qw * 16; l < qw * 16 + 16; ++l)
          cols.insert(direct[(ff_map_async_base(i, w * 64, threads) + 16 * l) / 16] % stride);
        CHECK(cols.size() == 16, "rows %d threads %d: a quarter-wave covers %d slots of its row",
              rows, threads, (int)cols.size());
      }
    }
  // against the register path: chunk e of the row-major tile lives at byte
  // ff_map_chunk_byte(e); in global memory it is element (e / 128) * stride + e % 128
  const int chunks = rows * FF_MAP_D / (threads * 8);
  std::vector<int> reg(tile_bytes / 16, -1);
  for (int j = 0; j < chunks; ++j)
    for (int tid = 0; tid < threads; ++tid) {
      const int e = ff_map_chunk(j, tid, threads);
      reg[ff_map_chunk_byte(e) / 16] = (e / FF_MAP_D) * stride + e % FF_MAP_D;
    }
  int unassigned = 0, differ = 0;
  for (int p = 0; p < tile_bytes / 16; ++p) {
    unassigned += direct[p] == -1;
    differ += direct[p] != reg[p];
  }
  CHECK(unassigned == 0, "rows %d threads %d: %d positions never assigned", rows, threads,
        unassigned);
  CHECK(differ == 0, "rows %d threads %d stride %d: %d positions hold another chunk than "
        "ff_map_chunk_byte's", rows, threads, stride, differ);
  std::printf("rows %d threads %d stride %d: %d loads per thread, image equal\n", rows, threads,
              stride, loads);
}

}  // namespace

int main() {
  // ff_map_src_byte is the inverse of ff_map_swz on 16-byte positions
  for (int p = 0; p < 256 * 16; ++p)
    CHECK(ff_map_swz(ff_map_src_byte(p)) == 16 * p, "ff_map_src_byte(%d) is not the preimage", p);
  for (int rows : {64, 256})
    for (int threads : {256, 512})
      for (int hq : {1, 2, 4, 32}) check(rows, threads, hq * FF_MAP_D);
  if (failures) {
    std::printf("%d checks failed\n", failures);
    return 1;
  }
  std::printf("all checks passed\n");
  return 0;
}
