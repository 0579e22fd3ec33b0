// LDS image of the 32x32x16 flash family's [rows][128] bf16 tiles: pure
// address arithmetic, no HIP dependency, so a host program can include the
// exact code the kernels run (tests/test_fa32_lds_map.py builds one and
// checks the image against the LDS bank rules).  fa32_common.h builds its
// loads and stores on these functions; nothing else encodes the map.
//
// A tile row is 256 bytes = 16 slots of 16 bytes = all 64 banks once, so the
// row index alone never changes a bank.  Row `row` stores its slot s at slot
//     s ^ g(row),   g(row) = ((row & 3) << 2) | ((row >> 2) & 3)
// (byte bits 4-7 of the offset).  g is a bijection on row & 15 and has
// period 16 in the row, and its upper two bits are row & 3:
//   - ds_read_b128 row fragments (ff_afrag / ff_bfrag): the hardware serves a
//     wave in four 16-lane groups, {0-3,12-15,20-27}, {4-11,16-19,28-31} and
//     the same two + 32.  The 16 lanes of a group read the same slot of 16
//     rows with 16 distinct row & 15, so g sends them to 16 distinct slots =
//     64 distinct banks: 4 LDS cycles, the conflict-free cost.
//   - ds_read_b64_tr_b16 (ff_tr_read8): served in 2 groups of 32 lanes; a
//     group reads 4 consecutive rows (row & 3 = 0..3, the rest of the row
//     index equal), 64 bytes from the same 64-byte column band each.  The
//     upper two bits of g move the 4 rows into 4 different bands, the lower
//     two permute the 16-byte slots inside a band: 64 dwords on 64 banks, 2
//     LDS cycles.
//   - ds_write_b128 staging stores: 8 contiguous lanes write 8 contiguous
//     slots of one row; XOR with a constant keeps them distinct mod 8, so the
//     store stays at its 8 array cycles (banks mod 32).
// The previous map, slot ^ (row & 7) on bits 4-6, was 2-way conflicted on the
// row fragments (16 rows on 8 slots) and 4-way on the tr reads (the XOR never
// left the 64-byte band): 8 + 8 cycles where this one takes 4 + 2.
#pragma once

#if defined(__HIP__) || defined(__CUDACC__)
#define FF_MAP_FN __host__ __device__ constexpr inline
#else
#define FF_MAP_FN constexpr inline
#endif

#define FF_MAP_D 128                       // bf16 elements per tile row
#define FF_MAP_ROW_BYTES (FF_MAP_D * 2)    // 256
#define FF_MAP_KS_BYTES (16 * FF_MAP_ROW_BYTES)  // tr reads: one ks step = 16 rows

// slot XOR of tile row `row`
FF_MAP_FN int ff_map_g(int row) { return ((row & 3) << 2) | ((row >> 2) & 3); }

// linear byte offset in a row-major [*][128] bf16 tile -> offset in the image
FF_MAP_FN int ff_map_swz(int byte_off) {
  return byte_off ^ (ff_map_g(byte_off >> 8) << 4);
}

// 16-byte operand fragment of row `row`: elements ks*16 + half*8 .. +8
// (ff_afrag: row = s2*32 + l31; ff_bfrag: any row)
FF_MAP_FN int ff_map_frag(int row, int ks, int half) {
  return ff_map_swz((row * FF_MAP_D + ks * 16 + half * 8) * 2);
}

// the two addresses of ff_tr_read8 (jj = 0, 1) at ks = 0: lane reads 8 bytes of
// tile row half*8 + 4*jj + ((l15 & 15) >> 2) at element column
// ds*32 + (l31 & 16) + (l15 & 3)*4.  Read ks adds ks * FF_MAP_KS_BYTES: 16
// rows further, where g repeats, and the sum never carries into the XORed
// bits (row <= 15 here, so the offset stays below 4096).
FF_MAP_FN int ff_map_tr(int ds, int l15, int l31, int half, int jj) {
  const int col2 = (ds * 32 + (l31 & 16) + (l15 & 3) * 4) * 2;
  const int row = half * 8 + 4 * jj + ((l15 & 15) >> 2);
  return (row * FF_MAP_ROW_BYTES + col2) ^ (ff_map_g(row) << 4);
}

// staging: thread tid of `threads` moves chunk j = the 8 elements at
// ff_map_chunk(j, tid, threads), stored at byte ff_map_chunk_byte(e)
FF_MAP_FN int ff_map_chunk(int j, int tid, int threads) { return (tid + j * threads) * 8; }
FF_MAP_FN int ff_map_chunk_byte(int e) { return ff_map_swz(e * 2); }
