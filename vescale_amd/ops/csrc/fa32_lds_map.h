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

// ---------------------------------------------------------------------------
// The SOURCE side of the same image, for direct global -> LDS loads
// (global_load_lds, 16 bytes per lane, no destination VGPR; ff_stage_async in
// fa32_common.h).  Such a load cannot scatter: one load of one wave fills 1 KiB
// of LINEAR LDS, lane l at base + 16*l, which is 4 whole tile rows.  So the
// swizzle moves to the address the lane reads FROM: the lane that fills the
// 16-byte position p of the image (byte 16*p) fetches the chunk that lives
// there.  ff_map_swz is an involution (it XORs bits 4-7 with a function of the
// bits above them), so that chunk is at byte ff_map_swz(16*p) of the row-major
// tile; the XOR permutes the 16 slots of one 256-byte row, so the 16 lanes of
// a quarter-wave still read one whole row and the global side stays coalesced.
//
// Positions to lanes: the tile is cut into 1 KiB pieces; wave w of W =
// threads/64 waves takes pieces w, w + W, w + 2W, ..., one load each.  Load i
// of thread tid (lane l = tid & 63 of wave w = tid >> 6) is piece w + i*W,
// position (w + i*W)*64 + l = tid + i*threads: ff_map_chunk's assignment in
// 16-byte units, so the direct path moves the same chunk per (i, tid) as the
// register path and only the place of the swizzle differs.
// ---------------------------------------------------------------------------
#define FF_MAP_PIECE_BYTES 1024  // one direct load of one wave: 64 lanes x 16 bytes

// byte offset, in the row-major [rows][128] tile, of the chunk at image position p
FF_MAP_FN int ff_map_src_byte(int p) { return ff_map_swz(16 * p); }
// image position that load i of thread tid fills
FF_MAP_FN int ff_map_async_pos(int i, int tid, int threads) { return tid + i * threads; }
// LDS byte offset of the wave-uniform base of that load (the lane adds 16*l)
FF_MAP_FN int ff_map_async_base(int i, int tid, int threads) {
  return ((tid >> 6) + i * (threads >> 6)) * FF_MAP_PIECE_BYTES;
}
// element offset that load reads from, in a tile whose rows are `stride`
// elements apart in global memory (stride = FF_MAP_D: a contiguous tile)
FF_MAP_FN int ff_map_async_src(int i, int tid, int threads, int stride) {
  const int b = ff_map_src_byte(ff_map_async_pos(i, tid, threads));
  return (b >> 8) * stride + ((b & (FF_MAP_ROW_BYTES - 1)) >> 1);
}
// With threads/16 a multiple of 16 (the period of g) load i reads the rows
// i * threads/16 below load 0's with the same XOR: src(i) = src(0) + i * step,
// which is how ff_stage_async forms its addresses.
FF_MAP_FN int ff_map_async_step(int threads, int stride) { return (threads >> 4) * stride; }
