// acx_tile.h -- the LDS tile of a wave's 64 rows: the interface the three tile classes share, the
// classes themselves (one header each), TileFor, which picks one by L, and what is written on top
// of the interface alone.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <type_traits>
#include "acx_tile_code.h"
#include "acx_tile_fast.h"
#include "acx_tile_generic.h"
#include "acx_tile_io.h"

namespace acx {

// ---------------------------------------------------------------------------------
// LDS staging.  A wave owns a tile of up to 64 consecutive envs.  The tile is moved
// HBM <-> LDS with coalesced 16-byte (or 8-byte) accesses by all 64 lanes, as int8
// letters; then each lane packs / unpacks its own row.  Three implementations with one
// interface (TileFor picks by L; the helpers they share are in acx_tile_io.h and acx_tile_base.h):
//   CodeTile   (acx_tile_code.h) compile-time L >= 64 with L % 8 == 0 (L = 128): one 16-bit slot of 2-bit
//              codes and a non-zero mask per 4 letters.
//   FastTile   (acx_tile_fast.h) any other compile-time L with L % 4 == 0 (L = 36): the LDS
//              tile is the int8 image of the global tile, row stride S dwords with
//              S = 2 mod 4 so each lane's 8-byte row reads/writes hit distinct bank
//              pairs; addresses are affine in the chunk index; pack/unpack are SWAR over
//              4 letters per dword.
//   GenericTile  (acx_tile_generic.h) runtime L (parity tests at any L <= 128): per-letter pack/unpack.
// Rows holding a value outside {-2..2} are flagged (flags[row]) at load time.
//
// The tile interface: what a kernel may use of a Tile ("all": each class implements it for real).
//   Tile(lds_slice, L), wave_bytes(L)   the wave's slice of dynamic LDS and its size: all
//   Lr()                       the row's L (compile-time where the class has one): all
//   PW                         64-bit words per bit plane, for PlaneRegs<PW>: all
//   load<PIPE, LIVE, NTL, BATCH>(g, R, lane)
//                              R contiguous global rows -> LDS, flags set: all.  PIPE (software-
//                              pipelined full tile): CodeTile; FastTile's loop is unrolled anyway,
//                              GenericTile ignores it.  LIVE (only the chunks inside each relator's
//                              letters, after set_lim): FastTile, CodeTile; GenericTile reads whole
//                              rows.  NTL (non-temporal loads): FastTile, CodeTile.  BATCH (loads
//                              in flight): FastTile
//   load_block(g, R)           the same by all threads of the block, block-wide barriers:
//                              FastTile, CodeTile; GenericTile has none (callers test LC)
//   load_rows(g, rows, R, lane)  only the rows in the wave-uniform mask `rows`: all
//   PREFETCH_OK, RPI, fetch_rows(g, rows, lane), put_rows(v, rows, apply, lane)
//                              load_rows in two halves, at most RPI rows: FastTile
//                              (PREFETCH_OK); CodeTile and GenericTile stub them, never called
//   pack(lane, regs)           lane's row -> PlaneRegs<PW> or PresRegs<NW>, true if the row is
//                              outside the domain: all.  pack<LIVE>(lane, PlaneRegs): skips groups
//                              past every row's live chunks, CodeTile; the others ignore LIVE
//   unpack(lane, regs), unpack_half(lane, regs, h1)
//                              registers -> lane's row / its relator h1 only: all
//   unpack_dirty<LIVE>(lane, regs)
//                              unpack, returning which relators changed (bit h): FastTile,
//                              CodeTile (LIVE: CodeTile); GenericTile always returns 3
//   LIVE_ROWS, set_lim(lane, n0, n1), widen_lim(lane, n0, n1)
//                              the live chunks of the row's relators, for load<LIVE> and
//                              store_dirty<LIVE>: FastTile, CodeTile; GenericTile (LIVE_ROWS
//                              false) stubs them
//   set_dirty(lane, m), store_dirty<NT, LIVE>(g, R, lane, fallback2)
//                              in-place store of the changed relators only: FastTile, CodeTile;
//                              GenericTile stores every row
//   store<FB, NT, F32>(g, gpitch, R, fallback, fpitch, lane, fallback2, skip)
//                              LDS -> global rows of any pitch, flagged rows from their fallback
//                              row (FB), as float32 (F32), rows in `skip` left out: all
//   store_rows<NT>(g, R, lane), store_rows_i8<NT>(g, R, lane)
//                              LDS -> contiguous rows as int32 / int8 letters: all (FastTile's
//                              store_rows also takes a chunk range)
//   NT_STEP_LOADS              the step kernels' NTL choice (see ld_tile): all
//   restore_flags(lane, code), flag_rows(lane, code), flags[], letter(r, k)
//                              the rows' fallback codes set / added by the kernel, and one letter
//                              of the LDS image (store_rows_i8_fb): all
// ---------------------------------------------------------------------------------

template <int NW, int LC, int VEC>
using TileFor = typename std::conditional<
    (LC >= 64 && LC % 8 == 0), CodeTile<NW, LC>,
    typename std::conditional<(LC > 0 && LC % 4 == 0), FastTile<NW, LC>, GenericTile<NW, LC, VEC>>::type>::type;

// The int8 trajectory rows of a tile with flagged rows (rare, wave-uniform branch): byte by byte,
// flagged rows as the int8 values of their fallback row (numpy's astype(int8) wrap)
template <class Tile>
__device__ __forceinline__ void store_rows_i8_fb(const Tile& t, int8_t* g, int R, int twoL, int lane,
                                              const int32_t* fb_in, const int32_t* fb_reset) {
    for (int i = lane; i < R * twoL; i += WAVE) {
        const int r = i / twoL, k = i - r * twoL;
        const uint32_t fc = t.flags[r];
        g[i] = (int8_t)(fc ? fb_src(fc, fb_in, fb_reset)[(int64_t)r * twoL + k] : t.letter(r, k));
    }
}

}  // namespace acx
