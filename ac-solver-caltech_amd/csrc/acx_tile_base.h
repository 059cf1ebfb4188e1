// acx_tile_base.h -- what FastTile and CodeTile have in common: a wave's LDS slice (the row image,
// then per-row flag, dirty and live-chunk bytes) and the members that only touch those bytes.
// A plain base struct; each tile adds its own row image format on top (acx_tile.h states the
// interface as a whole).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "acx_moves.h"
#include "acx_tile_io.h"

namespace acx {

// LC: compile-time L (a multiple of 4); SC: the image's row stride in dwords
template <int LC, int SC>
struct PackedTileBase {
    static constexpr int S = SC;

    uint32_t* lds;
    uint8_t* flags;
    uint8_t* dirty;         // per row: bit h = relator h differs from the loaded row (store_dirty)
    uint8_t* lim;           // per row and relator, lengths-carrying step: live 16-byte chunks (lim[2r + h])

    static __host__ __device__ constexpr size_t wave_bytes(int) { return (size_t)WAVE * S * 4 + 4 * WAVE; }
    __device__ __forceinline__ PackedTileBase(char* base) {
        lds = reinterpret_cast<uint32_t*>(base);
        flags = reinterpret_cast<uint8_t*>(base + WAVE * S * 4);
        dirty = flags + WAVE;
        lim = flags + 2 * WAVE;
    }
    // chunks of 4 letters (16 bytes of a global row); LC / 4 chunks per relator
    __device__ __forceinline__ static int live_chunks(int n) { return n <= 0 ? 0 : n >= LC ? LC / 4 : (n + 3) >> 2; }
    // chunk k (< LC / 2) of row r is live (inside its relator's letters)
    __device__ __forceinline__ bool live(int r, int k) const {
        const int h = k >= LC / 4 ? 1 : 0;
        return k - h * (LC / 4) < lim[2 * r + h];
    }
    __device__ __forceinline__ int Lr() const { return LC; }
};

// tile_bad (wave-uniform: some row of the tile is flagged) is each tile's own member, declared
// after the tile's other registers: as a member of the base it changed the L = 128 rollout's code.
// What the tiles do with it is here.
// restore_flags: per-row fallback codes (FB_*, acx_tile_io.h) replacing whatever the loads left in
// flags[]; the flagged rows of store<true> / store_dirty / store_rows_i8_fb copy their fallback row
__device__ __forceinline__ void tile_restore_flags(uint8_t* flags, bool& tile_bad, int lane, uint32_t code) {
    flags[lane] = (uint8_t)code;
    tile_bad = __any(code != 0u);
    wave_sync();
}
// flag_rows: additionally flag the rows of lanes with code != 0
__device__ __forceinline__ void tile_flag_rows(uint8_t* flags, bool& tile_bad, int lane, uint32_t code) {
    if (code) flags[lane] = (uint8_t)code;
    tile_bad = tile_bad || __any(code != 0u);
}

}  // namespace acx
