// acx_cur_layout.h -- the layout of acx_learner_step's part of the curriculum workspace, in uint64
// words from its start (acx_internal_curriculum_fused_offset(B) int32 words into the caller's
// buffer).  The one definition: the step kernel's ranking (acx_cur_rank.h, CurLayout) addresses
// the words with it, and acx_curriculum_workspace / acx_learner_failure_word size and locate them
// with it.
//   [SEQ] launch sequence number, [BASE] the scan's base, [FAILED] sticky failure word,
//   [TILES, TILES + T) tile counts, then G group totals, then G group arrival words
//   ARRIVE_STRIDE words apart (T tiles of TILE_ENVS envs, G groups of GROUP_TILES tiles).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace acx {
namespace cur_layout {

constexpr int TILE_ENVS = 64;    // a tile is one wave's envs
constexpr int GROUP_TILES = 64;  // a group's tiles are polled a lane each
// uint64 words between two groups' arrival words, the launch's only same-address atomics (64
// tiles add to each): 256 bytes apart, one per channel-interleave unit, the step is 6 % faster
// than with the words packed (fresh episodes 0.1257 vs 0.1345 ms, steady state 0.159 vs 0.165,
// profiles/r05/r05x_learner_probe_stride.json; spacing the tile count words too changed nothing).
constexpr int ARRIVE_STRIDE = 32;
constexpr int SEQ = 0, BASE = 1, FAILED = 2, TILES = 3;

__host__ __device__ constexpr int64_t tiles(int64_t B) { return (B + TILE_ENVS - 1) / TILE_ENVS; }
__host__ __device__ constexpr int64_t groups(int64_t n_tiles) { return (n_tiles + GROUP_TILES - 1) / GROUP_TILES; }
__host__ __device__ constexpr int64_t group_totals(int64_t n_tiles) { return TILES + n_tiles; }
__host__ __device__ constexpr int64_t arrivals(int64_t n_tiles) { return group_totals(n_tiles) + groups(n_tiles); }
// uint64 words of the whole part for B envs
__host__ __device__ constexpr int64_t words(int64_t B) {
    return arrivals(tiles(B)) + groups(tiles(B)) * ARRIVE_STRIDE;
}

}  // namespace cur_layout
}  // namespace acx
