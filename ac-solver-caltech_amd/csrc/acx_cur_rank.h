// acx_cur_rank.h -- the device side of the fused learner's ranking: the finished envs' prefix count
// inside the step kernel (step_body with LEARN, acx_learner_step).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "acx_cur_layout.h"
#include "acx_kernel_common.h"
#include "acx_moves.h"
#include "acx_step_args.h"

namespace acx {

// ---------------------------------------------------------------------------------
// The curriculum's ranking inside the step kernel (acx_learner_step, one launch).  Finished envs
// (done | truncated) take the initial states next_index, next_index + 1, ... in env order
// (training.py:329-336), so an env needs the number of finished envs before it -- a prefix count
// over the whole batch -- and the last tile needs the total (the new next_index).  Two levels,
// no chain: a tile is one wave's 64 envs, a group is 64 consecutive tiles.
//   * every tile publishes its count (a seq-tagged status word) and adds (1, count) to its
//     group's arrival word with one 64-bit atomic; the add that completes the group publishes the
//     group's total and clears the arrival word for the next launch (64 adds per address at most:
//     MI355X_MICROARCH "dequeue" -- one word saturates at ~88 adds per us);
//   * tile 0 publishes next_index as the scan's base;
//   * a tile that needs its prefix -- one with finished envs -- polls the base, the totals of the
//     groups before its own and the counts of the tiles before it in its group, until all are
//     there (no propagation through intermediate tiles: it waits only for earlier tiles to have
//     published once); the last tile polls every group total, writes next_index and advances the
//     launch's sequence number;
//   * words are written and polled with agent-scope atomics (each word is the whole hand-off:
//     "8-B agent atomics both sides"); a word of an earlier launch carries another sequence number
//     and reads as not there.  Every wave reads the sequence number before it publishes, so once
//     every group is complete no wave of the launch reads it again and the last tile may advance it;
//   * HIP promises no dispatch order: a tile that polls too long (2^20 polls, ~seconds -- an
//     earlier tile never scheduled) gives up and flags its finished envs needs_host = 3
//     (CurriculumRecord.process raises), so the launch always ends.  Any give-up -- a tile's
//     prefix, or the last tile's total, after which next_index is stale -- also sets the sticky
//     failure word: every later launch then ranks nothing (its finished envs get needs_host = 3) until
//     the host re-zeroes the workspace (LearnerEnv.reset_workspace, which also restores
//     next_index from curr_index), since a give-up can leave a group's arrival word incomplete;
//     CurriculumRecord.process raises on the word.  Concurrent launches on one workspace are not
//     supported (they would overwrite each other's words; nothing detects it).
// The words of cur_ws are laid out by acx_cur_layout.h (CurLayout below).
// ---------------------------------------------------------------------------------
constexpr uint64_t CUR_SET = 1ull << 62;
constexpr uint32_t CUR_FAIL = 0xffffffffu;
constexpr uint32_t CUR_SEQ_MASK = (1u << 30) - 1u;

__device__ __forceinline__ uint64_t cur_word(uint32_t seq, uint32_t v) {
    return CUR_SET | ((uint64_t)(seq & CUR_SEQ_MASK) << 32) | v;
}
__device__ __forceinline__ bool cur_is(uint64_t w, uint32_t seq) {
    return (w >> 62) == 1 && ((uint32_t)(w >> 32) & CUR_SEQ_MASK) == (seq & CUR_SEQ_MASK);
}
__device__ __forceinline__ uint64_t cur_load(const uint64_t* p) {
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ void cur_store(uint64_t* p, uint64_t v) {
    __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// the words of a.cur_ws (acx_cur_layout.h: the one definition, which acx_curriculum_workspace
// sizes the workspace with); a tile is a wave's envs, a group's tiles are polled a lane each
static_assert(cur_layout::TILE_ENVS == WAVE && cur_layout::GROUP_TILES == WAVE, "one tile per wave, one tile per lane");
struct CurLayout {
    int64_t tiles, groups;
    uint64_t *base, *tile, *group, *arrive;
    __device__ __forceinline__ CurLayout(const StepArgs& a) {
        tiles = cur_layout::tiles(a.B);
        groups = cur_layout::groups(tiles);
        base = a.cur_ws + cur_layout::BASE;
        tile = a.cur_ws + cur_layout::TILES;
        group = a.cur_ws + cur_layout::group_totals(tiles);
        arrive = a.cur_ws + cur_layout::arrivals(tiles);
    }
};

// this tile's count, its group arrival, and (tile 0) the base.  Returns the arrival word before
// this tile's add (lane 0), for cur_publish_end right after: deferring that to the tile's tail
// (so the add's return trip overlaps the stores) made the step slower, fresh episodes 0.143 vs
// 0.140 ms and steady state 0.21 vs 0.172 (same buffers, r05v), as later tiles then wait longer
// for the group total
// cnext: next_index as this wave read it, before publishing -- the last tile overwrites it once
// every tile has published, so the read must complete first: the published word takes an opaque
// dependency on it, both words being relaxed agent-scope atomics
__device__ __forceinline__ uint64_t cur_publish(const StepArgs& a, const WaveCtx& w, uint32_t seq, uint32_t cnt,
                                                int64_t cnext) {
    if (w.lane != 0) return 0;
    const CurLayout c(a);
    const int64_t t = w.r0 / WAVE, g = t / WAVE;
    if (t == 0) cur_store(c.base, cur_word(seq, (uint32_t)*a.cur_next));
    uint64_t word = cur_word(seq, cnt);
    asm volatile("" : "+v"(word) : "s"((uint32_t)cnext));
    cur_store(c.tile + t, word);
    return __hip_atomic_fetch_add(c.arrive + g * cur_layout::ARRIVE_STRIDE, (1ull << 32) | cnt, __ATOMIC_RELAXED,
                                  __HIP_MEMORY_SCOPE_AGENT);
}
// the sticky failure word (see above)
__device__ __forceinline__ void cur_set_failed(const StepArgs& a) { cur_store(a.cur_ws + cur_layout::FAILED, 1ull); }

// the add that completed its group publishes the group's total and clears the arrival word for
// the next launch
__device__ __forceinline__ void cur_publish_end(const StepArgs& a, const WaveCtx& w, uint32_t seq, uint32_t cnt,
                                                uint64_t old) {
    if (w.lane != 0) return;
    const CurLayout c(a);
    const int64_t t = w.r0 / WAVE, g = t / WAVE;
    const int64_t gsize = (c.tiles - g * WAVE) < WAVE ? (c.tiles - g * WAVE) : WAVE;
    if ((int64_t)(old >> 32) + 1 == gsize) {
        cur_store(c.group + g, cur_word(seq, (uint32_t)old + cnt));
        cur_store(c.arrive + g * cur_layout::ARRIVE_STRIDE, 0ull);
    }
}

// base + the counts of every tile before this one (all_groups: + every group's total instead: the
// last tile's next_index), or CUR_FAIL.  Wave-uniform control flow.  A word, once seen with this
// launch's seq, is final: each lane re-reads only the words it has not seen yet (`pend`), so the
// polls of the waiting tiles thin out as the prefix fills in (re-reading every word on every poll
// put ~4k waiting waves on the same few dozen lines).  Group totals are taken 4 per lane, 256 per
// round; the base (lane 0) and the own group's earlier tile counts (a lane each) with the first.
// (s_sleep 8 between polls instead: the same, r05v)
__device__ __forceinline__ uint32_t cur_prefix(const StepArgs& a, const WaveCtx& w, uint32_t seq, bool all_groups) {
    if (a.cur_fail == 1 || (a.cur_fail == 2 && all_groups)) return CUR_FAIL;  // test hook
    const CurLayout c(a);
    const int64_t t = w.r0 / WAVE, g = t / WAVE;
    const int64_t ng = all_groups ? c.groups : g;  // whole groups summed
    auto group_bits = [&](int64_t k0) {
        uint32_t b = 0;
#pragma unroll
        for (int i = 0; i < 4; ++i) b |= (k0 + 4 * w.lane + i < ng) ? 1u << i : 0u;
        return b;
    };
    uint32_t pend = group_bits(0);
    if (w.lane == 0) pend |= 1u << 5;                            // the base
    if (!all_groups && g * WAVE + w.lane < t) pend |= 1u << 4;  // a tile before this one in its group
    uint32_t x = 0, polls = 0;
    int64_t k0 = 0;
    while (true) {
        uint64_t v[6];
#pragma unroll
        for (int i = 0; i < 4; ++i) v[i] = (pend >> i) & 1u ? cur_load(c.group + k0 + 4 * w.lane + i) : 0ull;
        v[4] = (pend >> 4) & 1u ? cur_load(c.tile + g * WAVE + w.lane) : 0ull;
        v[5] = (pend >> 5) & 1u ? cur_load(c.base) : 0ull;
#pragma unroll
        for (int i = 0; i < 6; ++i)
            if (((pend >> i) & 1u) && cur_is(v[i], seq)) {
                x += (uint32_t)v[i];
                pend &= ~(1u << i);
            }
        if (__all(pend == 0u)) {
            k0 += 4 * WAVE;
            if (k0 >= ng) break;
            pend = group_bits(k0);
            continue;
        }
        if (++polls > (1u << 20)) return CUR_FAIL;
        __builtin_amdgcn_s_sleep(2);
    }
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) x += (uint32_t)__shfl_xor((int)x, o, WAVE);
    return x;
}

}  // namespace acx
