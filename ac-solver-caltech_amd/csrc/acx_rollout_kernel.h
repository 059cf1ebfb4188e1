// acx_rollout_kernel.h -- T steps of every env in one launch (rollout_kernel), and the pass that
// packs its move ids 8 to a word (pack_actions_kernel).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "acx.h"
#include "acx_kernel_common.h"
#include "acx_moves.h"
#include "acx_planes.h"
#include "acx_step_args.h"
#include "acx_tile.h"

namespace acx {

// OBS: 0 no trajectory, 1 int32 obs trajectory (obs_traj), 2 int8 obs trajectory (obs_traj8)
template <int NW, int LC, int VEC, int OBS>
__global__ __launch_bounds__(BLOCK, Occupancy<LC>::waves_per_simd) void rollout_kernel(RolloutArgs a) {
    using Tile = TileFor<NW, LC, VEC>;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    WaveCtx w;
    // which block of 256 envs: blockIdx, or (a.deal.heads) the one dealt by XCC -- the store-bound
    // launch ends when the slowest XCD has stored its share, so the shares follow the XCDs' rates
    int64_t blk = (int64_t)blockIdx.x;
    if (a.deal.heads) {
        blk = xcc_deal_block(a.deal, smem);
        if (blk < 0) return;
    }
    if (!wave_ctx_at(a.B, blk, w)) return;
    Tile tile(smem + w.wid * Tile::wave_bytes(a.L), a.L);
    const int L = tile.Lr(), twoL = 2 * L;
    const int64_t env = w.r0 + w.lane;

    // starting states are read only when an episode ends (not kept in registers, which are
    // the rollout's occupancy limit): by the resetting lane alone, or by a coalesced reload of
    // the tile when many lanes of the wave reset together.
    // Errors follow acx_step exactly, so T launches of acx_step give the same trajectory: a
    // failed move (err 1, 2, 4) leaves the state and the step count as they are for that step
    // (done = truncated = 0, reward = -(n0+n1)); an out-of-domain row (err 3: the input row, or
    // a starting row an autoreset loaded -- then held as that row, count 0) never moves and
    // never counts; its observations are its exact int32 values (fallback rows, FB_*).
    bool bad = false;
    bool bad_reset = false;  // the out-of-domain row is the env's starting row (FB_RESET)
    constexpr int PW = Tile::PW;
    PlaneRegs<PW> p;
    tile.template load<false, false, true>(a.state + w.r0 * twoL, w.R, w.lane);
    int first_err = ACX_ERR_NONE;
    int cnt = 0;
    const bool cyc = a.cyclical != 0;
    bool clean = false;
    if (w.active) {
        bad = tile.pack(w.lane, p);
        cnt = a.step_count[env];
        if (bad) first_err = ACX_ERR_DOMAIN;
        clean = pl::is_clean<PW>(p.w0, p.n0, p.w1, p.n1, cyc);
    }
    const int32_t max_reward = a.horizon * L * 2;
    // Drain the prologue's loads here: otherwise the waitcnt pass carries the pending
    // step_count load around the loop back-edge and waits vmcnt(0) (= for every store of
    // the previous step) at each use of `cnt`.
    __builtin_amdgcn_s_waitcnt(0);
    const int32_t* act_tile = a.actions + w.r0;  // wave-uniform

    // One env step of the wave: move, reward/done/truncated, autoreset, obs rows.
    auto step = [&](int t, uint32_t id) {
        const int64_t ti = (int64_t)t * a.B;
        // opaque per step: keeps uniform-base + lane addressing in the loop (hoisted 64-bit
        // per-lane pointers are what the register allocator spills)
        // the lane index recomputed per step (v_mbcnt), not held across the loop: a live copy
        // was what the register allocator spilled, and its reload put a vmcnt(0) -- a drain of
        // the previous step's stores -- at the top of every step
        const int lane = (int)__lane_id();
        int ln = lane;
        asm volatile("" : "+v"(ln));
        bool reset = false;
        bool both = false;  // the LDS image needs both relators (general move: both reduced)
        bool h1 = false;    // the moved relator (ac_moves.py:167-179: i = (id + 1) & 1)
        if (w.active) {
            const int act = (int)id;
            int e;
            both = !clean;
            h1 = ((act + 1) & 1) != 0;
            if (bad) e = ACX_ERR_DOMAIN;
            else if (clean) e = pl::ac_move_clean<PW>(p.w0, p.n0, p.w1, p.n1, act, L, cyc);
            else {
                const pl::MoveOut<PW> mo = pl::ac_move_call<PW>(p, act, L, cyc);
                p = mo.p;
                e = mo.e;
            }
            const bool ok = e == ACX_ERR_NONE;
            // a successful general move leaves both relators reduced -- clean unless the
            // reduction emptied one (an unreduced input like [y^-1 y]: the reference keeps going
            // with the empty relator, utils.py:264-266 checks only before the reduction)
            clean = clean || (ok && p.n0 > 0 && p.n1 > 0);
            if (first_err == ACX_ERR_NONE) first_err = e;
            const bool triv = ok && pl::is_trivial<PW>(p.w0, p.n0, p.w1, p.n1);
            cnt += ok ? 1 : 0;  // the reference raises before count_steps += 1 (ac_env.py:93-102)
            const bool trunc = ok && cnt >= a.horizon;
            if (a.reward_traj) st_scalar<false, int32_t>(a.reward_traj + ti + w.r0 + ln, triv ? max_reward : -(p.n0 + p.n1));
            if (a.done_traj) st_scalar<false, uint8_t>(a.done_traj + ti + w.r0 + ln, (uint8_t)triv);
            if (a.trunc_traj) st_scalar<false, uint8_t>(a.trunc_traj + ti + w.r0 + ln, (uint8_t)trunc);
            reset = triv || trunc;
            if (reset) cnt = 0;
        }
        const uint64_t rb = __ballot(reset);
        bool reloaded = false;  // wave-uniform: the whole tile now holds starting rows
        if (rb) {  // same-step autoreset to the starting states
            bool rbad = false;
            if (__popcll(rb) > RESET_TILE_MIN) {  // many lanes: one coalesced tile reload
                tile.load(a.reset_state + w.r0 * twoL, w.R, lane);
                if (reset) rbad = tile.pack(lane, p);
                wave_sync();
                reloaded = true;
            } else {  // a few lanes: the wave loads just their rows
                tile.load_rows(a.reset_state + w.r0 * twoL, rb, w.R, lane);
                if (reset) rbad = tile.pack(lane, p);
            }
            if (reset) {
                clean = pl::is_clean<PW>(p.w0, p.n0, p.w1, p.n1, cyc);
                bad = rbad;
                bad_reset = rbad;
                if (rbad && first_err == ACX_ERR_NONE) first_err = ACX_ERR_DOMAIN;
            }
        }
        if constexpr (OBS != 0) {
            // the LDS tile stays the int8 image of the current states: a clean move re-images
            // its target relator, a general move both; a row reset by load_rows already holds its
            // starting row; after a whole-tile reload every row is re-imaged
            if (w.active && !bad) {
                if (reloaded || both) tile.unpack(lane, p);
                else if (!reset) tile.unpack_half(lane, p, h1);
            }
            if (__ballot(w.active && bad)) {
                // rare: out-of-domain rows as their exact values from their fallback rows
                tile.restore_flags(lane, (w.active && bad) ? (bad_reset ? FB_RESET : FB_IN) : 0u);
                if constexpr (OBS == 1)
                    tile.template store<true>(a.obs_traj + (ti + w.r0) * twoL, twoL, w.R, a.state + w.r0 * twoL, twoL,
                                              lane, a.reset_state + w.r0 * twoL);
                else
                    store_rows_i8_fb(tile, a.obs_traj8 + (ti + w.r0) * twoL, w.R, twoL, lane, a.state + w.r0 * twoL,
                                     a.reset_state + w.r0 * twoL);
                wave_sync();
                return;
            }
            wave_sync();
            if constexpr (OBS == 1) {
                tile.template store_rows<NT_OBS>(a.obs_traj + (ti + w.r0) * twoL, w.R, lane);
            } else {
                tile.template store_rows_i8<NT_OBS>(a.obs_traj8 + (ti + w.r0) * twoL, w.R, lane);
            }
            wave_sync();
        }
    };
    // ids outside [0,12) -> 15 (ACX_ERR_ACTION in ac_move)
    auto decode = [](int32_t v) { return (uint32_t)v < 12u ? (uint32_t)v : 15u; };

    // Move ids are loaded ACT_BLOCK steps at a time and kept packed, 4 bits each, in
    // ACT_BLOCK/8 registers.  The wait for a load issued after trajectory stores covers those
    // stores too (loads and stores pending on vmcnt may complete out of order, so the
    // compiler waits vmcnt(0)): a drain of the wave's write queue.  8-step batches cost 8 %
    // of the rollout in drains (tools/store_pattern.py, ACT8 vs none); with obs stores the
    // batch is 32 steps, loaded as four groups of 8 (only the first wait finds stores).
    constexpr int ACT_BLOCK = OBS != 0 ? 32 : 8;
    constexpr int ACT_GROUP = 8;
    constexpr int QW = ACT_BLOCK / 8;
    uint32_t q[QW];
#pragma unroll
    for (int k = 0; k < QW; ++k) q[k] = 0;
    for (int t = 0; t < a.T; ++t) {
        if ((t & (ACT_BLOCK - 1)) == 0) {
            // recomputed (v_mbcnt), not kept live across the loop
            int lc = (int)__lane_id();
            lc = lc < w.R ? lc : 0;
            if (a.packed) {  // one uint32 per 8 steps (acx_pack_actions)
                const uint32_t* pk = a.packed + (int64_t)(t >> 3) * a.B + w.r0;
#pragma unroll
                for (int g = 0; g < QW; ++g) q[g] = t + 8 * g < a.T ? (pk + (int64_t)g * a.B)[lc] : 0u;
            } else {
#pragma unroll
            for (int g = 0; g < ACT_BLOCK / ACT_GROUP; ++g) {
                int32_t v[ACT_GROUP];
#pragma unroll
                for (int k = 0; k < ACT_GROUP; ++k) {
                    const int tk = t + g * ACT_GROUP + k;
                    v[k] = tk < a.T ? (act_tile + (int64_t)tk * a.B)[lc] : 0;
                }
                uint32_t qg = 0;
#pragma unroll
                for (int k = 0; k < ACT_GROUP; ++k) qg |= decode(v[k]) << (4 * k);
                q[g] = qg;
            }
            }
            // consume the loaded words here: otherwise the waitcnt pass sees them pending where
            // this block rejoins the step and puts a vmcnt(0) on the first use of the move id in
            // EVERY step (a drain of the wave's previous trajectory stores per step)
#pragma unroll
            for (int k = 0; k < QW; ++k) asm volatile("" ::"v"(q[k]));
        }
        const uint32_t id = q[0] & 15u;
#pragma unroll
        for (int k = 0; k < QW; ++k) q[k] = (q[k] >> 4) | (k + 1 < QW ? q[k + 1] << 28 : 0u);
        step(t, id);
    }
    if (w.active) {
        if (!bad) tile.unpack(w.lane, p);
        a.step_count[env] = cnt;
        if (a.err) a.err[env] = (uint8_t)first_err;
        if (first_err != ACX_ERR_NONE && a.err_count) atomicAdd(a.err_count, 1);
    }
    // out-of-domain rows: their input row (untouched in HBM), or the starting row they reset to
    tile.restore_flags(w.lane, (w.active && bad) ? (bad_reset ? FB_RESET : FB_IN) : 0u);
    tile.template store<true, NT_STATE>(a.state + w.r0 * twoL, twoL, w.R, a.state + w.r0 * twoL, twoL,
                                                 w.lane, a.reset_state + w.r0 * twoL);
}

// Move ids (T, B) int32 -> (ceil(T/8), B) uint32, 8 consecutive steps of one env per word,
// 4 bits each (ids outside [0,12) -> 15, ACX_ERR_ACTION).  The rollout then reads 0.5 B per
// env-step instead of 4: its action reads are small scattered requests between trajectory
// write bursts, and at 4 B they cost 7 % of the rollout (tools/store_pattern.py ACT8 vs
// PACK8); this pass streams them once.
__device__ __forceinline__ uint32_t pack_id(int32_t v) { return (uint32_t)v < 12u ? (uint32_t)v : 15u; }

// VEC4: four consecutive envs per thread with 16-byte loads/stores (B % 4 == 0, aligned)
template <bool VEC4>
__global__ __launch_bounds__(256) void pack_actions_kernel(const int32_t* __restrict__ actions,
                                                           uint32_t* __restrict__ packed, int T, int64_t B) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int t0 = (int)blockIdx.y * 8;
    if constexpr (VEC4) {
        if (4 * i >= B) return;
        const int4* src = reinterpret_cast<const int4*>(actions) + i;
        const int64_t row4 = B / 4;
        int4 v[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) v[k] = t0 + k < T ? src[(int64_t)(t0 + k) * row4] : make_int4(0, 0, 0, 0);
        uint4 q = make_uint4(0, 0, 0, 0);
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            if (t0 + k >= T) continue;
            q.x |= pack_id(v[k].x) << (4 * k);
            q.y |= pack_id(v[k].y) << (4 * k);
            q.z |= pack_id(v[k].z) << (4 * k);
            q.w |= pack_id(v[k].w) << (4 * k);
        }
        reinterpret_cast<uint4*>(packed + (int64_t)blockIdx.y * B)[i] = q;
    } else {
        if (i >= B) return;
        int32_t v[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) v[k] = t0 + k < T ? actions[(int64_t)(t0 + k) * B + i] : 0;
        uint32_t q = 0;
#pragma unroll
        for (int k = 0; k < 8; ++k) q |= (t0 + k < T ? pack_id(v[k]) : 0u) << (4 * k);
        packed[(int64_t)blockIdx.y * B + i] = q;
    }
}

}  // namespace acx
