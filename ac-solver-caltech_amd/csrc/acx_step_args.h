// acx_step_args.h -- the argument structs of the env-side kernels (step, rollout, expand12,
// canonicalize, unpack: acx_kernels.hip's header comment maps their headers).  They are passed by
// value as kernel arguments: field order and types fix the offsets the compiled kernels read.
#pragma once
#include <stdint.h>

namespace acx {

struct StepArgs {
    const int32_t* state_in;
    int32_t* state_out;
    const int32_t* action;
    const int32_t* reset_state;
    int32_t* step_count;
    int32_t* reward;
    uint8_t* done;
    uint8_t* truncated;
    int32_t* lengths_out;
    int32_t* final_obs;
    uint8_t* err;
    int32_t* err_count;
    // learner-side outputs (acx_step_learner; all NULL for acx_step)
    const int64_t* action64;
    float* obs_f32;
    float* reward_f32;
    float* done_f32;
    uint8_t* action_hist;
    int32_t* episode_len;
    int64_t B;
    int L, horizon, cyclical, hist_cap;
    // acx_learner_step: the round-1 curriculum fused into the step (training.py:319-352).
    // cur_ws NULL: none.  cur_ws: the uint64 words of acx_cur_layout.h (the launch sequence number,
    // the tiles' counts, the groups' totals and arrival words; cur_publish, cur_prefix)
    uint64_t* cur_ws;
    const int32_t* cur_states;  // (n_states, 2L) initial states
    int64_t n_states;
    int32_t* cur_next;          // [1] max(states_processed) + 1
    int32_t* curr_index;        // (B)
    uint8_t* needs_host;        // (B)
    // state_out == state_in (set by the launcher): the state store writes changed relators only
    int in_place;
    // next-step autoreset (acx_step_next; NULL: same-step): per env, its episode ended on the
    // previous call -- this call resets it instead of stepping, and records whether it ends now
    uint8_t* pending;
    // lengths-carrying step (acx_step_lengths): lengths_out holds the rows' relator lengths on
    // entry (canonical rows), so only their letters are read and written
    int live;
    // move-history ring (NULL: move k of an episode at row k): per env, the row of its current
    // episode's move 0; an episode's first move sets it to hist_t mod hist_cap (hist_t: the
    // caller's step counter), so envs whose episodes are out of phase still write this step's
    // moves to one row -- coalesced -- instead of one cache line per lane
    int32_t* hist_base;
    int64_t hist_t;
    // tests only (acx_internal_learner_ranking_fails): ranking waits give up at once, as one that
    // polled 2^20 times would (1: every wait, needs_host = 3; 2: only the last tile's total)
    int cur_fail;
    // acx_step_lengths_reduced (live steps only; NULL: none): per env, bit 0 = both relators are
    // non-empty and freely reduced, bit 1 = and cyclically reduced, as the previous step left them.
    // A conjugation of such a row reads only its target relator (step_body).  Written every call.
    uint8_t* reduced;
};

// The rollout's XCC deal (acx_kernel_common.h xcc_deal_block; filled by launch_rollout).  heads NULL:
// the plain deal, block = blockIdx.  heads: the caller's workspace (ACX_ROLLOUT_DEAL_WORDS uint32,
// zeroed on the launch's stream before the kernel), range x's head counter at word
// x * XCC_HEAD_STRIDE -- a cache line each, so the XCDs' atomics do not queue on one line.
// bound: the ranges' limits, bound[0] = 0 <= ... <= bound[8] = blocks of the batch.
constexpr uint32_t XCC_RANGES = 8;
constexpr uint32_t XCC_HEAD_STRIDE = 32;
struct XccDeal {
    uint32_t* heads;
    uint32_t bound[XCC_RANGES + 1];
};

struct RolloutArgs {
    int32_t* state;
    const int32_t* actions;
    const uint32_t* packed;  // or: move ids pre-packed by pack_actions_kernel (actions unused)
    const int32_t* reset_state;
    int32_t* step_count;
    int32_t* obs_traj;
    int32_t* reward_traj;
    uint8_t* done_traj;
    uint8_t* trunc_traj;
    uint8_t* err;
    int32_t* err_count;
    int64_t B;
    int T, L, horizon, cyclical;
    int8_t* obs_traj8;  // acx_rollout_obs8: the trajectory as int8 letters (obs_traj unused)
    XccDeal deal;       // acx_rollout_deal (heads NULL: block = blockIdx)
};

struct ExpandArgs {
    const int32_t* parents;
    int32_t* children;
    int32_t* child_len;
    uint64_t* child_key;
    uint8_t* err;
    int32_t* err_count;
    int64_t N;
    int L, cyclical, kw64;
};

struct CanonArgs {
    const int32_t* state_in;
    int32_t* state_out;
    int32_t* lengths_out;
    uint8_t* err;
    int32_t* err_count;
    int64_t B;
    int L, cyclical;
};

struct UnpackArgs {
    const uint64_t* keys;
    int32_t* states;
    int32_t* lengths_out;
    int64_t M;
    int L, kw64;
};

}  // namespace acx
