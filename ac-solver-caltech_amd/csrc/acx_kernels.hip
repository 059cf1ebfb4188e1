// acx_kernels.hip -- MI355X (gfx950) kernels for the Andrews-Curtis environment hot path.
//
// Design (DESIGN.md has the full story):
//   * HBM holds presentations as (B, 2L) int32 rows (the tensor the Python host owns).
//   * One wavefront handles a tile of 64 envs, one env per lane.  The tile is staged
//     through LDS with coalesced 16-byte loads/stores (a row is 2L int32 = 288 B at
//     L = 36, so a lane reading "its" row directly would touch 64 lines per load);
//     in LDS each letter is one int8, rows padded to an odd number of dwords so the
//     per-lane row reads are bank-conflict free.
//   * Each lane then packs its two relators into registers.  The expansion kernels (expand12*,
//     canon, unpack_keys) hold a relator at 2 bits per letter (x=0, x^-1=1, y=2, y^-1=3, so
//     inversion is `code ^ 1`), as little multiword integers Word<NW> (acx_moves.h: NW 32-bit
//     words, letter k at bits [2k, 2k+2)).  The step and rollout kernels hold it as two bit
//     planes (acx_planes.h: sign and generator masks, letter k at bit k) and run the same moves
//     on them.
//   * A move is O(NW) register work, no per-letter loops (on Word<NW>; the planes likewise):
//       concatenate r_i <- r_i r_j^{+-1}  (reference ac_moves.py:4-76): the junction
//         cancellation count is the first non-zero letter of
//         reverse(r_i) XOR r_j^{+-1} XOR 0x55..  (count-trailing-zeros), the splice is
//         mask | shift;
//       conjugate r_i <- g r_i g^-1 (ac_moves.py:79-156): first/last letter tests + splice;
//       free reduction (utils.py:211-220): a SWAR "adjacent inverse pair" mask; the loop
//         only runs when that mask is non-zero, which needs an unreduced input (moves
//         keep reduced words reduced);
//       cyclic reduction (utils.py:223-232): peel count = first non-zero letter of
//         w XOR reverse(w) XOR 0x55.. .
//   * No MFMA: the path is integer/byte work and HBM-bound.
//
// This file is the one translation unit of the env-side kernels (build.py compiles it once more
// per -DACX_PART=n).  Everything but the C-ABI is in headers, one concern each, bottom layer first:
//   acx_moves.h, acx_planes.h   the word algebra (Word<NW> / bit planes)
//   acx_tile_io.h               HBM <-> LDS staging helpers and their cache-policy constants
//   acx_tile_base.h             what FastTile and CodeTile share
//   acx_tile_code.h, acx_tile_fast.h, acx_tile_generic.h   the three LDS tile classes
//   acx_tile.h                  the interface they share, and TileFor, which picks one by L
//   acx_step_args.h             the kernels' argument structs
//   acx_cur_layout.h            the fused learner's workspace layout
//   acx_kernel_common.h         the per-wave prologue (WaveCtx) and other bits the kernels share
//   acx_cur_rank.h              the learner's ranking inside the step kernel
//   acx_step_kernel.h           step_body, step_kernel, step_lengths_kernel
//   acx_step_pair.h             step_pair_kernel: two lanes per env, small batches
//   acx_rollout_kernel.h        rollout_kernel, pack_actions_kernel
//   acx_expand_kernels.h        the four expand12 kernels, canon_kernel, unpack_keys_kernel
//   acx_launch.h                dispatch by L, the launchers, the -DACX_PART=n instantiation table
// Here: the C-ABI (include/acx.h), main object only -- argument checks, then a launcher.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <new>

#include "acx.h"

#include "acx_cur_layout.h"
#include "acx_expand_kernels.h"
#include "acx_launch.h"
#include "acx_rollout_kernel.h"
#include "acx_step_args.h"

#ifndef ACX_PART  // the C-ABI lives in the main object only
using namespace acx;

// ---- the entries' argument checks (a failed check is ACX_E_ARG; B == 0 is ACX_OK once the
// ---- ranges hold, before any pointer is looked at) ----
static bool dims_ok(int64_t B, int32_t L) { return B >= 0 && L >= 1 && L <= ACX_MAX_L; }
// a required buffer of rows: present and 16-byte aligned
static bool rows16(const void* p) { return p && aligned16(p); }
static bool hist_range_ok(int32_t hist_cap, int64_t hist_t) { return hist_cap >= 0 && hist_t >= 0; }

// The three plain step kinds (ACX_STEP_PLAN_*: acx_step, acx_step_lengths, acx_step_lengths_reduced):
// checks the kind's arguments and fills `a` with all of them but the move ids.  Called by the entry
// itself and by acx_step_plan_create, so a plan is checked exactly as its entry.  The lengths kinds
// are in place (state_out == state_in) and need lengths; reduced is _LENGTHS_REDUCED's alone.
static int plain_step_args(StepArgs& a, int32_t kind, const int32_t* state_in, int32_t* state_out,
                           const int32_t* reset_state, int32_t* step_count, int32_t* reward, uint8_t* done,
                           uint8_t* truncated, int32_t* lengths, uint8_t* reduced, int32_t* final_obs, uint8_t* err,
                           int32_t* err_count, int64_t B, int32_t L, int32_t horizon, int32_t cyclical) {
    const bool live = kind != ACX_STEP_PLAN_STEP, with_reduced = kind == ACX_STEP_PLAN_LENGTHS_REDUCED;
    if (!dims_ok(B, L) || (!with_reduced && reduced)) return ACX_E_ARG;
    if (B > 0) {
        if (!rows16(state_in) || !rows16(state_out)) return ACX_E_ARG;
        if (reset_state && !step_count) return ACX_E_ARG;
        if (live && (state_out != state_in || !lengths)) return ACX_E_ARG;
        if (with_reduced && !reduced) return ACX_E_ARG;
    }
    a.state_in = state_in;
    a.state_out = state_out;
    a.reset_state = reset_state;
    a.step_count = step_count;
    a.reward = reward;
    a.done = done;
    a.truncated = truncated;
    a.lengths_out = lengths;
    a.final_obs = final_obs;
    a.err = err;
    a.err_count = err_count;
    a.B = B;
    a.L = L;
    a.horizon = horizon;
    a.cyclical = cyclical;
    a.live = live ? 1 : 0;
    a.reduced = reduced;
    return ACX_OK;
}

// a plain step from checked arguments and this call's move ids
static int launch_plain_step(StepArgs a, const int32_t* action, void* stream) {
    if (a.B == 0) return ACX_OK;
    if (!action) return ACX_E_ARG;
    a.action = action;
    StepLaunch f{a, (hipStream_t)stream, false};
    return dispatch(a.L, f);
}

// the move history of the entries that record one (checked by the entry)
static void set_history(StepArgs& a, uint8_t* action_hist, int32_t hist_cap, int32_t* hist_base, int64_t hist_t,
                        int32_t* episode_len) {
    a.action_hist = action_hist;
    a.hist_cap = hist_cap;
    a.hist_base = hist_base;
    a.hist_t = hist_t;
    a.episode_len = episode_len;
}

// acx_step_learner and acx_learner_step: the arguments they share, checked and filled (in place)
static int learner_step_args(StepArgs& a, int32_t* state, const int32_t* action, const int64_t* action_i64,
                             const int32_t* reset_state, int32_t* step_count, float* obs_f32, float* reward_f32,
                             float* done_f32, uint8_t* done, uint8_t* truncated, uint8_t* action_hist,
                             int32_t hist_cap, int32_t* hist_base, int64_t hist_t, int32_t* episode_len, uint8_t* err,
                             int32_t* err_count, int64_t B, int32_t L, int32_t horizon, int32_t cyclical) {
    if (!dims_ok(B, L) || !hist_range_ok(hist_cap, hist_t) || (hist_base && !action_hist)) return ACX_E_ARG;
    if (B == 0) return ACX_OK;
    if (!rows16(state) || !step_count || (!action == !action_i64) || (action_hist && hist_cap == 0)) return ACX_E_ARG;
    if (obs_f32 && !aligned16(obs_f32)) return ACX_E_ARG;
    a.state_in = state;
    a.state_out = state;
    a.action = action;
    a.reset_state = reset_state;
    a.step_count = step_count;
    a.done = done;
    a.truncated = truncated;
    a.err = err;
    a.err_count = err_count;
    a.action64 = action_i64;
    a.obs_f32 = obs_f32;
    a.reward_f32 = reward_f32;
    a.done_f32 = done_f32;
    a.B = B;
    a.L = L;
    a.horizon = horizon;
    a.cyclical = cyclical;
    set_history(a, action_hist, hist_cap, hist_base, hist_t, episode_len);
    return ACX_OK;
}

// The three rollout entries (acx_rollout, acx_rollout_packed, acx_rollout_obs8): the checks they
// share, and `a` filled with every argument.  B == 0 or T == 0 is ACX_OK once the ranges hold, before
// any pointer is looked at.  Which of actions / packed_actions / obs_traj / obs_traj8 an entry requires
// is its own check.
static int rollout_args(RolloutArgs& a, int32_t* state, const int32_t* actions, const uint32_t* packed_actions,
                        const int32_t* reset_state, int32_t* step_count, int32_t* obs_traj, int8_t* obs_traj8,
                        int32_t* reward_traj, uint8_t* done_traj, uint8_t* trunc_traj, uint8_t* err,
                        int32_t* err_count, int32_t T, int64_t B, int32_t L, int32_t horizon, int32_t cyclical) {
    if (!dims_ok(B, L) || T < 0) return ACX_E_ARG;
    if (B == 0 || T == 0) return ACX_OK;
    if (!rows16(state) || !rows16(reset_state) || !step_count) return ACX_E_ARG;
    if ((obs_traj && !aligned16(obs_traj)) || (obs_traj8 && !aligned16(obs_traj8))) return ACX_E_ARG;
    a.state = state;
    a.actions = actions;
    a.packed = packed_actions;
    a.reset_state = reset_state;
    a.step_count = step_count;
    a.obs_traj = obs_traj;
    a.obs_traj8 = obs_traj8;
    a.reward_traj = reward_traj;
    a.done_traj = done_traj;
    a.trunc_traj = trunc_traj;
    a.err = err;
    a.err_count = err_count;
    a.B = B;
    a.T = T;
    a.L = L;
    a.horizon = horizon;
    a.cyclical = cyclical;
    return ACX_OK;
}

extern "C" {

int32_t acx_key_words(int32_t L) { return key_words(L); }

// build provenance: build.py passes the sha256 of the sources this library is compiled from
#ifndef ACX_SOURCE_HASH
#define ACX_SOURCE_HASH "unknown"
#endif
const char* acx_version(void) { return "acx 0.3 gfx950 acx-src-sha256:" ACX_SOURCE_HASH; }

int acx_step(const int32_t* state_in, int32_t* state_out, const int32_t* action, const int32_t* reset_state,
             int32_t* step_count, int32_t* reward, uint8_t* done, uint8_t* truncated, int32_t* lengths_out,
             int32_t* final_obs, uint8_t* err, int32_t* err_count, int64_t B, int32_t L, int32_t horizon,
             int32_t cyclical, void* stream) {
    StepArgs a{};
    const int rc = plain_step_args(a, ACX_STEP_PLAN_STEP, state_in, state_out, reset_state, step_count, reward, done,
                                   truncated, lengths_out, nullptr, final_obs, err, err_count, B, L, horizon, cyclical);
    return rc != ACX_OK ? rc : launch_plain_step(a, action, stream);
}

int acx_step_lengths(int32_t* state, const int32_t* action, const int32_t* reset_state, int32_t* step_count,
                     int32_t* reward, uint8_t* done, uint8_t* truncated, int32_t* lengths, int32_t* final_obs,
                     uint8_t* err, int32_t* err_count, int64_t B, int32_t L, int32_t horizon, int32_t cyclical,
                     void* stream) {
    StepArgs a{};
    const int rc = plain_step_args(a, ACX_STEP_PLAN_LENGTHS, state, state, reset_state, step_count, reward, done,
                                   truncated, lengths, nullptr, final_obs, err, err_count, B, L, horizon, cyclical);
    return rc != ACX_OK ? rc : launch_plain_step(a, action, stream);
}

int acx_step_lengths_reduced(int32_t* state, const int32_t* action, const int32_t* reset_state, int32_t* step_count,
                             int32_t* reward, uint8_t* done, uint8_t* truncated, int32_t* lengths, uint8_t* reduced,
                             int32_t* final_obs, uint8_t* err, int32_t* err_count, int64_t B, int32_t L,
                             int32_t horizon, int32_t cyclical, void* stream) {
    StepArgs a{};
    const int rc = plain_step_args(a, ACX_STEP_PLAN_LENGTHS_REDUCED, state, state, reset_state, step_count, reward, done,
                                   truncated, lengths, reduced, final_obs, err, err_count, B, L, horizon, cyclical);
    return rc != ACX_OK ? rc : launch_plain_step(a, action, stream);
}

// a per-call step with everything but the move ids resolved once (acx.h): the launch is then a
// three-argument call -- at 65,536 envs a caller's ctypes call with 17 arguments took as long as
// half the kernel, and the host, not the GPU, set the eager rate
struct acx_step_plan {
    StepArgs a;  // checked and filled by plain_step_args; action is the launch's
};

acx_step_plan* acx_step_plan_create(int32_t kind, const int32_t* state_in, int32_t* state_out,
                                    const int32_t* reset_state, int32_t* step_count, int32_t* reward, uint8_t* done,
                                    uint8_t* truncated, int32_t* lengths, uint8_t* reduced, int32_t* final_obs,
                                    uint8_t* err, int32_t* err_count, int64_t B, int32_t L, int32_t horizon,
                                    int32_t cyclical) {
    // the checks of the kind's entry (acx_step / acx_step_lengths / _reduced), made once
    if (kind < ACX_STEP_PLAN_STEP || kind > ACX_STEP_PLAN_LENGTHS_REDUCED) return nullptr;
    StepArgs a{};
    if (plain_step_args(a, kind, state_in, state_out, reset_state, step_count, reward, done, truncated, lengths, reduced,
                        final_obs, err, err_count, B, L, horizon, cyclical) != ACX_OK)
        return nullptr;
    return new (std::nothrow) acx_step_plan{a};
}

int acx_step_plan_launch(const acx_step_plan* p, const int32_t* action, void* stream) {
    return p ? launch_plain_step(p->a, action, stream) : ACX_E_ARG;
}

void acx_step_plan_destroy(acx_step_plan* p) { delete p; }

int acx_step_next(const int32_t* state_in, int32_t* state_out, const int32_t* action, const int32_t* reset_state,
                  int32_t* step_count, int32_t* reward, uint8_t* done, uint8_t* truncated, int32_t* lengths_out,
                  uint8_t* pending, uint8_t* action_hist, int32_t hist_cap, int32_t* hist_base, int64_t hist_t,
                  int32_t* episode_len, uint8_t* err, int32_t* err_count, int64_t B, int32_t L, int32_t horizon,
                  int32_t cyclical, void* stream) {
    if (!hist_range_ok(hist_cap, hist_t) || (hist_base && !action_hist)) return ACX_E_ARG;
    // acx_step's arguments (no final_obs), then this entry's own
    StepArgs a{};
    const int rc = plain_step_args(a, ACX_STEP_PLAN_STEP, state_in, state_out, reset_state, step_count, reward, done,
                                   truncated, lengths_out, nullptr, nullptr, err, err_count, B, L, horizon, cyclical);
    if (rc != ACX_OK || B == 0) return rc;
    if (!action || !reset_state || !step_count || !pending) return ACX_E_ARG;
    if ((action_hist != nullptr) != (hist_cap > 0) || (episode_len && !action_hist)) return ACX_E_ARG;
    a.action = action;
    a.pending = pending;
    set_history(a, action_hist, hist_cap, hist_base, hist_t, episode_len);
    // with a move history: the learner instantiation (it compiles the history writes)
    StepLaunch f{a, (hipStream_t)stream, action_hist != nullptr};
    return dispatch(L, f);
}

int acx_step_learner(int32_t* state, const int32_t* action, const int64_t* action_i64, const int32_t* reset_state,
                     int32_t* step_count, float* obs_f32, float* reward_f32, float* done_f32, uint8_t* done,
                     uint8_t* truncated, uint8_t* action_hist, int32_t hist_cap, int32_t* hist_base, int64_t hist_t,
                     int32_t* episode_len, int32_t* final_obs, uint8_t* err, int32_t* err_count, int64_t B, int32_t L,
                     int32_t horizon, int32_t cyclical, void* stream) {
    StepArgs a{};
    const int rc = learner_step_args(a, state, action, action_i64, reset_state, step_count, obs_f32, reward_f32, done_f32,
                                     done, truncated, action_hist, hist_cap, hist_base, hist_t, episode_len, err,
                                     err_count, B, L, horizon, cyclical);
    if (rc != ACX_OK || B == 0) return rc;
    a.final_obs = final_obs;
    StepLaunch f{a, (hipStream_t)stream, true};
    return dispatch(L, f);
}

int acx_step_record(const int32_t* state_in, int32_t* state_out, const int32_t* action, const int32_t* reset_state,
                    int32_t* step_count, int32_t* reward, uint8_t* done, uint8_t* truncated, int32_t* lengths_out,
                    int32_t* final_obs, uint8_t* action_hist, int32_t hist_cap, int32_t* hist_base, int64_t hist_t,
                    int32_t* episode_len, uint8_t* err, int32_t* err_count, int64_t B, int32_t L, int32_t horizon,
                    int32_t cyclical, void* stream) {
    if (!hist_range_ok(hist_cap, hist_t)) return ACX_E_ARG;
    // the learner instantiation (it compiles the history writes) with the plain step's arguments
    StepArgs a{};
    const int rc = plain_step_args(a, ACX_STEP_PLAN_STEP, state_in, state_out, reset_state, step_count, reward, done,
                                   truncated, lengths_out, nullptr, final_obs, err, err_count, B, L, horizon, cyclical);
    if (rc != ACX_OK || B == 0) return rc;
    if (!action || !step_count || !action_hist || hist_cap == 0) return ACX_E_ARG;
    a.action = action;
    set_history(a, action_hist, hist_cap, hist_base, hist_t, episode_len);
    StepLaunch f{a, (hipStream_t)stream, true};
    return dispatch(L, f);
}

// acx_curriculum.hip: where acx_learner_step's part of the shared workspace starts (int32 words)
int64_t acx_internal_curriculum_fused_offset(int64_t B);

// int32 words into the workspace: the fused part's uint64 word cur_layout::FAILED
int64_t acx_learner_failure_word(int64_t B) {
    return acx_internal_curriculum_fused_offset(B) + 2 * cur_layout::FAILED;
}

static int g_learner_fail = 0;  // tests only
// tests only: acx_learner_step's ranking polls give up at once: 1 every one, 2 only the last tile's
// total (next_index), 0 none
void acx_internal_learner_ranking_fails(int32_t on) { g_learner_fail = on; }

int acx_learner_step(int32_t* state, const int32_t* action, const int64_t* action_i64, int32_t* reset_state,
                     int32_t* step_count, float* obs_f32, float* reward_f32, float* done_f32, uint8_t* done,
                     uint8_t* truncated, uint8_t* action_hist, int32_t hist_cap, int32_t* hist_base, int64_t hist_t,
                     int32_t* episode_len, uint8_t* err, int32_t* err_count, const int32_t* curriculum_states,
                     int64_t n_states, int32_t* next_index, int32_t* curr_index, uint8_t* needs_host,
                     int32_t* workspace, int64_t B, int32_t L, int32_t horizon, int32_t cyclical, void* stream) {
    if (n_states < 0 || n_states > INT32_MAX) return ACX_E_ARG;
    if (B >= (1ll << 31)) return ACX_E_ARG;  // the look-back's 32-bit prefixes (next_index + finished envs)
    StepArgs a{};
    const int rc = learner_step_args(a, state, action, action_i64, reset_state, step_count, obs_f32, reward_f32, done_f32,
                                     done, truncated, action_hist, hist_cap, hist_base, hist_t, episode_len, err,
                                     err_count, B, L, horizon, cyclical);
    if (rc != ACX_OK || B == 0) return rc;
    if (!done || !truncated || !reset_state || !curriculum_states || !next_index || !curr_index || !needs_host ||
        !workspace)
        return ACX_E_ARG;
    if ((L % 2) == 0 && (!aligned16(reset_state) || !aligned16(curriculum_states))) return ACX_E_ARG;  // int4 row copies
    // one launch: the step kernel ranks the finished envs itself (cur_publish / cur_prefix) in its part of the
    // workspace (acx_curriculum_workspace(B) int32 words, zeroed before the first call, 8-byte aligned)
    int32_t* ws = workspace + acx_internal_curriculum_fused_offset(B);
    if ((reinterpret_cast<uintptr_t>(ws) & 7u) != 0) return ACX_E_ARG;
    a.cur_ws = reinterpret_cast<uint64_t*>(ws);
    a.cur_states = curriculum_states;
    a.n_states = n_states;
    a.cur_next = next_index;
    a.curr_index = curr_index;
    a.needs_host = needs_host;
    a.cur_fail = g_learner_fail;
    StepLaunch f{a, (hipStream_t)stream, true};
    return dispatch(L, f);
}

int acx_rollout(int32_t* state, const int32_t* actions, const int32_t* reset_state, int32_t* step_count,
                int32_t* obs_traj, int32_t* reward_traj, uint8_t* done_traj, uint8_t* trunc_traj, uint8_t* err,
                int32_t* err_count, int32_t T, int64_t B, int32_t L, int32_t horizon, int32_t cyclical,
                void* stream) {
    RolloutArgs a{};
    const int rc = rollout_args(a, state, actions, nullptr, reset_state, step_count, obs_traj, nullptr, reward_traj,
                                done_traj, trunc_traj, err, err_count, T, B, L, horizon, cyclical);
    if (rc != ACX_OK || B == 0 || T == 0) return rc;
    if (!actions) return ACX_E_ARG;
    RolloutLaunch f{a, (hipStream_t)stream};
    return dispatch(L, f);
}

int64_t acx_packed_actions_words(int32_t T, int64_t B) { return T <= 0 || B <= 0 ? 0 : (int64_t)((T + 7) / 8) * B; }

int acx_pack_actions(const int32_t* actions, uint32_t* packed, int32_t T, int64_t B, void* stream) {
    if (B < 0 || T < 0) return ACX_E_ARG;
    if (B == 0 || T == 0) return ACX_OK;
    if (!actions || !packed || (T + 7) / 8 > 65535) return ACX_E_ARG;
    if (B % 4 == 0 && aligned16(actions) && aligned16(packed)) {
        const dim3 grid((unsigned)((B / 4 + 255) / 256), (unsigned)((T + 7) / 8));
        pack_actions_kernel<true><<<grid, dim3(256), 0, (hipStream_t)stream>>>(actions, packed, T, B);
    } else {
        const dim3 grid((unsigned)((B + 255) / 256), (unsigned)((T + 7) / 8));
        pack_actions_kernel<false><<<grid, dim3(256), 0, (hipStream_t)stream>>>(actions, packed, T, B);
    }
    return finish_launch();
}

int acx_rollout_packed(int32_t* state, const uint32_t* packed_actions, const int32_t* reset_state,
                       int32_t* step_count, int32_t* obs_traj, int32_t* reward_traj, uint8_t* done_traj,
                       uint8_t* trunc_traj, uint8_t* err, int32_t* err_count, int32_t T, int64_t B, int32_t L,
                       int32_t horizon, int32_t cyclical, void* stream) {
    RolloutArgs a{};
    const int rc = rollout_args(a, state, nullptr, packed_actions, reset_state, step_count, obs_traj, nullptr,
                                reward_traj, done_traj, trunc_traj, err, err_count, T, B, L, horizon, cyclical);
    if (rc != ACX_OK || B == 0 || T == 0) return rc;
    if (!packed_actions) return ACX_E_ARG;
    RolloutLaunch f{a, (hipStream_t)stream};
    return dispatch(L, f);
}

int acx_rollout_obs8(int32_t* state, const int32_t* actions, const uint32_t* packed_actions, const int32_t* reset_state,
                     int32_t* step_count, int8_t* obs_traj8, int32_t* reward_traj, uint8_t* done_traj,
                     uint8_t* trunc_traj, uint8_t* err, int32_t* err_count, int32_t T, int64_t B, int32_t L,
                     int32_t horizon, int32_t cyclical, void* stream) {
    RolloutArgs a{};
    const int rc = rollout_args(a, state, actions, packed_actions, reset_state, step_count, nullptr, obs_traj8,
                                reward_traj, done_traj, trunc_traj, err, err_count, T, B, L, horizon, cyclical);
    if (rc != ACX_OK || B == 0 || T == 0) return rc;
    if (!obs_traj8 || (!actions == !packed_actions)) return ACX_E_ARG;
    RolloutLaunch f{a, (hipStream_t)stream};
    return dispatch(L, f);
}

static bool deal_ok(int32_t deal, int32_t pct, int32_t over_pct) {
    return deal >= ACX_DEAL_PLAIN && deal <= ACX_DEAL_AUTO && pct >= 0 && pct <= 100 && over_pct >= 100 &&
           over_pct <= 400;
}

int acx_rollout_deal(int32_t* state, const int32_t* actions, const uint32_t* packed_actions, const int32_t* reset_state,
                     int32_t* step_count, int32_t* obs_traj, int8_t* obs_traj8, int32_t* reward_traj,
                     uint8_t* done_traj, uint8_t* trunc_traj, uint8_t* err, int32_t* err_count, int32_t T, int64_t B,
                     int32_t L, int32_t horizon, int32_t cyclical, int32_t deal, int32_t pct, int32_t over_pct,
                     uint32_t* deal_ws, void* stream) {
    if (!deal_ok(deal, pct, over_pct)) return ACX_E_ARG;
    RolloutArgs a{};
    const int rc = rollout_args(a, state, actions, packed_actions, reset_state, step_count, obs_traj, obs_traj8,
                                reward_traj, done_traj, trunc_traj, err, err_count, T, B, L, horizon, cyclical);
    if (rc != ACX_OK || B == 0 || T == 0) return rc;
    if ((!actions == !packed_actions) || (obs_traj && obs_traj8)) return ACX_E_ARG;
    if (deal != ACX_DEAL_PLAIN && (!deal_ws || ((uintptr_t)deal_ws & 3u))) return ACX_E_ARG;
    RolloutLaunch f{a, (hipStream_t)stream, DealRequest{deal, pct, over_pct, deal_ws, nullptr}};
    return dispatch(L, f);
}

int acx_rollout_deal_info(int32_t T, int64_t B, int32_t L, int32_t obs_kind, int32_t deal, int32_t pct,
                          int32_t over_pct, int64_t* info) {
    if (!dims_ok(B, L) || T < 0 || obs_kind < 0 || obs_kind > 2 || !deal_ok(deal, pct, over_pct) || !info)
        return ACX_E_ARG;
    // only which kernel and how many blocks matter here: the trajectory pointers pick the kernel
    RolloutArgs a{};
    a.B = B;
    a.T = T;
    a.L = L;
    a.obs_traj = obs_kind == 1 ? reinterpret_cast<int32_t*>(info) : nullptr;
    a.obs_traj8 = obs_kind == 2 ? reinterpret_cast<int8_t*>(info) : nullptr;
    RolloutLaunch f{a, nullptr, DealRequest{deal, pct, over_pct, nullptr, info}};
    return dispatch(L, f);
}

int acx_expand12(const int32_t* parents, int32_t* children, int32_t* child_len, uint64_t* child_key, uint8_t* err,
                 int32_t* err_count, int64_t N, int32_t L, int32_t cyclical, void* stream) {
    if (!dims_ok(N, L)) return ACX_E_ARG;
    if (N == 0) return ACX_OK;
    if (!parents || !aligned16(parents) || (children && !aligned16(children))) return ACX_E_ARG;
    ExpandArgs a{parents, children, child_len, child_key, err, err_count, N, L, cyclical, acx_key_words(L)};
    ExpandLaunch f{a, (hipStream_t)stream};
    return dispatch(L, f);
}

int acx_canonicalize(const int32_t* state_in, int32_t* state_out, int32_t* lengths_out, uint8_t* err,
                     int32_t* err_count, int64_t B, int32_t L, int32_t cyclical, void* stream) {
    if (!dims_ok(B, L)) return ACX_E_ARG;
    if (B == 0) return ACX_OK;
    if (!state_in || !state_out || !aligned16(state_in) || !aligned16(state_out)) return ACX_E_ARG;
    CanonArgs a{state_in, state_out, lengths_out, err, err_count, B, L, cyclical};
    CanonLaunch f{a, (hipStream_t)stream};
    return dispatch(L, f);
}

int acx_unpack_keys(const uint64_t* keys, int32_t* states, int32_t* lengths_out, int64_t M, int32_t L,
                    void* stream) {
    if (!dims_ok(M, L)) return ACX_E_ARG;
    if (M == 0) return ACX_OK;
    if (!keys || !states || !aligned16(states)) return ACX_E_ARG;
    UnpackArgs a{keys, states, lengths_out, M, L, acx_key_words(L)};
    UnpackLaunch f{a, (hipStream_t)stream};
    return dispatch(L, f);
}

}  // extern "C"
#endif  // ACX_PART
