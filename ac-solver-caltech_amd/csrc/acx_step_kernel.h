// acx_step_kernel.h -- the step: one wave per tile of 64 envs, one env per lane (step_body), and its
// two kernels (step_kernel, with and without the learner's outputs, and step_lengths_kernel).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "acx.h"
#include "acx_cur_rank.h"
#include "acx_kernel_common.h"
#include "acx_moves.h"
#include "acx_planes.h"
#include "acx_step_args.h"
#include "acx_tile.h"

namespace acx {

// the rows of the tile in the wave-uniform mask `rows` <- src(q, r) (q: the row's ordinal in the
// mask, r: its row in the tile), written to state_out, obs_f32 (as float) and, with to_reset,
// reset_state: the whole wave copies, 16-byte chunks spread over the lanes (a lane copying its
// own row issued 4 x 2L/4 instructions for the wave per finished env)
template <class Src>
__device__ __forceinline__ void copy_rows(const StepArgs& a, const WaveCtx& w, uint64_t rows, int twoL, Src src,
                                          bool to_reset) {
    const int n = __popcll(rows);
    if (n == 0) return;
    const bool full = rows == ~0ull;
    int32_t* st = a.state_out + w.r0 * twoL;
    float* of = a.obs_f32 ? a.obs_f32 + w.r0 * twoL : nullptr;
    int32_t* rs = to_reset ? const_cast<int32_t*>(a.reset_state) + w.r0 * twoL : nullptr;  // learner: writable
    auto row_of = [&](int q) {
        if (full) return q;
        uint64_t m = rows;
        for (int j = 0; j < q; ++j) m &= m - 1;
        return (int)__builtin_ctzll(m);
    };
    if ((twoL & 3) == 0) {
        const int cpr = twoL >> 2;
        for (int i = w.lane; i < n * cpr; i += WAVE) {
            const int q = i / cpr, c = i - q * cpr, r = row_of(q);
            const int4 v = reinterpret_cast<const int4*>(src(q, r))[c];
            reinterpret_cast<int4*>(st + (int64_t)r * twoL)[c] = v;
            if (rs) reinterpret_cast<int4*>(rs + (int64_t)r * twoL)[c] = v;
            if (of) reinterpret_cast<float4*>(of + (int64_t)r * twoL)[c] = make_float4((float)v.x, (float)v.y, (float)v.z,
                                                                                       (float)v.w);
        }
    } else {
        for (int i = w.lane; i < n * twoL; i += WAVE) {
            const int q = i / twoL, c = i - q * twoL, r = row_of(q);
            const int32_t v = src(q, r)[c];
            st[(int64_t)r * twoL + c] = v;
            if (rs) rs[(int64_t)r * twoL + c] = v;
            if (of) of[(int64_t)r * twoL + c] = (float)v;
        }
    }
}

// LEARN: acx_step_learner's extra inputs/outputs (compiled out of the plain acx_step path);
// LIVE: the lengths-carrying step (its own kernel, so the plain step's registers stay its own)
template <int NW, int LC, int VEC, bool LEARN, bool LIVE, int BATCH = 0>
__device__ __forceinline__ void step_body(const StepArgs& a) {
    using Tile = TileFor<NW, LC, VEC>;
        extern __shared__ __attribute__((aligned(16))) char smem[];
    WaveCtx w;
    // acx_learner_step: the curriculum fused in (cur_publish / cur_prefix)
    const bool cur = LEARN && a.cur_ws != nullptr;  // kernel argument: uniform
    if (!wave_ctx(a.B, w)) return;
    // the launch's sequence number, read before this tile publishes (cur_publish)
    const uint32_t cseq = cur ? (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)cur_load(a.cur_ws + cur_layout::SEQ)) : 0u;
    // next_index as this launch found it (the last tile replaces it only after every tile has
    // published, i.e. read it).  exhausted (round 1 complete): no finished env gets a state from
    // the table, so no tile waits for its ranking; the host draws for every finished env.
    // (Leaving a finished env's rows out of the tile's stores when the table surely lasts the
    // launch, so that its copy needs no drain, was slower: the tile's obs store then takes its
    // per-chunk flagged path, 0.164 vs 0.150 ms per steady-state step, r05zg.)
    const int64_t cnext = cur ? (int64_t)__builtin_amdgcn_readfirstlane(
                                    __hip_atomic_load(a.cur_next, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT))
                              : 0;
    const bool exhausted = cur && cnext >= a.n_states;
    // a give-up in an earlier launch (cur_set_failed) left the workspace unusable until the host
    // re-zeroes it: this launch ranks nothing
    const bool broken = cur && __builtin_amdgcn_readfirstlane((int)(uint32_t)cur_load(a.cur_ws + cur_layout::FAILED)) != 0;
    // the table surely lasts the launch (every finished env gets an initial state from it): a
    // finished env is not autoreset here -- its rows are left out of the tile's stores and written
    // once, by the curriculum copy, which then needs no drain of the tile's stores (below)
    const bool sure = cur && !broken && !exhausted && a.n_states - cnext >= a.B;
    Tile tile(smem + w.wid * Tile::wave_bytes(a.L), a.L);
    const int L = tile.Lr(), twoL = 2 * L;
    const int64_t env = w.r0 + w.lane;

    // the env's move id and step count: issued ahead of the tile so their latency hides under it
    int act_in = 0, cnt_in = 0;
    const bool pend = w.active && a.pending && a.pending[env] != 0;  // next-step autoreset: reset now
    if (w.active) {
        if (LEARN && a.action64) {  // policy samples (int64); out of range -> ACX_ERR_ACTION
            const int64_t v = a.action64[env];
            act_in = (v >= 0 && v < 12) ? (int)v : -1;
        } else {
            act_in = a.action[env];
        }
        cnt_in = a.step_count ? a.step_count[env] : 0;
    }
    int hb = 0;  // the move-history ring's row of this env's episode move 0
    if (LEARN && w.active && a.hist_base) hb = a.hist_base[env];
    // Relator skip (acx_step_lengths_reduced): a conjugation (ids 4..11, ac_moves.py:79-156)
    // reads and writes only its target r_i, and simplify_presentation (utils.py:246-283) leaves a
    // reduced r_j as it is -- so when the previous step left both relators reduced (a.reduced) the
    // untouched relator is not read at all; its length comes from the carried lengths.  Not
    // skipped: an r_j of one letter (the triviality test, utils.py:57-87, needs it), a step that
    // truncates (final_obs holds the whole row) and next-step resets.  The lane then holds r_j as
    // empty (n = 0, no live chunks), which the move, the dirty image and the write-back leave alone.
    bool skip = false;
    int skip_h = 0, n_skip = 0;  // the relator left unread and its length
    if constexpr (LIVE) {
        int n_in0 = 0, n_in1 = 0;  // the rows' relator lengths on entry
        if (w.active) {
            n_in0 = a.lengths_out[2 * env];
            n_in1 = a.lengths_out[2 * env + 1];
        }
        if constexpr (Tile::LIVE_ROWS) {
            if (a.reduced && w.active) {
                const uint32_t rf = a.reduced[env];
                skip_h = act_in & 1;  // ids 4..11: the move's target is r_{(id + 1) & 1}
                n_skip = skip_h ? n_in1 : n_in0;
                skip = ((rf >> (a.cyclical ? 1 : 0)) & 1u) != 0u && act_in >= 4 && act_in < 12 && !pend &&
                       n_skip >= 2 && n_skip <= L && !(a.step_count && cnt_in + 1 >= a.horizon);
            }
        }
        tile.set_lim(w.lane, (skip && skip_h == 0) ? 0 : n_in0, (skip && skip_h == 1) ? 0 : n_in1);
        wave_sync();
        tile.template load<true, true, Tile::NT_STEP_LOADS>(a.state_in + w.r0 * twoL, w.R, w.lane);
    } else {
        tile.template load<true, false, Tile::NT_STEP_LOADS, BATCH>(a.state_in + w.r0 * twoL, w.R, w.lane);
    }

    // Truncations are known before the move (step_count + 1 >= horizon, unless the move fails):
    // their starting rows are fetched now, under the pack and the move, and put into the tile
    // before this step's stores -- loaded after the move instead, behind those stores, they were
    // a second dependent round trip that doubled the life of every wave holding one (a learner
    // step with episodes out of phase, ~B/H truncations per step: +44 us on a 124 us step)
    constexpr bool PREF = !LIVE && Tile::PREFETCH_OK;
    uint64_t pre = 0;  // wave-uniform: the rows fetched
    int4 pv = {0, 0, 0, 0};
    if constexpr (PREF) {
        if (a.reset_state && a.step_count && !a.pending) {  // kernel arguments: uniform
            pre = __ballot(w.active && cnt_in + 1 >= a.horizon);
            if (__popcll(pre) > Tile::RPI || sure) pre = 0;  // more (a synchronised truncation): the tile reload below
            if (pre) pv = tile.fetch_rows(a.reset_state + w.r0 * twoL, pre, w.lane);
        }
    }

    bool fin = false;    // done | truncated (the curriculum's "finished")
    bool reset = false;  // same-step autoreset of this env
    bool keep = false;   // the env's row is left as loaded (out of domain, or its move failed)
    constexpr int PW = Tile::PW;
    PlaneRegs<PW> p;
    int cnt0 = 0, cnt = 0, e = ACX_ERR_NONE;
    uint32_t dm = 0;     // relators of the row that differ from state_in (in-place store)
    int act = 0;
    bool triv = false, trunc = false;
    int32_t rwd = 0;
    bool bad = false, clean = false;
    const bool cyc = a.cyclical != 0;
    if (w.active) {
        act = act_in;
        cnt0 = cnt_in;
        cnt = a.step_count ? cnt0 + 1 : 0;
        bad = tile.template pack<LIVE>(w.lane, p);
        clean = !bad && !skip && pl::is_clean<PW>(p.w0, p.n0, p.w1, p.n1, cyc);
    }
    // the curriculum (acx_learner_step, training.py:319-336): every tile publishes its finished
    // count as soon as it is known; the ranking itself waits until the tile's stores are issued
    // (the tail below).  Usually that is before the move: a truncating env finishes unless its move
    // fails, which on a reduced row only an emptying concatenation (n_i == n_j) can; any other env
    // finishes only if the move makes it trivial, which needs the relator it leaves alone at one
    // letter.  A tile with an env outside those cases publishes after the move.
    uint64_t fm = 0;
    bool early = false;  // wave-uniform: published before the move
    uint32_t early_cnt = 0;
    if (cur && !broken) {
        bool unc = false, f0 = false;
        if (w.active && !pend && !bad && act_in >= 0 && act_in < 12) {
            const bool i1 = ((act_in + 1) & 1) != 0;  // the move's target relator (ac_moves.py:192-206)
            const int nt = i1 ? p.n1 : p.n0, nu = i1 ? p.n0 : p.n1;
            const bool tr = a.step_count && cnt0 + 1 >= a.horizon;
            if (!clean) unc = true;  // the general path reduces both relators: anything can happen
            else if (tr) { unc = act_in < 4 && nt == nu; f0 = true; }
            else unc = nu <= 1;
        }
        if (!__any(unc)) {
            early = true;
            early_cnt = (uint32_t)__popcll(__ballot(f0));
            cur_publish_end(a, w, cseq, early_cnt, cur_publish(a, w, cseq, early_cnt, cnext));
        }
    }
    if (w.active) {
        if (pend) e = ACX_ERR_NONE;  // no move: the env resets (gymnasium >= 1.0 NEXT_STEP autoreset)
        else if (bad) e = ACX_ERR_DOMAIN;
        else if (skip) e = pl::ac_move_clean<PW>(p.w0, p.n0, p.w1, p.n1, act, L, cyc);  // reduced: see above
        else if (clean) e = pl::ac_move_clean<PW>(p.w0, p.n0, p.w1, p.n1, act, L, cyc);
        else {
                const pl::MoveOut<PW> mo = pl::ac_move_call<PW>(p, act, L, cyc);
                p = mo.p;
                e = mo.e;
            }
        keep = e != ACX_ERR_NONE;
        if (keep) cnt = cnt0;  // the reference raises before count_steps += 1 (ac_env.py:93-102)
        if (!keep) dm = tile.template unpack_dirty<LIVE>(w.lane, p);
        // (a skipped relator is held as n = 0 in p and has >= 2 letters: never trivial)
        triv = !pend && !keep && pl::is_trivial<PW>(p.w0, p.n0, p.w1, p.n1);
        trunc = !pend && !keep && a.step_count && cnt >= a.horizon;
        // a resetting step (next-step autoreset) returns reward 0, as the vector env's reset does
        rwd = pend ? 0 : triv ? a.horizon * L * 2 : -(p.n0 + p.n1 + n_skip * (int)skip);
        fin = triv || trunc;
        // same-step autoreset: an env that ends resets now; next-step: a pending env resets now and
        // an env that ends is reset by the next call
        reset = a.pending ? pend : (fin && a.reset_state && !keep && !sure);
    }
    if (cur) {
        fm = __ballot(fin);
        const uint32_t cnt = (uint32_t)__popcll(fm);
        if (!broken) {
            if (!early) cur_publish_end(a, w, cseq, cnt, cur_publish(a, w, cseq, cnt, cnext));
            else if (cnt != early_cnt && w.lane == 0) cur_set_failed(a);  // cannot happen: made loud
        }
    }
    if constexpr (PREF) {
        if (pre) tile.put_rows(pv, pre, pre & __ballot(reset), w.lane);
    }
    if (w.active) {
        // info["actions"] (ac_env.py:96,105): the episode's moves, one byte each, move k of env i
        // at row k, or with the ring at row (hist_base[i] + k) mod hist_cap -- envs at the same
        // episode position (ring: every env whose episode had no failed move) write one
        // coalesced row segment (an (env, k) layout made every lane's byte its own cache line:
        // 90 us of a 300 us step; (k, env) with episodes out of phase, 26 us of a 196 us one)
        if (LEARN && a.action_hist && !pend && cnt0 < a.hist_cap) {
            int row = cnt0;
            if (a.hist_base) {
                if (cnt0 == 0) {
                    hb = (int)(a.hist_t % a.hist_cap);
                    a.hist_base[env] = hb;
                }
                row = hb + cnt0 < a.hist_cap ? hb + cnt0 : hb + cnt0 - a.hist_cap;
            }
            a.action_hist[(int64_t)row * a.B + env] = (uint8_t)act;
        }
        if (a.reward) st_scalar<false, int32_t>(a.reward + env, rwd);
        if (a.done) st_scalar<false, uint8_t>(a.done + env, (uint8_t)triv);
        if (a.truncated) st_scalar<false, uint8_t>(a.truncated + env, (uint8_t)trunc);
        if constexpr (LEARN) {
            if (a.reward_f32) a.reward_f32[env] = (float)rwd;
            if (a.done_f32) a.done_f32[env] = triv ? 1.0f : 0.0f;
            if (a.episode_len) a.episode_len[env] = (triv || trunc) ? cnt : 0;
        }
        if (a.pending) a.pending[env] = fin ? 1 : 0;
        // final_obs <- post-move state (per lane: rare, and only with final_obs)
        if (reset && a.final_obs) regs_to_global<PW>(a.final_obs + env * twoL, p, L);
    }
    // out-of-domain rows the load did not flag (a zero inside a relator: CodeTile's slots cannot
    // hold it) are stored from their input row too
    tile.flag_rows(w.lane, (w.active && e == ACX_ERR_DOMAIN) ? FB_IN : 0u);
    const uint64_t rb = __ballot(reset);
    if (rb) {
        // same-step autoreset to the env's starting state.  An out-of-domain starting row is
        // taken as it is, like the reference's reset (ac_env.py:113-129, no validation): the
        // env's row becomes that row's exact values (copied from reset_state, FB_RESET), its
        // step count 0 and its err ACX_ERR_DOMAIN; from then on it is an out-of-domain row.
        bool rbad = false;
        if (__popcll(rb) > RESET_TILE_MIN) {
            // many lanes (a synchronised truncation): one coalesced load of the tile's starting
            // states (per-lane reads of every row cost ~1 ms on a whole-batch truncation step);
            // the other lanes re-stage their state, rows left as loaded copy state_in
            wave_sync();
            tile.load(a.reset_state + w.r0 * twoL, w.R, w.lane);
            if (reset) rbad = tile.pack(w.lane, p);
            wave_sync();
            if (w.active && !keep && !rbad) tile.unpack(w.lane, p);
            dm = (w.active && !keep) ? 3u : 0u;  // the tile now holds starting rows: write every kept-moving row
            tile.restore_flags(w.lane, (w.active && keep) ? FB_IN : (rbad ? FB_RESET : 0u));
        } else {
            // a few lanes: the wave loads just their rows (scattered resets cost their rows only),
            // those it has not fetched before the move
            const uint64_t late = rb & ~pre;
            if (late) tile.load_rows(a.reset_state + w.r0 * twoL, late, w.R, w.lane);
            if (reset) {
                // the tile row already holds the starting row's image (what unpack would write
                // for a row in the domain; a row outside it is stored from its fallback): pack
                // only checks it and sets the lengths
                rbad = tile.pack(w.lane, p);
                dm = 3u;
            }
            tile.flag_rows(w.lane, rbad ? FB_RESET : 0u);
        }
        if (rbad) e = ACX_ERR_DOMAIN;  // lengths_out: the non-zero counts of the starting row
        if (reset) cnt = 0;
    }
    if (sure && fin) {  // the curriculum copy writes the row (no autoreset above: rb has none of them)
        cnt = 0;
        dm = 0u;
    }
    if (w.active) {
        if (a.step_count) st_scalar<false, int32_t>(a.step_count + env, cnt);
        if (a.lengths_out) {
            // lengths-carrying step: an out-of-domain row is read whole on the next call (L, L)
            const bool whole = LIVE && e == ACX_ERR_DOMAIN;
            st_scalar<false, int32_t>(a.lengths_out + 2 * env, whole ? L : (skip && skip_h == 0) ? n_skip : p.n0);
            st_scalar<false, int32_t>(a.lengths_out + 2 * env + 1, whole ? L : (skip && skip_h == 1) ? n_skip : p.n1);
        }
        // a moved row is reduced: freely, and cyclically too when cyclical (simplify_presentation,
        // utils.py:246-283) -- but may hold an empty relator (validity is asserted before the
        // reduction, :264-266: an unreduced y^-1 y empties); a failed, reset or out-of-domain row
        // is read whole next time
        if (LIVE && a.reduced) {
            const bool full = (p.n0 > 0 || (skip && skip_h == 0)) && (p.n1 > 0 || (skip && skip_h == 1));
            st_scalar<false, uint8_t>(
                a.reduced + env,
                (uint8_t)((!keep && !reset && !pend && e == ACX_ERR_NONE && full) ? (a.cyclical ? 3 : 1) : 0));
        }
        if (a.err) st_scalar<false, uint8_t>(a.err + env, (uint8_t)e);
        if (e != ACX_ERR_NONE && a.err_count) atomicAdd(a.err_count, 1);
    }
    if (a.in_place) {
        // state_out == state_in: write only the relators that changed (a gated move, a
        // cyclic conjugation that is a no-op and a failed env leave their row as it is in HBM);
        // lengths-carrying: of those, only the chunks inside the old or the new letters
        tile.set_dirty(w.lane, dm);
        if constexpr (LIVE) tile.widen_lim(w.lane, p.n0, p.n1);
        wave_sync();
        if (__ballot(dm != 0u)) {
            if constexpr (LIVE)
                tile.template store_dirty<NT_WRITEBACK, true>(a.state_out + w.r0 * twoL, w.R, w.lane,
                                                       a.reset_state + w.r0 * twoL);
            else
                tile.template store_dirty<NT_WRITEBACK>(a.state_out + w.r0 * twoL, w.R, w.lane, a.reset_state + w.r0 * twoL);
        }
    } else {
        wave_sync();
        tile.template store<true, NT_STATE>(a.state_out + w.r0 * twoL, twoL, w.R, a.state_in + w.r0 * twoL,
                                                     twoL, w.lane,
                                  a.reset_state + w.r0 * twoL);
    }
    if (LEARN && a.obs_f32)  // the same rows as float32, straight into the learner's buffer
        tile.template store<true, NT_OBS, true>(reinterpret_cast<int32_t*>(a.obs_f32) + w.r0 * twoL, twoL, w.R,
                                               a.state_in + w.r0 * twoL, twoL, w.lane, a.reset_state + w.r0 * twoL,
                                               sure ? fm : 0ull);
    if (cur) {
        // The curriculum's tail (training.py:329-336, 349-352).  A finished env was reset to its own
        // starting row above like any env; now -- every store of the tile issued, so the memory
        // system stays busy while a tile waits -- a tile with finished envs waits for its prefix
        // and each finished env with index k = prefix + (finished envs before it in the tile) <
        // n_states takes initial state k: its state, obs_f32 and reset_state rows are overwritten
        // with that row as it is (acx_curriculum_assign's copy; a row outside the packed domain
        // is then reported with err 3 by the next step) and curr_index = k; past the table's end
        // (round 1 complete) needs_host = 1 and the host draws.  The last tile waits for the total
        // (the new next_index).  The copies are made by the whole wave, 16-byte chunks over the
        // lanes (copy_rows): one lane copying its own row made the steady-state step 0.165 ms
        // instead of 0.150 (r05zg).
        const uint32_t first = broken ? CUR_FAIL : (fm && !exhausted) ? cur_prefix(a, w, cseq, false) : 0u;
        if (!broken && w.r0 + w.R == a.B) {
            const uint32_t tot = cur_prefix(a, w, cseq, true);
            if (w.lane == 0) {
                // every group is complete: no wave of this launch reads next_index or the sequence
                // number again -- advance both for the next one.  A total that never arrived leaves
                // next_index stale: the workspace is marked failed (the host restores both)
                if (tot != CUR_FAIL) {
                    *a.cur_next = (int32_t)((int64_t)tot < a.n_states ? (int64_t)tot : a.n_states);
                    cur_store(a.cur_ws + cur_layout::SEQ, (uint64_t)((cseq + 1u) & CUR_SEQ_MASK));
                } else {
                    cur_set_failed(a);
                }
            }
        }
        const bool failed = first == CUR_FAIL;  // wave-uniform
        if (failed && !broken && w.lane == 0) cur_set_failed(a);
        // finished envs with index k = first + (finished envs before it in the tile) < n_states
        uint64_t take = 0;
        if (fm && !exhausted && !failed) {
            const int64_t nq = a.n_states - (int64_t)first;  // how many of the tile's finished envs get a state
            take = fm;
            while (take && (int64_t)__popcll(take) > nq) take &= ~(1ull << (63 - __builtin_clzll(take)));
        }
        if (take) {
            // the rows were autoreset above (a failed ranking leaves them so): the tile's own
            // stores of them complete first -- unless `sure`: the tile left them out
            if (!sure) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            copy_rows(a, w, take, twoL, [&](int q, int) { return a.cur_states + ((int64_t)first + q) * twoL; }, true);
        }
        // `sure` and a finished env without a state (a failed ranking): its own starting row, as the
        // autoreset would have left it
        const uint64_t own = sure ? (fm & ~take) : 0ull;
        if (own) copy_rows(a, w, own, twoL, [&](int, int r) { return a.reset_state + (w.r0 + r) * twoL; }, false);
        if (w.active) {
            uint8_t nh = 0;
            if (fin) {
                if (failed) nh = 3;
                else if ((take >> w.lane) & 1ull) a.curr_index[env] = (int32_t)((int64_t)first + __popcll(fm & ((1ull << w.lane) - 1ull)));
                else nh = 1;
            }
            a.needs_host[env] = nh;
        }
    }
}

template <int NW, int LC, int VEC, bool LEARN>
__global__ __launch_bounds__(BLOCK, Occupancy<LC>::waves_per_simd) void step_kernel(StepArgs a) {
    step_body<NW, LC, VEC, LEARN, false>(a);
}

// acx_step_lengths (in place, lengths in and out).  At L = 128 the tile's LDS allows 4 waves per
// SIMD; the live-chunk predicates took the register count just past 128 VGPRs (3 waves), so
// the allocator is held to 4
template <int NW, int LC, int VEC>
__global__ __launch_bounds__(BLOCK, LC == 128 ? 4 : Occupancy<LC>::waves_per_simd) void step_lengths_kernel(StepArgs a) {
    step_body<NW, LC, VEC, false, true>(a);
}

}  // namespace acx
