// acx_mcts.hip -- MCTS over a batch of presentations, scored by the caller: one wave (64 threads)
// owns one search, and a step of all searches is two launches (select, backup) with the caller's
// scorer between them.  The searches are independent, so no workgroup ever waits on another.  It is
// the third engine of the scored-step frame (acx_scored.h): where acx_vgreedy.hip has a heap, this
// one has a tree with visit statistics, UCB1 selection and a backup.
//
// Reference: value_search/mcts.py:177-314 (mcts_search) with time_limit=None; the solution cache
// is the second instantiation of the begin and select kernels (begin_body / select_body below).  The root is node 0 with visit = 1; its own value is never read, so it is not
// scored.  At the top of every iteration: len(visited) < budget and iterations < 50 * budget
// (:244), so a budget of 0 or 1 runs no iteration, and an iteration overshoots the budget by up to
// 11 nodes.  An iteration:
//   select (:68-73, :46-65)  from the root, while the node has children: a child with visit == 0
//     of least prior if there is one (the first in action order on ties), otherwise the child of
//     greatest -(vsum / visit) + c * sqrt(log(N) / visit), N the node's visit count, by a strict >
//     (the first in action order on ties).  A node's children are the rows one expansion appended:
//     child0 .. child0 + nch;
//   a terminal leaf (:252) ends the search, found: only the root can be one (an empty path);
//   expand (:76-109)  all 12 children are made first: any raising move ends the search
//     (ACX_BFS_MOVE_ERROR), even behind a trivial child (unlike acx_vgreedy.hip).  Every new state
//     enters the visited set and the store in action order -- the reference dedups incrementally,
//     so a twin of an earlier child of the same expansion is dropped there too -- and
//     nodes_explored counts them all, the trivial one and those after it included;
//   the first trivial new child (:267-270) ends the search, found; it is a stored node, and its
//     path the plain walk [(action, total), ...] with no root entry;
//   no new child (:259-263): prior(leaf) + 50.0 is backed up from the leaf to the root -- visit += 1,
//     vsum += value at every node of the descent -- and the next iteration follows unscored;
//   otherwise the new children are the step's candidates: their priors are max(v, 0) (:154), and
//     the least of them is backed up the same way (:297-298); the children keep visit = 0.
// The loop ending on its first test is ACX_BFS_BUDGET, on its second -- a search whose reachable
// leaves are all dead ends spins until iterations == 50 * budget -- ACX_BFS_EXHAUSTED.  Every
// unsolved ending returns (False, []).
//
// The reference's statistics are Python doubles, and near-ties between UCB scores are common, so
// the decisions here are bit-identical and not merely close: vsum is a double, visit a uint32, a
// prior the scorer's float32 widened; the score (ucb, below) is fp64 in the reference's operation
// order with contraction off (the default would fuse c * sqrt(..) + e into one v_fma_f64; fp64
// division and sqrt are IEEE-rounded sequences on gfx950); log(N) is read from the caller's table
// of the host libm's values -- a device log's last bit is not the host's.
//
// A search's memory is a private slice of each of the handle's arrays, R = B + 11 rows
// (B = max_nodes_each; the overshoot), and persists between launches:
//   store  (R, kw) uint64   node keys in append order (node 0 is the root).  An iteration's
//                           candidates are its new nodes, rows cand_base .. cand_base + cand_n;
//   meta   (R) uint32       parent index << 4 | action (the path reader walks it);
//   depth  (R) uint32       path length of each node;
//   rec    (R) 24 bytes     vsum double, visit uint32, prior float, child0 uint32, nch uint32;
//   trail  (R) uint32       the node ids of the current descent, root first;
//   table  (nb * 8) uint64  the visited set (acx_visited.h), nb = ceil((R + 12) / 4) buckets;
//   state, res, the five results, the iteration's candidate count and its offset (140 bytes).
// Bytes per search (acx_mcts_bytes):
//   (8 kw + 36) (B + 11) + 64 ceil((B + 23) / 4) + 140,   kw = acx_key_words(L).
//
// mcts_select_kernel<NW>: iterations until the search has candidates to score, has ended, or has
//   spent ACX_MCTS_SPIN = 64 iterations on dead ends (the bound of a launch: a spinning search
//   takes about 50 B / 64 launches).  A level of the descent is one load per lane a < nch of child
//   a's record; the winner's child0, nch and visit are broadcast from its lane, so a level is one
//   dependent global load.  Then expand and append (acx_pop.h) with the visited insert between.
// The offsets and the gather are the step frame's (acx_scored.h).
// mcts_backup_kernel: the candidates' scores; a NaN or +inf ends the search (ACX_BEAM_NAN); the
//   priors are stored, and the least is backed up along the trail.  A search whose candidates do not
//   fit the caller's M ends with ACX_MBFS_OVERFLOW.
// Both backups update the trail's nodes in parallel: each node gets exactly one add, so the sums
// are the reference's.
// Every loop is bounded: iterations of a launch by ACX_MCTS_SPIN, the descent by the rows (a node's
// depth), probes by nb, the path walk by the node's depth.
//
// The store, the records and the table are shared by the lanes across phases: table reads are
// workgroup-scope atomic loads and the rewrite an atomic store (acx_batch.h); everything else is
// plain loads and stores ordered by the barriers and the launch boundaries.
//
// Registers and LDS (tools/kernel_resources.py; every figure: profiles/mcts/kernel_resources.md):
//   mcts_select_kernel<1 / 2 / 3 / 4 / 8>   60 / 62 / 65 / 68 / 87 VGPRs, 288 / 384 / 480 / 576 / 960 B of
//       LDS: 8 / 8 / 7 / 7 / 5 waves per SIMD (<2> also has 24 B of private memory per lane, as
//       vgreedy_pop_kernel<2>); 106 SGPRs with 128 / 139 / 113 / 134 / 172 SGPR spills, kept in VGPR
//       lanes (no scratch for them);
//   mcts_backup_kernel 14 VGPRs, no LDS; mcts_begin_kernel 11 VGPRs, 96 B; the frame's offsets,
//   gather and results kernels 53 (64 B of LDS), 8 and 13 VGPRs, as in acx_vgreedy.hip.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "acx.h"
#include "acx_moves.h"

#include "acx_batch.h"
#include "acx_beam_key.h"
#include "acx_bfs_common.h"
#include "acx_cache.h"
#include "acx_pop.h"
#include "acx_scored.h"
#include "acx_visited.h"

namespace acx {
namespace mcts {

using namespace acx::bfs;
using namespace acx::pop;
using batch::Buckets;
using scored::ended;

constexpr int SPIN = ACX_MCTS_SPIN;

struct Rec {
    double vsum;
    uint32_t visit;
    float prior;
    uint32_t child0, nch;
};
static_assert(sizeof(Rec) == 24, "the bytes formula of include/acx.h");

struct State : scored::State {
    int32_t tl;  // nodes of the trail: the descent of the iteration whose candidates are out
    uint32_t leaf;
};

struct Args : batch::Args {
    Rec* rec;
    uint32_t* trail;
    State* state;
    int32_t* counts;   // (n) the iteration's candidates per search
    int64_t* offsets;  // (n + 1) their exclusive prefix sum
    int64_t n;         // searches of the running call
};

// The UCB1 score of a child (mcts.py:57-61) in the reference's operation order, every operation
// rounded on its own.
__device__ __forceinline__ double ucb(double vsum, uint32_t visit, double logN, double c) {
#pragma clang fp contract(off)
    const double nv = (double)visit;
    const double mean = vsum / nv;
    const double exploitation = -mean;
    const double exploration = c * sqrt(logN / nv);
    return exploitation + exploration;
}

// the value a dead end backs up (mcts.py:262)
__device__ __forceinline__ double dead_end_value(float prior) {
#pragma clang fp contract(off)
    return (double)prior + 50.0;
}

__device__ __forceinline__ uint32_t bcast(uint32_t v, uint32_t lane) {
    return (uint32_t)__builtin_amdgcn_readlane((int)v, (int)lane);
}
__device__ __forceinline__ double bcast(double v, uint32_t lane) {
    return __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(v), (int)lane),
                            __builtin_amdgcn_readlane(__double2loint(v), (int)lane));
}

// visit += 1, vsum += value at every node of the trail: one add per node
__device__ __forceinline__ void back_up(Rec* rec, const uint32_t* trail, int tl, int64_t rows, double value, int lane) {
    for (int t = lane; t < tl; t += GT) {
        const uint32_t v = trail[t];
        if (v >= (uint64_t)rows) continue;  // (never: the trail names appended nodes)
        rec[v].visit += 1;
        rec[v].vsum += value;
    }
}

// The begin and select kernels' bodies, with the solution cache's probe compiled in or not (CACHE;
// acx_cache.h): the kernels below are their two instantiations each.  With a cache
// (mcts.py:224-229, 265-289) the root is probed before the first iteration, and after an expansion
// its new children -- not the ones already visited -- are looked at in action order, the terminal
// test first, then the cache; nodes_explored counts all of the expansion's new children.
template <int NW, bool CACHE>
__device__ __forceinline__ void begin_body(const Args& a, const cache::Attach& at) {
    const int64_t q = blockIdx.x;
    uint64_t* store = a.store + q * a.rows * a.kw;
    uint32_t* meta = a.meta + q * a.rows;
    uint64_t* table = a.table + q * (int64_t)a.nb * BUCKET;
    const batch::Root root = batch::root_setup<GT, NW>(a, q, store, meta, table);
    cache::Hit hit{cache::MISS, 0, 0};
    if constexpr (CACHE) {
        if (!root.refused) hit = cache::probe<NW + 1>(at.view, root.key, a.kw, a.L, threadIdx.x);
    }
    if (threadIdx.x != 0) return;
    // (a search's results are written where it ends)
    if (!root.refused) batch::write_result(a, q, Res{ACX_MBFS_OVERFLOW, 0, 0, 0, 0, 0}, 0, 0, 0);
    a.state[q] = State{{1, root.max_nodes, 0, 1, root.refused, 0, root.total0, 0}, 0, 0};
    (a.depth + q * a.rows)[0] = 0;
    (a.rec + q * a.rows)[0] = Rec{0.0, 1u, 0.0f, 0u, 0u};  // visit = 1 (mcts.py:234); the value is never read
    a.counts[q] = 0;
    if constexpr (CACHE) {
        at.hit[q] = hit;
        if (hit.entry != cache::MISS) cache::ended_cached(a, q, a.state + q, at, hit, 0, 0, root.total0, 1, 0, 0);
    }
}

template <int NW, class... At>
__global__ __launch_bounds__(GT) void mcts_begin_kernel(Args a, At... at) {
    begin_body<NW, sizeof...(At) != 0>(a, cache::attach_of(at...));
}

template <int NW, bool CACHE>
__device__ __forceinline__ void select_body(const Args& a, const double* log_table, int64_t n_log, double c,
                                            const cache::Attach& at) {
    __shared__ uint64_t ck[12 * (NW + 1)];  // the expansion's child keys, kw words each
    __shared__ uint32_t slot[12];           // table index of the entry a child holds
    __shared__ uint32_t lost[12];           // an earlier child of the expansion took that entry

    const int lane = threadIdx.x;
    const int64_t q = blockIdx.x;
    const int L = a.L, kw = a.kw;
    const bool cyc = a.cyc != 0;
    State* S = a.state + q;
    if (S->done) return;  // (its count is 0 since it ended)
    uint64_t* store = a.store + q * a.rows * kw;
    uint32_t* meta = a.meta + q * a.rows;
    uint32_t* depth = a.depth + q * a.rows;
    Rec* rec = a.rec + q * a.rows;
    uint32_t* trail = a.trail + q * a.rows;
    uint64_t* table = a.table + q * (int64_t)a.nb * BUCKET;

    int64_t n_nodes = S->n_nodes, iters = S->steps;
    const int64_t max_nodes = S->max_nodes;
    const uint32_t running = S->running;  // the root's total: min_length is not the reference's to report
    const int32_t pending = S->cand_n;
    __syncthreads();  // the state is read before lane 0 rewrites it
    if (pending != 0 || n_nodes < 1 || n_nodes > a.rows) {  // (never: a backup takes the candidates)
        if (lane == 0) ended(a, q, S, ACX_MBFS_OVERFLOW, 0, 0, n_nodes, iters, running, 0);
        return;
    }

    for (int spin = 0; spin < SPIN; ++spin) {
        // the loop test (mcts.py:244)
        if (n_nodes >= max_nodes || iters >= 50 * max_nodes) {
            if (lane == 0)
                ended(a, q, S, n_nodes >= max_nodes ? ACX_BFS_BUDGET : ACX_BFS_EXHAUSTED, 0, 0, n_nodes, iters, running, 0);
            return;
        }
        ++iters;

        // select: the descent, one record load per level
        uint32_t node = 0, c0, nc, N;
        {
            const Rec r0 = rec[0];
            c0 = r0.child0, nc = r0.nch, N = r0.visit;
        }
        int tl = 0;
        int32_t bad = 0;
        for (;;) {
            if (lane == 0) trail[tl] = node;
            ++tl;
            if (nc == 0) break;
            if (tl >= a.rows || nc > 12u || (uint64_t)c0 + nc > (uint64_t)n_nodes || c0 == 0) {  // (never)
                bad = ACX_MBFS_OVERFLOW;
                break;
            }
            const bool has = (uint32_t)lane < nc;
            Rec r = Rec{0.0, 1u, 0.0f, 0u, 0u};
            if (has) r = rec[c0 + lane];
            const uint32_t unvisited = (uint32_t)__ballot(has && r.visit == 0);
            int w = -1;
            if (unvisited) {  // the unvisited child of least prior, the first on ties (:50-52)
                float best = 0.0f;
#pragma unroll
                for (int k = 0; k < 12; ++k) {
                    if (!((unvisited >> k) & 1u)) continue;
                    const float p = __uint_as_float(bcast(__float_as_uint(r.prior), k));
                    if (w < 0 || p < best) best = p, w = k;
                }
            } else {  // the greatest UCB1 score by a strict > (:54-65)
                if ((int64_t)N >= n_log) {  // the caller's table is too short for this search
                    bad = ACX_MBFS_OVERFLOW;
                    break;
                }
                const double score = ucb(r.vsum, r.visit, log_table[N], c);
                double best = -__builtin_huge_val();
#pragma unroll
                for (int k = 0; k < 12; ++k) {
                    if ((uint32_t)k >= nc) continue;
                    const double s = bcast(score, k);
                    if (s > best) best = s, w = k;
                }
                if (w < 0) {  // no score above -inf: the reference's best_child_ucb returns None
                    bad = ACX_MBFS_OVERFLOW;
                    break;
                }
            }
            const uint32_t wl = (uint32_t)__builtin_amdgcn_readfirstlane(w);
            node = c0 + wl;
            N = bcast(r.visit, wl);
            nc = bcast(r.nch, wl);
            c0 = bcast(r.child0, wl);
        }
        if (bad) {
            if (lane == 0) ended(a, q, S, bad, 0, 0, n_nodes, iters, running, 0);
            return;
        }
        const uint32_t leaf = node;
        const uint32_t dpar = depth[leaf];
        if (leaf == 0 && running == 2u) {  // a terminal leaf (:252): the root, and the path is empty
            if (lane == 0) {
                ended(a, q, S, ACX_BFS_FOUND, 0, 0, n_nodes, iters, running, 0);
                a.res[q].status = ACX_BFS_BUDGET;  // (for the path reader: nothing to write)
            }
            return;
        }

        // expand: all 12 children, then the verdicts
        const Children ch = expand<NW>(store, leaf, ck, lost, lane, L, kw, cyc, [](uint32_t) {});
        __syncthreads();
        if (ch.first_err != NONE) {
            if (lane == 0) ended(a, q, S, ACX_BFS_MOVE_ERROR, 0, 0, n_nodes, iters, running, 0);
            return;
        }

        // insert
        const uint64_t NB = (uint64_t)n_nodes;
        visited::Outcome ins = visited::SEEN;
        if (lane < 12) {
            const uint64_t code = NB + (uint64_t)lane;
            const Key<NW + 1> key = kload<NW + 1>(ck + lane * kw, kw);
            ins = visited::insert(
                Buckets{table, a.nb}, a.ep, code, khash<NW + 1>(key, kw),
                [&](uint64_t vc) {
                    return vc < NB ? keq<NW + 1>(store + vc * kw, key, kw)
                                   : (vc - NB < 12u && keq<NW + 1>(ck + (vc - NB) * kw, key, kw));
                },
                [&](uint32_t sl, uint64_t displaced) {  // a later child of the expansion that held it learns it lost
                    slot[lane] = sl;
                    const uint64_t lc = displaced - NB;
                    if (displaced != visited::NO_CODE && lc < 12u) lost[lc] = 1;
                });
        }
        __syncthreads();
        if (__ballot(ins == visited::FULL)) {  // (uniform) cannot happen at load <= 1/2
            if (lane == 0) ended(a, q, S, ACX_MBFS_OVERFLOW, 0, 0, n_nodes, iters, running, 0);
            return;
        }

        // append the survivors in action order: the leaf's children
        const bool alive = lane < 12 && ins == visited::HELD && !lost[lane];
        const Survivors sv = survivors(alive, lane);
        append(alive, sv.rank, lane, leaf, dpar, n_nodes, a.rows, kw, ck, slot, store, meta, depth, table,
               [&](int64_t pos) { rec[pos] = Rec{0.0, 0u, 0.0f, 0u, 0u}; });
        const uint32_t cnt = sv.cnt;
        const int64_t base = n_nodes;
        n_nodes += cnt;
        const uint32_t trivial = (uint32_t)__ballot(alive && ch.tot == 2u);
        if constexpr (CACHE) {  // the new children below the first trivial one, in action order
            const uint32_t upto = trivial ? (uint32_t)__builtin_ctz(trivial) : 12u;
            for (uint32_t cc = 0; cc < upto; ++cc) {
                if (!((sv.m >> cc) & 1u)) continue;
                const cache::Hit hit = cache::probe<NW + 1>(at.view, ck + cc * kw, kw, L, lane);
                if (hit.entry == cache::MISS) continue;
                if (lane == 0)
                    cache::ended_cached(a, q, S, at, hit, (int32_t)cc, leaf, (uint32_t)key_total(ck + cc * kw, L), n_nodes,
                                        iters, (int64_t)dpar + 1);
                return;
            }
        }
        if (trivial) {  // the first trivial new child (:267-270)
            if (lane == 0)
                ended(a, q, S, ACX_BFS_FOUND, __builtin_ctz(trivial), leaf, n_nodes, iters, running, (int64_t)dpar + 1);
            return;
        }
        if (cnt != 0) {  // the candidates of this step; the backup follows their scores
            if (lane == 0) {
                rec[leaf].child0 = (uint32_t)base;
                rec[leaf].nch = cnt;
                S->n_nodes = n_nodes;
                S->steps = iters;
                S->cand_base = base;
                S->cand_n = (int32_t)cnt;
                S->tl = tl;
                S->leaf = leaf;
                a.counts[q] = (int32_t)cnt;
            }
            return;
        }

        // a dead end (:259-263)
        const double value = dead_end_value(rec[leaf].prior);
        __syncthreads();  // the leaf's prior is read before its record is rewritten
        back_up(rec, trail, tl, a.rows, value, lane);
        __syncthreads();  // the next descent reads the records
    }
    if (lane == 0) {  // the launch's bound: the search goes on with the next one
        S->steps = iters;
        a.counts[q] = 0;
    }
}

template <int NW, class... At>
__global__ __launch_bounds__(GT) void mcts_select_kernel(Args a, const double* log_table, int64_t n_log, double c,
                                                         At... at) {
    select_body<NW, sizeof...(At) != 0>(a, log_table, n_log, c, cache::attach_of(at...));
}

__global__ __launch_bounds__(GT) void mcts_backup_kernel(Args a, const float* scores, int64_t M) {
    const int lane = threadIdx.x;
    const int64_t q = blockIdx.x;
    State* S = a.state + q;
    if (S->done) return;
    const int n = a.counts[q];  // 0 for a launch of dead ends
    const int64_t off = a.offsets[q];
    const int64_t base = S->cand_base, n_nodes = S->n_nodes;
    const int tl = S->tl;
    if (n == 0) return;
    const int64_t iters = S->steps;
    const uint32_t running = S->running;
    __syncthreads();  // the state is read before lane 0 rewrites it
    // a count, an offset or an M that does not fit the iteration (a caller's M that is not the one
    // acx_mcts_select wrote): the priors cannot be stored, so the search ends and says so, with
    // all-zero outputs as a refused search has
    if (n < 0 || n > 12 || off < 0 || off + n > M || base < 1 || base + n > a.rows || tl < 1 || tl > a.rows) {
        if (lane == 0) ended(a, q, S, ACX_MBFS_OVERFLOW, 0, 0, n_nodes, 0, 0, 0);
        return;
    }
    Rec* rec = a.rec + q * a.rows;
    const uint32_t* trail = a.trail + q * a.rows;

    const bool alive = lane < n;
    const float v = alive ? scores[off + lane] : 0.0f;
    const uint32_t bits = __float_as_uint(v);
    const bool refused = __ballot(alive && (beam::score_is_nan(bits) || bits == 0x7f800000u)) != 0;
    if (refused) {  // (uniform) a NaN, or +inf: the reference's selection would find no child
        if (lane == 0) ended(a, q, S, ACX_BEAM_NAN, 0, 0, n_nodes, iters, running, 0);
        return;
    }
    const float prior = v < 0.0f ? 0.0f : v;  // max(v, 0) (:154)
    if (alive) rec[base + lane].prior = prior;
    float least = 0.0f;  // min(new_children, key=prior_value) (:297)
#pragma unroll
    for (int k = 0; k < 12; ++k) {
        if (k >= n) continue;
        const float p = __uint_as_float(mcts::bcast(__float_as_uint(prior), k));
        if (k == 0 || p < least) least = p;
    }
    back_up(rec, trail, tl, a.rows, (double)least, lane);
    if (lane == 0) {
        S->cand_n = 0;
        a.counts[q] = 0;
    }
}

__global__ __launch_bounds__(TPB) void ucb_kernel(const double* vsum, const uint32_t* visit, const double* logN, double c,
                                                  double* out, int64_t n) {
    const int64_t i = (int64_t)blockIdx.x * TPB + threadIdx.x;
    if (i < n) out[i] = ucb(vsum[i], visit[i], logN[i], c);
}

// what the handle (acx_batch.h) and the step frame (acx_scored.h) need of this engine
struct Engine {
    using Args = mcts::Args;
    // a found search's path (mcts.py:166-174): the edges to the trivial child, no root entry
    // a search that ended on a cache hit below the root: the edges to the child that hit
    static constexpr uint32_t WITH_PATH = 1u << ACX_BFS_FOUND | 1u << ACX_BFS_CACHED;
    static constexpr bool ROOT_ENTRY = false;
    static constexpr int GATHER_THREADS = GT, MOST = 12;
    static constexpr bool LIVE = true;
    static int64_t rows_for(int64_t B) { return pop::rows_for(B); }
    static uint32_t buckets_for(int64_t B) { return pop::buckets_for(B); }
    template <class F>
    static void arrays(Args& a, F f) {
        pop::arrays(a, f, a.rec, sizeof(Rec), a.trail, 4);
        scored::arrays(a, f);
    }
};
static_assert(sizeof(State) == 56 && scored::RECORD<State> == 140, "the bytes formula of include/acx.h");

}  // namespace mcts
}  // namespace acx

namespace mcts = acx::mcts;
namespace batch = acx::batch;
namespace scored = acx::scored;
using mcts::Engine;

extern "C" {

int64_t acx_mcts_bytes(int32_t L, int64_t max_nodes_each) { return batch::bytes<Engine>(L, max_nodes_each); }

void* acx_mcts_create(int32_t L, int64_t n_searches, int64_t max_nodes_each, int32_t cyclical) {
    return batch::create<Engine>(L, n_searches, max_nodes_each, cyclical);
}

void acx_mcts_destroy(void* h) { batch::destroy<Engine>(h); }

int acx_mcts_begin(void* h, const int32_t* states, const int64_t* budgets, int64_t n, void* stream) {
    return scored::begin<Engine>(h, states, budgets, true, n, stream, [=](auto nw, const mcts::Args& a, auto... at) {
        mcts::mcts_begin_kernel<decltype(nw)::value>
            <<<dim3((unsigned)a.n), dim3(mcts::GT), 0, (hipStream_t)stream>>>(a, at...);
    });
}

int acx_mcts_set_cache(void* h, void* cache) { return acx::cache::set_cache<batch::Handle<Engine>>(h, cache); }

int acx_mcts_cache_hits(void* h, int64_t n, int64_t* entry, int32_t* rel, int32_t* k, void* stream) {
    return acx::cache::read_hits<batch::Handle<Engine>>(h, n, entry, rel, k, stream);
}

int acx_mcts_select(void* h, const double* log_table, int64_t n_log, double c_explore, int64_t* pair, void* stream) {
    if (!log_table || n_log < 2 || c_explore != c_explore) return ACX_E_ARG;
    return scored::make<Engine>(h, pair, stream, [=](auto nw, const mcts::Args& a, auto... at) {
        mcts::mcts_select_kernel<decltype(nw)::value>
            <<<dim3((unsigned)a.n), dim3(mcts::GT), 0, (hipStream_t)stream>>>(a, log_table, n_log, c_explore, at...);
    });
}

int acx_mcts_gather(void* h, uint64_t* keys, int64_t M, void* stream) {
    return scored::gather<Engine>(h, keys, M, stream);
}

int acx_mcts_backup(void* h, const float* scores, int64_t M, void* stream) {
    return scored::take<Engine>(h, scores, M, stream, [=](const mcts::Args& a, hipStream_t st) {
        mcts::mcts_backup_kernel<<<dim3((unsigned)a.n), dim3(mcts::GT), 0, st>>>(a, scores, M);
    });
}

int acx_mcts_finish(void* h, int32_t* status, int64_t* nodes, int64_t* iterations, int32_t* min_length,
                    int64_t* path_len, void* stream) {
    return scored::finish<Engine>(h, status, nodes, iterations, min_length, path_len, stream);
}

int acx_mcts_paths(void* h, int64_t n, const int64_t* offsets, int32_t* actions, int32_t* totals, int64_t cap,
                   void* stream) {
    return batch::paths<Engine>(h, n, offsets, actions, totals, cap, stream);
}

int acx_internal_ucb(const double* sum, const uint32_t* visit, const double* logN, double c, double* out, int64_t n,
                     void* stream) {
    if (n < 0 || (n > 0 && (!sum || !visit || !logN || !out))) return ACX_E_ARG;
    if (n == 0) return ACX_OK;
    mcts::ucb_kernel<<<dim3((unsigned)((n + acx::bfs::TPB - 1) / acx::bfs::TPB)), dim3(acx::bfs::TPB), 0,
                       (hipStream_t)stream>>>(sum, visit, logN, c, out, n);
    return hipGetLastError() == hipSuccess ? ACX_OK : ACX_E_LAUNCH;
}

}  // extern "C"
