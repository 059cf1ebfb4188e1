// acx_vgreedy.hip -- value-guided greedy search over a batch of presentations, scored by the
// caller: one wave (64 threads) owns one search, and a step of all searches is two launches (pop,
// push) with the caller's scorer between them.  The searches are independent, so no workgroup ever
// waits on another.  It is the heap of acx_mgreedy.hip whose keys arrive from the caller's model one
// launch after the nodes they belong to.
//
// Reference: value_search/value_guided_search.py:294-414 (value_guided_greedy_search) with
// time_limit=None; the solution cache is the second instantiation of the begin and pop kernels
// (acx_cache.h; below, "with a cache").  The root is node 0 and the only heap entry; its score
// never decides anything, so it is not scored.  While the heap is not empty the least (score,
// path_length, node_id) is popped -- node ids are unique, so the order is total and no state is
// ever compared (unlike acx_prio.h) -- and its 12 children are taken in action order; per child: a
// raising move ends the search (ACX_BFS_MOVE_ERROR); min_length takes the child's total, duplicates
// and children of refused moves included (:358-359); a total of 2 ends the search, found, before the
// visited test (:364-369), with nodes_explored the number of distinct states before this pop's
// children (they are registered after the loop, :398-402); a child not in the visited set is a
// candidate (:382-383).  The candidates are scored together and pushed with depth + 1 (:386-406);
// only then comes the budget test len(state_to_id) >= max_nodes, once per pop (:408-411), so a pop
// overshoots the budget by up to 11 nodes and a budget of 1 still runs one pop.  The heap emptying
// is ACX_BFS_EXHAUSTED.  Every unsolved ending returns (False, []): no path, unlike greedy.py:121.
//
// Two actions of one pop that yield the same new state: the reference tests against state_to_id as
// it stood before the pop, so it gives both a node id and pushes both; only len(state_to_id) counts
// them once.  The later twin has the same score and depth and a larger id, so it pops after the
// first, when each of its children is visited, and had one been trivial or the budget reached the
// search would have ended at the first twin's pop: its pop changes nothing observable (paths hold
// actions and totals, never ids).  This engine keeps the first and drops the later ones (`lost`, as
// acx_mgreedy.hip), so n_nodes is len(state_to_id).  That holds wherever the scorer gives equal rows
// equal scores; tests/test_vgreedy_cpu.py compares the two variants.
//
// A search's memory is a private slice of each of the handle's arrays, R = B + 11 rows
// (B = max_nodes_each; the overshoot), and persists between launches:
//   store  (R, kw) uint64   node keys in append order (node 0 is the root).  A pop's candidates are
//                           its new nodes, rows cand_base .. cand_base + cand_n, so the gather
//                           copies them from here;
//   meta   (R) uint32       parent index << 4 | action (the path reader walks it);
//   depth  (R) uint32       path length of each node;
//   hk     (R) uint64       the frontier, an implicit min-heap of fan-out 64 (acx_heap.h):
//   hid    (R) uint32       hk = score_key(score bits) << 32 | depth (acx_beam_key.h: the floats'
//                           order, -0.0 ties with +0.0), hid = the node's index, which decides
//                           ties on hk;
//   table  (nb * 8) uint64  the visited set (acx_visited.h), nb = ceil((R + 12) / 4) buckets;
//   state, res, the five results, the pop's candidate count and its offset (140 bytes).
// Bytes per search (acx_vgreedy_bytes):
//   (8 kw + 20) (B + 11) + 64 ceil((B + 23) / 4) + 140,   kw = acx_key_words(L).
//
// vgreedy_pop_kernel<NW>: take (acx_heap.h); expand (acx_pop.h) -- lane a < 12 makes child a;
//   insert -- visited::insert with the pop's round code n_nodes + a; append (acx_pop.h) -- the
//   survivors go to rows n_nodes.. in action order and are the step's candidates.  A pop without a
//   survivor is decided here: the budget verdict, then the empty heap.
// The offsets and the gather are the step frame's (acx_scored.h, shared with acx_beam.hip): the host
//   reads M (rows to score) and live (searches not ended).  M == 0 with live > 0 is legal: a pop
//   whose children were all known.
// vgreedy_push_kernel: the candidates' scores; a NaN ends the search (ACX_BEAM_NAN, the beam's
//   value, shared); then the budget verdict; otherwise the new leaves' heap words are written at
//   the heap's end and pushed (acx_heap.h).  A search whose candidates do not fit the caller's M
//   ends with ACX_MBFS_OVERFLOW instead of staying live without them.
// Every loop is bounded: pops by the rows (each pop removes one of at most R appended nodes), sifts
// by the heap height, probes by nb, the path walk by the node's depth.
//
// The heap, the store and the table are shared by the lanes across phases: table reads are
// workgroup-scope atomic loads and the rewrite an atomic store (acx_batch.h); everything else is
// plain loads and stores ordered by the barriers and the launch boundaries.
//
// Registers and LDS (tools/kernel_resources.py; every figure: profiles/heap_shared/kernel_resources.md):
//   vgreedy_pop_kernel<1 / 2 / 3 / 4 / 8>   41 / 43 / 45 / 47 / 59 VGPRs, 288 / 384 / 480 / 576 / 960 B of
//       LDS: 8 waves per SIMD (<2> also has 24 B of private memory per lane, as mgreedy_kernel<2>);
//       106 SGPRs with 92 / 96 / 117 / 162 / 119 SGPR spills, kept in VGPR lanes (no scratch for them);
//   vgreedy_push_kernel 26 VGPRs, no LDS; vgreedy_begin_kernel 11 VGPRs, 96 B; the frame's offsets,
//   gather and results kernels 53 (64 B of LDS), 8 and 13 VGPRs.
//
// With a cache (acx_vgreedy_set_cache; value_guided_search.py:326-330, 372-380): the root is probed
// in the begin kernel (a hit: nodes 1, min_length 2, no pop), and a pop probes its children in
// action order below the first raising or trivial one -- the reference tests a child's triviality,
// then the cache, then the visited set -- one wave-wide probe per child.  A hit ends the search with
// ACX_BFS_CACHED, the nodes of a found search and min_length 2; the path reader returns the path to
// the popped node plus the child's (action, total), and the hit record (entry, rel, k) goes to the
// attachment's array, not to the search's slice.  vgreedy_pop_kernel<1 / 2 / 3 / 4 / 8, cache::Attach>:
// 53 / 55 / 57 / 59 / 68 VGPRs, the same LDS (profiles/cache/kernel_resources.md, where its
// name has _cached before _kernel).
//
// Fused with the FeatureMLP scorer (acx_vgreedy_run_mlp; acx_mlp.h, acx_feat.h): the pop and push
// kernels' bodies are device functions, and vgreedy_fused_kernel<NW> / vgreedy_fused_kernel<NW, cache::Attach>
// loop them in one launch, up to max_pops times per search, with the scorer between them on the
// device: 4 candidates at a time, lane c computes candidate c's 14 features from its store row
// (acx_features' arithmetic, normalisation included) into LDS, the wave runs the layers, and lane c
// keeps y; the push reads the pop's scores from LDS.  Nothing returns to the host between pops; lane 0
// adds the search's pops and whether it is still live to the call's pair.  A launch is bounded by
// max_pops, never by a budget, and the state a launch leaves is the state a push leaves: stepped and
// fused calls may alternate on a handle.
// vgreedy_fused_kernel<1 / 2 / 3 / 4 / 8>   126 / 128 / 130 / 132 / 169 VGPRs, 4,432 / 4,528 / 4,624 /
//       4,720 / 5,104 B of LDS (the pop's + 4,096 B of activations + 48 B of scores), no scratch but
//       <2>'s 24 B, which are pop_body<2>'s; vgreedy_fused_kernel<.., cache::Attach> 128 / 133 / 166 / 167 /
//       171 VGPRs, the same LDS (profiles/fused_mlp/kernel_resources.md, where its name
//       has _cached before _kernel).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "acx.h"
#include "acx_moves.h"

#include "acx_batch.h"
#include "acx_beam_key.h"
#include "acx_bfs_common.h"
#include "acx_cache.h"
#include "acx_feat.h"
#include "acx_heap.h"
#include "acx_mlp.h"
#include "acx_pop.h"
#include "acx_scored.h"
#include "acx_visited.h"

namespace acx {
namespace vgreedy {

using namespace acx::bfs;
using namespace acx::pop;
using batch::Buckets;
using scored::ended;

struct State : scored::State {
    int64_t hn;  // entries of the heap
};

struct Args : pop::Args {
    State* state;
    int32_t* counts;   // (n) the pop's candidates per search
    int64_t* offsets;  // (n + 1) their exclusive prefix sum
    int64_t n;         // searches of the running call
};

// The heap's order (acx_heap.h): hk, then the node index.  No entry's hk is all ones: a NaN is
// never keyed, and +inf's key is 0xff800000.
struct Order {
    __device__ __forceinline__ bool less(uint64_t ka, uint32_t va, uint64_t kb, uint32_t vb) const {
        return ka != kb ? ka < kb : va < vb;
    }
    __device__ __forceinline__ uint32_t winner(unsigned long long tied, int lane, uint32_t v) const {
        const bool mine = (tied >> lane) & 1ull;
        const uint32_t vmin = wave_min(mine ? v : NONE);
        return (uint32_t)__builtin_ctzll(__ballot(mine && v == vmin));
    }
};

// The begin and pop kernels' bodies, with the solution cache's probe compiled in or not (CACHE;
// acx_cache.h): the kernels below are their two instantiations each.
template <int NW, bool CACHE>
__device__ __forceinline__ void begin_body(const Args& a, const cache::Attach& at) {
    const int64_t q = blockIdx.x;
    uint64_t* store = a.store + q * a.rows * a.kw;
    uint32_t* meta = a.meta + q * a.rows;
    uint64_t* table = a.table + q * (int64_t)a.nb * BUCKET;
    const batch::Root root = batch::root_setup<GT, NW>(a, q, store, meta, table);
    cache::Hit hit{cache::MISS, 0, 0};
    if constexpr (CACHE) {  // the root is checked before anything (value_guided_search.py:326-330)
        if (!root.refused) hit = cache::probe<NW + 1>(at.view, root.key, a.kw, a.L, threadIdx.x);
    }
    if (threadIdx.x != 0) return;
    // (a search's results are written where it ends)
    if (!root.refused) batch::write_result(a, q, Res{ACX_MBFS_OVERFLOW, 0, 0, 0, 0, 0}, 0, 0, 0);
    a.state[q] = State{{1, root.max_nodes, 0, 1, root.refused, 0, root.total0, 0}, 1};
    (a.depth + q * a.rows)[0] = 0;
    (a.hk + q * a.rows)[0] = 0;  // the root's score decides nothing: it is the only entry
    (a.hid + q * a.rows)[0] = 0;
    a.counts[q] = 0;
    if constexpr (CACHE) {
        at.hit[q] = hit;
        if (hit.entry != cache::MISS) cache::ended_cached(a, q, a.state + q, at, hit, 0, 0, root.total0, 1, 0, 0);
    }
}

template <int NW, class... At>
__global__ __launch_bounds__(GT) void vgreedy_begin_kernel(Args a, At... at) {
    begin_body<NW, sizeof...(At) != 0>(a, cache::attach_of(at...));
}

template <int NW, bool CACHE>
__device__ __forceinline__ void pop_body(const Args& a, const cache::Attach& at) {
    __shared__ uint64_t ck[12 * (NW + 1)];  // the pop's child keys, kw words each
    __shared__ uint32_t slot[12];           // table index of the entry a child holds
    __shared__ uint32_t lost[12];           // an earlier child of the pop took that entry

    const int lane = threadIdx.x;
    const int64_t q = blockIdx.x;
    const int L = a.L, kw = a.kw;
    const bool cyc = a.cyc != 0;
    State* S = a.state + q;
    if (S->done) return;  // (its count is 0 since it ended)
    uint64_t* store = a.store + q * a.rows * kw;
    uint32_t* meta = a.meta + q * a.rows;
    uint32_t* depth = a.depth + q * a.rows;
    uint64_t* hk = a.hk + q * a.rows;
    uint32_t* hid = a.hid + q * a.rows;
    uint64_t* table = a.table + q * (int64_t)a.nb * BUCKET;

    const int64_t n_nodes = S->n_nodes, max_nodes = S->max_nodes, steps = S->steps + 1;
    int64_t hn = S->hn;
    uint32_t running = S->running;
    __syncthreads();  // the state is read before lane 0 rewrites it
    if (hn < 1 || hn > a.rows || n_nodes < 1 || n_nodes > a.rows) {  // (never: an empty heap ends a search below)
        if (lane == 0) ended(a, q, S, ACX_BFS_EXHAUSTED, 0, 0, n_nodes, steps - 1, running, 0);
        return;
    }

    // take: the minimum leaves, the last entry sifts down from the root
    const uint32_t id = hid[0];
    --hn;
    heap::take(hk, hid, hn, lane, Order{});
    if (id >= (uint64_t)n_nodes) {  // (never: a heap entry names an appended node)
        if (lane == 0) ended(a, q, S, ACX_MBFS_OVERFLOW, 0, 0, n_nodes, steps, running, 0);
        return;
    }
    const uint32_t dpar = depth[id];

    // expand
    const Children ch = expand<NW>(store, id, ck, lost, lane, L, kw, cyc, [](uint32_t) {});
    running = min(running, wave_min((uint32_t)lane < ch.seen_to ? ch.tot : NONE));
    __syncthreads();
    if constexpr (CACHE) {
        // the children the reference looks at, in action order: each is probed after its trivial test
        // and before its visited test (:372-380), so the first hit below the first raising or trivial
        // child ends the search; one wave-wide probe per child, at most 12
        const uint32_t upto = min(ch.end0, 12u);
        for (uint32_t c = 0; c < upto; ++c) {
            const cache::Hit hit = cache::probe<NW + 1>(at.view, ck + c * kw, kw, L, lane);
            if (hit.entry == cache::MISS) continue;
            if (lane == 0)
                cache::ended_cached(a, q, S, at, hit, (int32_t)c, id, (uint32_t)key_total(ck + c * kw, L), n_nodes, steps,
                                    (int64_t)dpar + 1);
            return;
        }
    }
    if (ch.end0 != NONE) {  // nodes_explored: the distinct states before this pop's children
        if (lane == 0) {
            if (ch.first_err < ch.first_suc)
                ended(a, q, S, ACX_BFS_MOVE_ERROR, 0, 0, n_nodes, steps, running, 0);
            else
                ended(a, q, S, ACX_BFS_FOUND, (int32_t)ch.first_suc, id, n_nodes, steps, running, (int64_t)dpar + 1);
        }
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
            [&](uint32_t sl, uint64_t displaced) {  // a later child of the pop that held it learns it lost
                slot[lane] = sl;
                const uint64_t lc = displaced - NB;
                if (displaced != visited::NO_CODE && lc < 12u) lost[lc] = 1;
            });
    }
    __syncthreads();
    if (__ballot(ins == visited::FULL)) {  // (uniform) cannot happen at load <= 1/2
        if (lane == 0) ended(a, q, S, ACX_MBFS_OVERFLOW, 0, 0, n_nodes, steps, running, 0);
        return;
    }

    // append the survivors in action order: they are the step's candidates
    const bool alive = lane < 12 && ins == visited::HELD && !lost[lane];
    const Survivors sv = survivors(alive, lane);
    append(alive, sv.rank, lane, id, dpar, n_nodes, a.rows, kw, ck, slot, store, meta, depth, table, [](int64_t) {});
    if (lane != 0) return;
    const uint32_t cnt = sv.cnt;
    const int64_t after = n_nodes + cnt;
    if (cnt == 0 && after >= max_nodes) {  // nothing to score: the budget test, then the loop condition
        ended(a, q, S, ACX_BFS_BUDGET, 0, 0, after, steps, running, 0);
    } else if (cnt == 0 && hn == 0) {
        ended(a, q, S, ACX_BFS_EXHAUSTED, 0, 0, after, steps, running, 0);
    } else {
        S->n_nodes = after;
        S->steps = steps;
        S->hn = hn;
        S->cand_base = n_nodes;
        S->cand_n = (int32_t)cnt;
        S->running = running;
        a.counts[q] = (int32_t)cnt;
    }
}

template <int NW, class... At>
__global__ __launch_bounds__(GT) void vgreedy_pop_kernel(Args a, At... at) {
    pop_body<NW, sizeof...(At) != 0>(a, cache::attach_of(at...));
}

// The push kernel's body: the scores of search q's candidates are scores[off ..], off the search's
// offset (acx_scored.h) or, FUSED, 0: the fused kernel's scores are the search's own M = 12 slots.
template <bool FUSED>
__device__ __forceinline__ void push_body(const Args& a, const float* scores, int64_t M) {
    const int lane = threadIdx.x;
    const int64_t q = blockIdx.x;
    State* S = a.state + q;
    if (S->done) return;
    const int n = a.counts[q];  // 0 for a pop without a candidate
    const int64_t off = FUSED ? 0 : a.offsets[q];
    const int64_t hn = S->hn, base = S->cand_base, n_nodes = S->n_nodes, max_nodes = S->max_nodes;
    if (n == 0) return;
    const int64_t steps = S->steps;
    const uint32_t running = S->running;
    __syncthreads();  // the state is read before lane 0 rewrites it
    // a count, an offset or an M that does not fit the pop (a caller's M that is not the one
    // acx_vgreedy_pop wrote): the candidates cannot enter the heap, so the search ends and says so,
    // with all-zero outputs as a refused search has
    if (n < 0 || n > 12 || off < 0 || off + n > M || hn < 0 || base < 1 || base + n > a.rows || hn + n > a.rows) {
        if (lane == 0) ended(a, q, S, ACX_MBFS_OVERFLOW, 0, 0, n_nodes, 0, 0, 0);
        return;
    }
    uint32_t* depth = a.depth + q * a.rows;
    uint64_t* hk = a.hk + q * a.rows;
    uint32_t* hid = a.hid + q * a.rows;

    const bool alive = lane < n;
    const uint32_t bits = alive ? __float_as_uint(scores[off + lane]) : 0u;
    const bool nan = __ballot(alive && beam::score_is_nan(bits)) != 0;
    __syncthreads();  // the state is read before lane 0 rewrites it
    if (nan || n_nodes >= max_nodes) {  // (uniform) the NaN is sticky; the budget test follows the pushes
        if (lane == 0) ended(a, q, S, nan ? ACX_BEAM_NAN : ACX_BFS_BUDGET, 0, 0, n_nodes, steps, running, 0);
        return;
    }

    // the new leaves, at the heap's end in action order, then into the heap
    const uint64_t myk = alive ? ((uint64_t)beam::score_key(bits) << 32) | depth[base + lane] : ~0ull;
    if (alive) {
        hk[hn + lane] = myk;
        hid[hn + lane] = (uint32_t)(base + lane);
    }
    __syncthreads();
    heap::push(hk, hid, hn, (1u << n) - 1u, (uint32_t)n, alive, hn + lane, myk, base, lane, Order{});
    if (lane == 0) {
        S->hn = hn + n;
        S->cand_n = 0;
    }
}

__global__ __launch_bounds__(GT) void vgreedy_push_kernel(Args a, const float* scores, int64_t M) {
    push_body<false>(a, scores, M);
}

// Up to max_pops pops of search q in one launch, scored by the network (acx_mlp.h): per pop the pop
// kernel's body, then, 4 candidates at a time, lane c's candidate's features from its store row
// (acx_feat.h: acx_features' arithmetic, normalisation included) into LDS and the layers, lane c
// keeping y; then the push kernel's body over the pop's scores.  Lane 0 adds the pops done and
// whether the search is still live to pair.
template <int NW, bool CACHE>
__device__ __forceinline__ void fused_body(const Args& a, const cache::Attach& at, const mlp::Net& net,
                                           const float* mean, const float* stdv, int64_t max_pops,
                                           unsigned long long* pair) {
    __shared__ __attribute__((aligned(16))) float act[mlp::MAX_W][mlp::G];
    __shared__ float sc[12];
    const int lane = threadIdx.x;
    const int64_t q = blockIdx.x;
    const State* S = a.state + q;
    const uint64_t* store = a.store + q * a.rows * a.kw;
    int64_t pops = 0;
    bool done = S->done != 0;
    __syncthreads();  // the state is read before lane 0 rewrites it
    while (!done && pops < max_pops) {
        pop_body<NW, CACHE>(a, at);
        ++pops;
        __syncthreads();
        done = S->done != 0;
        const int n = done ? 0 : min(a.counts[q], 12);
        const int64_t base = S->cand_base;
        for (int c0 = 0; c0 < n; c0 += mlp::G) {  // (uniform)
            __syncthreads();  // the last candidates' chains have read act
            if (lane < mlp::G) {
                float f[feat::NF] = {};
                if (c0 + lane < n && base + c0 + lane < a.rows) {  // (the second: always)
                    PresRegs<NW> p;
                    load_key<NW>(store + (base + c0 + lane) * a.kw, a.kw, a.L, p);
                    feat::Counts k;
                    k.n[0] = p.n0;
                    k.n[1] = p.n1;
#pragma unroll
                    for (uint32_t c = 0; c < 4; ++c) {
                        k.c[0][c] = feat::count_code<NW>(p.w0, p.n0, c);
                        k.c[1][c] = feat::count_code<NW>(p.w1, p.n1, c);
                    }
                    feat::write_features(k, f, mean, stdv);
                }
#pragma unroll
                for (int i = 0; i < feat::NF; ++i) act[i][lane] = f[i];
            }
            __syncthreads();
            const float y = mlp::forward(net, act, lane);
            if (lane < mlp::G && c0 + lane < n) sc[c0 + lane] = y;
        }
        __syncthreads();
        if (n > 0) push_body<true>(a, sc, 12);
        __syncthreads();
        done = S->done != 0;
    }
    if (lane == 0) {
        atomicAdd(pair, (unsigned long long)pops);
        if (!done) atomicAdd(pair + 1, 1ull);
    }
}

// (the attachment is the second argument, as it was when this kernel had a twin: a pack that is
// not last is not deduced, so the launch names it -- vgreedy_fused_kernel<NW, decltype(at)...>)
template <int NW, class... At>
__global__ __launch_bounds__(GT) void vgreedy_fused_kernel(Args a, At... at, mlp::Net net, const float* mean,
                                                           const float* stdv, int64_t max_pops,
                                                           unsigned long long* pair) {
    fused_body<NW, sizeof...(At) != 0>(a, cache::attach_of(at...), net, mean, stdv, max_pops, pair);
}

// what the handle (acx_batch.h) and the step frame (acx_scored.h) need of this engine
struct Engine {
    using Args = vgreedy::Args;
    // a found search's path (value_guided_search.py:87-97,366-367): the edges + (action, 2), no root entry
    // a search that ended on a cache hit below the root: the edges + the (action, total) of the state that hit
    static constexpr uint32_t WITH_PATH = 1u << ACX_BFS_FOUND | 1u << ACX_BFS_CACHED;
    static constexpr bool ROOT_ENTRY = false;
    static constexpr int GATHER_THREADS = GT, MOST = 12;
    static constexpr bool LIVE = true;
    static int64_t rows_for(int64_t B) { return pop::rows_for(B); }
    static uint32_t buckets_for(int64_t B) { return pop::buckets_for(B); }
    template <class F>
    static void arrays(Args& a, F f) {
        pop::arrays(a, f, a.hk, 8, a.hid, 4);
        scored::arrays(a, f);
    }
};
static_assert(sizeof(State) == 56 && scored::RECORD<State> == 140, "the bytes formula of include/acx.h");

}  // namespace vgreedy
}  // namespace acx

namespace vgreedy = acx::vgreedy;
namespace batch = acx::batch;
namespace scored = acx::scored;
using vgreedy::Engine;

extern "C" {

int64_t acx_vgreedy_bytes(int32_t L, int64_t max_nodes_each) { return batch::bytes<Engine>(L, max_nodes_each); }

void* acx_vgreedy_create(int32_t L, int64_t n_searches, int64_t max_nodes_each, int32_t cyclical) {
    return batch::create<Engine>(L, n_searches, max_nodes_each, cyclical);
}

void acx_vgreedy_destroy(void* h) { batch::destroy<Engine>(h); }

int acx_vgreedy_begin(void* h, const int32_t* states, const int64_t* budgets, int64_t n, void* stream) {
    return scored::begin<Engine>(h, states, budgets, true, n, stream, [=](auto nw, const vgreedy::Args& a, auto... at) {
        vgreedy::vgreedy_begin_kernel<decltype(nw)::value>
            <<<dim3((unsigned)a.n), dim3(vgreedy::GT), 0, (hipStream_t)stream>>>(a, at...);
    });
}

int acx_vgreedy_pop(void* h, int64_t* pair, void* stream) {
    return scored::make<Engine>(h, pair, stream, [=](auto nw, const vgreedy::Args& a, auto... at) {
        vgreedy::vgreedy_pop_kernel<decltype(nw)::value>
            <<<dim3((unsigned)a.n), dim3(vgreedy::GT), 0, (hipStream_t)stream>>>(a, at...);
    });
}

int acx_vgreedy_set_cache(void* h, void* cache) { return acx::cache::set_cache<batch::Handle<Engine>>(h, cache); }

int acx_vgreedy_cache_hits(void* h, int64_t n, int64_t* entry, int32_t* rel, int32_t* k, void* stream) {
    return acx::cache::read_hits<batch::Handle<Engine>>(h, n, entry, rel, k, stream);
}

int acx_vgreedy_gather(void* h, uint64_t* keys, int64_t M, void* stream) {
    return scored::gather<Engine>(h, keys, M, stream);
}

int acx_vgreedy_push(void* h, const float* scores, int64_t M, void* stream) {
    return scored::take<Engine>(h, scores, M, stream, [=](const vgreedy::Args& a, hipStream_t st) {
        vgreedy::vgreedy_push_kernel<<<dim3((unsigned)a.n), dim3(vgreedy::GT), 0, st>>>(a, scores, M);
    });
}

int acx_vgreedy_run_mlp(void* h, const float* params, const int32_t* dims, int32_t n_layers, const float* mean,
                        const float* stdv, int64_t max_pops, int64_t* pair, void* stream) {
    batch::Handle<Engine>* S = static_cast<batch::Handle<Engine>*>(h);
    if (!S || !acx::mlp::aligned(params) || !acx::mlp::valid(dims, n_layers) || (!mean != !stdv) || max_pops < 1 || !pair)
        return ACX_E_ARG;
    const vgreedy::Args& a = S->a;
    hipStream_t st = (hipStream_t)stream;
    unsigned long long* out = reinterpret_cast<unsigned long long*>(pair);
    if (hipMemsetAsync(out, 0, 16, st) != hipSuccess) return ACX_E_LAUNCH;
    if (a.n == 0) return ACX_OK;
    const acx::mlp::Net net = acx::mlp::net_of(params, dims, n_layers);
    scored::launch_by_cache(S, [=](auto nw, const vgreedy::Args& a, auto... at) {
        vgreedy::vgreedy_fused_kernel<decltype(nw)::value, decltype(at)...>
            <<<dim3((unsigned)a.n), dim3(vgreedy::GT), 0, st>>>(a, at..., net, mean, stdv, max_pops, out);
    });
    return hipGetLastError() == hipSuccess ? ACX_OK : ACX_E_LAUNCH;
}

int acx_vgreedy_finish(void* h, int32_t* status, int64_t* nodes, int64_t* steps, int32_t* min_length,
                       int64_t* path_len, void* stream) {
    return scored::finish<Engine>(h, status, nodes, steps, min_length, path_len, stream);
}

int acx_vgreedy_paths(void* h, int64_t n, const int64_t* offsets, int32_t* actions, int32_t* totals, int64_t cap,
                      void* stream) {
    return batch::paths<Engine>(h, n, offsets, actions, totals, cap, stream);
}

}  // extern "C"
