// acx_vgreedy.hip -- value-guided greedy search over a batch of presentations, scored by the
// caller: one wave (64 threads) owns one search, and a step of all searches is two launches (pop,
// push) with the caller's scorer between them.  The searches are independent, so no workgroup ever
// waits on another.  It is the heap of acx_mgreedy.hip whose keys arrive from the caller's model one
// launch after the nodes they belong to.
//
// Reference: value_search/value_guided_search.py:294-414 (value_guided_greedy_search) with
// solution_cache=None and time_limit=None.  The root is node 0 and the only heap entry; its score
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
//   hk     (R) uint64       the frontier, an implicit min-heap of fan-out 64 (entry i's children
//   hid    (R) uint32       are 64 i + 1 .. 64 i + 64): hk = score_key(score bits) << 32 | depth
//                           (acx_beam_key.h: the floats' order, -0.0 ties with +0.0), hid = the
//                           node's index, which decides ties on hk;
//   table  (nb * 8) uint64  the visited set (acx_visited.h), nb = ceil((R + 12) / 4) buckets;
//   state, res, the five results, the pop's candidate count and its offset (140 bytes).
// Bytes per search (acx_vgreedy_bytes):
//   (8 kw + 20) (B + 11) + 64 ceil((B + 23) / 4) + 140,   kw = acx_key_words(L).
//
// vgreedy_pop_kernel<NW>: take -- the minimum is entry 0; the last entry sifts down from the root,
//   per level the 64 children are one coalesced load (lane = child) and a wave minimum of (hk, hid)
//   by shuffles, 5 levels at most; expand -- lane a < 12 makes child a, the first raising child and
//   the first success come from wave ballots; insert -- visited::insert with the pop's round code
//   n_nodes + a; append -- the survivors go to rows n_nodes.. in action order with parent << 4 |
//   action and their depth, and their table entries are rewritten from the pop's code to the row.
//   The survivors are the step's candidates.  A pop without a survivor is decided here: the budget
//   verdict, then the empty heap.
// vgreedy_offsets_kernel: the per-search candidate counts become offsets; the host reads M (rows to
//   score) and live (searches not ended).  M == 0 with live > 0 is legal: a pop whose children were
//   all known.
// vgreedy_gather_kernel: one contiguous copy per search into the (M, kw) array.
// vgreedy_push_kernel: the candidates' scores; a NaN ends the search (ACX_BEAM_NAN, the beam's
//   value, shared); then the budget verdict; otherwise the new leaves' heap words are written at
//   the heap's end, under at most two parents, and per parent, while the smallest new leaf beats the
//   entry in the parent's slot, lane 0 sifts it up (acx_mgreedy.hip's push).  A search whose
//   candidates do not fit the caller's M ends with ACX_MBFS_OVERFLOW instead of staying live
//   without them.
// Every loop is bounded: pops by the rows (each pop removes one of at most R appended nodes), sifts
// by the heap height, probes by nb, the path walk by the node's depth.
//
// The heap, the store and the table are shared by the lanes across phases: table reads are
// workgroup-scope atomic loads and the rewrite an atomic store (acx_batch.h); everything else is
// plain loads and stores ordered by the barriers and the launch boundaries.
//
// The heap's take and sift are a private copy of acx_mgreedy.hip's: its entry order compares states
// (prio_cmp_states, with LDS key staging for ties) where this one compares two integers, and
// mgreedy_kernel's registers and LDS stay exactly as they were.
//
// Registers and LDS (hipcc --offload-arch=gfx950 -O3, the kernels' metadata, tools/kernel_resources.py):
//   vgreedy_pop_kernel<1 / 2 / 3 / 4 / 8>   41 / 43 / 45 / 47 / 59 VGPRs, 288 / 384 / 480 / 576 / 960 B of
//       LDS: 8 waves per SIMD (<2> also has 24 B of private memory per lane, as mgreedy_kernel<2>);
//       106 SGPRs with 92 / 100 / 118 / 160 / 134 SGPR spills, kept in VGPR lanes (no scratch for
//       them; mgreedy_kernel has 152 / 150 / 132 / 172 / 196);
//   vgreedy_push_kernel   26 VGPRs, no LDS;   vgreedy_offsets_kernel   53 VGPRs, 64 B of LDS;
//   vgreedy_begin_kernel  11 VGPRs, 96 B;     vgreedy_gather_kernel 8 and vgreedy_finish_kernel 13 VGPRs.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "acx.h"
#include "acx_moves.h"

#include "acx_batch.h"
#include "acx_beam_key.h"
#include "acx_bfs_common.h"
#include "acx_visited.h"

namespace acx {
namespace vgreedy {

using namespace acx::bfs;
using batch::Buckets;
using batch::Res;
using visited::BUCKET;

constexpr int GT = WAVE;       // threads per search: one wave (the ballots below rely on it)
constexpr int FAN = 64;        // heap fan-out = lanes of the wave
constexpr int LEVELS = 5;      // 1 + 64 + 64^2 + 64^3 + 64^4 > 2^24 + 11 entries
constexpr int OVERSHOOT = 11;  // nodes a pop can append past the budget
static_assert(GT == WAVE && FAN == WAVE, "one wave per search");

// a search between two launches
struct State {
    int64_t n_nodes, max_nodes, steps, hn, cand_base;  // hn: entries of the heap
    int32_t done, cand_n;
    uint32_t running;  // min total of the root and the children looked at
    int32_t pad;
};

struct Args : batch::Args {  // (depth is batch::Args's)
    uint64_t* hk;
    uint32_t* hid;
    State* state;
    int32_t* counts;   // (n) the pop's candidates per search
    int64_t* offsets;  // (n + 1) their exclusive prefix sum
    int64_t n;         // searches of the running call
};

__device__ __forceinline__ uint64_t shfl_xor64(uint64_t v, int o) {
    const uint32_t lo = (uint32_t)__shfl_xor((int)(uint32_t)v, o, WAVE);
    const uint32_t hi = (uint32_t)__shfl_xor((int)(uint32_t)(v >> 32), o, WAVE);
    return (uint64_t)lo | ((uint64_t)hi << 32);
}

// heap order: (ka, node va) before (kb, node vb).  A lane without an entry holds (~0, NONE): no
// entry's hk is all ones (a NaN is never keyed, and +inf's key is 0xff800000).
__device__ __forceinline__ bool entry_less(uint64_t ka, uint32_t va, uint64_t kb, uint32_t vb) {
    return ka != kb ? ka < kb : va < vb;
}

// the lane holding the wave's least (k, v); kmin, vmin: that entry (every lane gets the same)
__device__ __forceinline__ uint32_t wave_least(uint64_t k, uint32_t v, uint64_t& kmin, uint32_t& vmin) {
    kmin = k;
#pragma unroll
    for (int o = 1; o < WAVE; o <<= 1) {
        const uint64_t w = shfl_xor64(kmin, o);
        kmin = w < kmin ? w : kmin;
    }
    vmin = wave_min(k == kmin ? v : NONE);
    return (uint32_t)__builtin_ctzll(__ballot(k == kmin && v == vmin));
}

__device__ __forceinline__ void finish(const Args& a, int64_t q, State* S, int32_t status, int32_t act, int64_t node,
                                       int64_t n_nodes, int64_t steps, uint32_t running, int64_t plen) {
    batch::write_result(a, q, Res{status, act, node, 2, 0, n_nodes}, steps, running, plen);
    S->done = 1;
    S->n_nodes = n_nodes;
    S->steps = steps;
    S->cand_n = 0;
    a.counts[q] = 0;
}

template <int NW>
__global__ __launch_bounds__(GT) void vgreedy_begin_kernel(Args a) {
    const int64_t q = blockIdx.x;
    uint64_t* store = a.store + q * a.rows * a.kw;
    uint32_t* meta = a.meta + q * a.rows;
    uint64_t* table = a.table + q * (int64_t)a.nb * BUCKET;
    const batch::Root root = batch::root_setup<GT, NW>(a, q, store, meta, table);
    if (threadIdx.x != 0) return;
    // (a search's results are written where it ends)
    if (!root.refused) batch::write_result(a, q, Res{ACX_MBFS_OVERFLOW, 0, 0, 0, 0, 0}, 0, 0, 0);
    a.state[q] = State{1, root.max_nodes, 0, 1, 1, root.refused, 0, root.total0, 0};
    (a.depth + q * a.rows)[0] = 0;
    (a.hk + q * a.rows)[0] = 0;  // the root's score decides nothing: it is the only entry
    (a.hid + q * a.rows)[0] = 0;
    a.counts[q] = 0;
}

template <int NW>
__global__ __launch_bounds__(GT) void vgreedy_pop_kernel(Args a) {
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
        if (lane == 0) finish(a, q, S, ACX_BFS_EXHAUSTED, 0, 0, n_nodes, steps - 1, running, 0);
        return;
    }

    // take: the minimum leaves, the last entry sifts down from the root
    const uint32_t id = hid[0];
    --hn;
    if (hn > 0) {
        const uint64_t xk = hk[hn];
        const uint32_t xv = hid[hn];
        int64_t i = 0;
        for (int lvl = 0; lvl < LEVELS; ++lvl) {
            const int64_t c0 = (int64_t)FAN * i + 1;
            if (c0 >= hn) break;
            const int64_t c = c0 + lane;
            const bool has = c < hn;
            uint64_t k;
            uint32_t v;
            const uint32_t cl = wave_least(has ? hk[c] : ~0ull, has ? hid[c] : NONE, k, v);  // (lane 0 holds an entry)
            if (!entry_less(k, v, xk, xv)) break;
            if (lane == 0) {
                hk[i] = k;
                hid[i] = v;
            }
            i = c0 + cl;
        }
        if (lane == 0) {
            hk[i] = xk;
            hid[i] = xv;
        }
    }
    if (id >= (uint64_t)n_nodes) {  // (never: a heap entry names an appended node)
        if (lane == 0) finish(a, q, S, ACX_MBFS_OVERFLOW, 0, 0, n_nodes, steps, running, 0);
        return;
    }
    const uint32_t dpar = depth[id];

    // expand
    bool raised = false;
    uint32_t tot = NONE;
    if (lane < 12) {
        lost[lane] = 0;
        PresRegs<NW> pr;
        load_key<NW>(store + (uint64_t)id * kw, kw, L, pr);
        const bool clean = is_clean<NW>(pr.w0, pr.n0, pr.w1, pr.n1, cyc);
        PresRegs<NW> c;
        raised = child_of<NW>(pr, clean, lane, L, cyc, c) != ACX_ERR_NONE;
        if (!raised) tot = (uint32_t)(c.n0 + c.n1);
        uint64_t key[NW + 1];
        make_key<NW>(L, c, key);
#pragma unroll
        for (int k = 0; k < NW + 1; ++k)
            if (k < kw) ck[lane * kw + k] = key[k];
    }
    const unsigned long long errb = __ballot(raised);
    const unsigned long long sucb = __ballot(tot == 2u);
    const uint32_t first_err = errb ? (uint32_t)__builtin_ctzll(errb) : NONE;
    const uint32_t first_suc = sucb ? (uint32_t)__builtin_ctzll(sucb) : NONE;
    // the children the reference looks at: below the raising one, up to the success
    const uint32_t end0 = min(first_err, first_suc);
    const uint32_t seen_to = first_suc < first_err ? first_suc + 1 : min(first_err, 12u);
    running = min(running, wave_min((uint32_t)lane < seen_to ? tot : NONE));
    __syncthreads();
    if (end0 != NONE) {  // nodes_explored: the distinct states before this pop's children
        if (lane == 0) {
            if (first_err < first_suc) finish(a, q, S, ACX_BFS_MOVE_ERROR, 0, 0, n_nodes, steps, running, 0);
            else finish(a, q, S, ACX_BFS_FOUND, (int32_t)first_suc, id, n_nodes, steps, running, (int64_t)dpar + 1);
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
        if (lane == 0) finish(a, q, S, ACX_MBFS_OVERFLOW, 0, 0, n_nodes, steps, running, 0);
        return;
    }

    // append the survivors in action order: they are the step's candidates
    const bool alive = lane < 12 && ins == visited::HELD && !lost[lane];
    const uint32_t m = (uint32_t)__ballot(alive);
    const uint32_t cnt = __popc(m);
    const uint32_t rank = __popc(m & ((1u << (lane & 31)) - 1u));
    if (alive) {
        const int64_t pos = n_nodes + rank;
        if (pos < a.rows) {  // (always: n_nodes < max_nodes <= B before the pop)
            for (int k = 0; k < kw; ++k) store[pos * kw + k] = ck[lane * kw + k];
            meta[pos] = (id << 4) | (uint32_t)lane;
            depth[pos] = dpar + 1;
            batch::recode_entry(table, slot[lane], (uint64_t)pos);
        }
    }
    if (lane != 0) return;
    const int64_t after = n_nodes + cnt;
    if (cnt == 0 && after >= max_nodes) {  // nothing to score: the budget test, then the loop condition
        finish(a, q, S, ACX_BFS_BUDGET, 0, 0, after, steps, running, 0);
    } else if (cnt == 0 && hn == 0) {
        finish(a, q, S, ACX_BFS_EXHAUSTED, 0, 0, after, steps, running, 0);
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

// offsets = exclusive prefix sum of counts (n + 1 entries); pair[0] = their sum M, pair[1] = the
// searches that have not ended: one block
__global__ __launch_bounds__(1024) void vgreedy_offsets_kernel(Args a, int64_t* pair) {
    __shared__ uint32_t sh[1024 / WAVE];
    int64_t run = 0, live = 0;
    for (int64_t b = 0; b < a.n; b += 1024) {
        const int64_t i = b + threadIdx.x;
        const uint32_t v = i < a.n ? (uint32_t)a.counts[i] : 0u;
        uint32_t tot, ltot;
        const uint32_t ex = block_excl_scan<1024>(v, sh, tot);
        if (i < a.n) a.offsets[i] = run + ex;
        run += tot;
        __syncthreads();  // sh is rewritten
        block_excl_scan<1024>(i < a.n && !a.state[i].done ? 1u : 0u, sh, ltot);
        live += ltot;
        __syncthreads();  // sh is rewritten by the next chunk
    }
    if (threadIdx.x == 0) {
        a.offsets[a.n] = run;
        pair[0] = run;
        pair[1] = live;
    }
}

// the candidates' keys of search q are consecutive rows of its store: one copy per search
__global__ __launch_bounds__(GT) void vgreedy_gather_kernel(Args a, uint64_t* keys, int64_t M) {
    const int64_t q = blockIdx.x;
    const State* S = a.state + q;
    const int64_t n = a.counts[q], off = a.offsets[q], base = S->cand_base;
    if (n <= 0 || n > 12 || off < 0 || off + n > M || base < 0 || base + n > a.rows) return;
    const uint64_t* src = a.store + (q * a.rows + base) * a.kw;
    uint64_t* dst = keys + off * a.kw;
    for (int64_t t = threadIdx.x; t < n * a.kw; t += GT) dst[t] = src[t];
}

__global__ __launch_bounds__(GT) void vgreedy_push_kernel(Args a, const float* scores, int64_t M) {
    const int lane = threadIdx.x;
    const int64_t q = blockIdx.x;
    State* S = a.state + q;
    if (S->done) return;
    const int n = a.counts[q];  // 0 for a pop without a candidate
    const int64_t off = a.offsets[q];
    const int64_t hn = S->hn, base = S->cand_base, n_nodes = S->n_nodes, max_nodes = S->max_nodes;
    if (n == 0) return;
    const int64_t steps = S->steps;
    const uint32_t running = S->running;
    __syncthreads();  // the state is read before lane 0 rewrites it
    // a count, an offset or an M that does not fit the pop (a caller's M that is not the one
    // acx_vgreedy_pop wrote): the candidates cannot enter the heap, so the search ends and says so,
    // with all-zero outputs as a refused search has
    if (n < 0 || n > 12 || off < 0 || off + n > M || hn < 0 || base < 1 || base + n > a.rows || hn + n > a.rows) {
        if (lane == 0) finish(a, q, S, ACX_MBFS_OVERFLOW, 0, 0, n_nodes, 0, 0, 0);
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
        if (lane == 0) finish(a, q, S, nan ? ACX_BEAM_NAN : ACX_BFS_BUDGET, 0, 0, n_nodes, steps, running, 0);
        return;
    }

    // the new leaves, at the heap's end in action order
    const uint32_t myv = (uint32_t)(base + lane);
    const uint64_t myk = alive ? ((uint64_t)beam::score_key(bits) << 32) | depth[base + lane] : ~0ull;
    if (alive) {
        hk[hn + lane] = myk;
        hid[hn + lane] = myv;
    }
    __syncthreads();

    // The leaves sit under at most two heap parents (12 < 64).  Per parent: while the smallest of
    // its new leaves beats the entry in the parent's slot, lane 0 sifts that leaf up from its slot
    // (the parent's entry moves into the leaf; what settles in the parent's slot is smaller than what
    // was there, so the leaves already dealt with stay in order); the others are looked at again.
    if (hn + n > 1) {
        const int64_t pa = ((hn > 1 ? hn : 1) - 1) / FAN, pb = (hn + (int64_t)n - 2) / FAN;
        for (int64_t p = pa; p <= pb; ++p) {  // (uniform, at most 2)
            bool cand = alive && hn + lane >= 1 && (hn + lane - 1) / FAN == p;
            for (int it = 0; it < 12; ++it) {  // (uniform) each round retires one new leaf
                uint64_t xk;
                uint32_t xv;
                const uint32_t w = wave_least(cand ? myk : ~0ull, cand ? myv : NONE, xk, xv);
                if (xv == NONE) break;  // no leaf left under this parent
                if (!entry_less(xk, xv, hk[p], hid[p])) break;
                if (lane == 0) {
                    int64_t i = hn + w;
                    for (int lvl = 0; lvl < LEVELS && i > 0; ++lvl) {
                        const int64_t par = (i - 1) / FAN;
                        const uint64_t pk = hk[par];
                        const uint32_t pv = hid[par];
                        if (!entry_less(xk, xv, pk, pv)) break;
                        hk[i] = pk;
                        hid[i] = pv;
                        i = par;
                    }
                    hk[i] = xk;
                    hid[i] = xv;
                }
                cand = cand && (uint32_t)lane != w;
                __syncthreads();
            }
        }
    }
    if (lane == 0) {
        S->hn = hn + n;
        S->cand_n = 0;
    }
}

__global__ __launch_bounds__(TPB) void vgreedy_finish_kernel(Args a, int32_t* status, int64_t* nodes, int64_t* steps,
                                                             int32_t* min_length, int64_t* path_len) {
    const int64_t q = (int64_t)blockIdx.x * TPB + threadIdx.x;
    if (q >= a.n) return;
    status[q] = a.status[q];
    nodes[q] = a.nodes[q];
    steps[q] = a.parents[q];
    min_length[q] = a.min_length[q];
    path_len[q] = a.path_len[q];
}

// what the handle (acx_batch.h) needs of this engine
struct Engine {
    using Args = vgreedy::Args;
    // a found search's path (value_guided_search.py:87-97,366-367): the edges + (action, 2), no root entry
    static constexpr uint32_t WITH_PATH = 1u << ACX_BFS_FOUND;
    static constexpr bool ROOT_ENTRY = false;
    static int64_t rows_for(int64_t B) { return B + OVERSHOOT; }
    static uint32_t buckets_for(int64_t B) { return (uint32_t)((2 * (rows_for(B) + 12) + BUCKET - 1) / BUCKET); }
    template <class F>
    static void arrays(Args& a, F f) {
        const size_t R = (size_t)a.rows;
        f(a.store, 8 * (size_t)a.kw * R, false);
        f(a.meta, 4 * R, false);
        f(a.depth, 4 * R, false);
        f(a.hk, 8 * R, false);
        f(a.hid, 4 * R, false);
        f(a.table, 8 * (size_t)BUCKET * a.nb, true);
        f(a.res, sizeof(Res), true);
        f(a.state, sizeof(State), true);  // (zeroed: no candidates before the first begin)
        f(a.counts, 4, true);
        f(a.offsets, 16, true);  // n + 1 entries
        f(a.status, 4, true);
        f(a.nodes, 8, true);
        f(a.parents, 8, true);  // steps
        f(a.min_length, 4, true);
        f(a.path_len, 8, true);
    }
};
using Handle = batch::Handle<Engine>;
static_assert(sizeof(Res) + sizeof(State) + 4 + 16 + 4 + 8 + 8 + 4 + 8 == 140, "the bytes formula of include/acx.h");

struct Begin {
    const Args& a;
    hipStream_t st;
    template <int NW>
    void go() { vgreedy_begin_kernel<NW><<<dim3((unsigned)a.n), dim3(GT), 0, st>>>(a); }
};
struct Pop {
    const Args& a;
    hipStream_t st;
    template <int NW>
    void go() { vgreedy_pop_kernel<NW><<<dim3((unsigned)a.n), dim3(GT), 0, st>>>(a); }
};

}  // namespace vgreedy
}  // namespace acx

namespace vgreedy = acx::vgreedy;
namespace batch = acx::batch;
using vgreedy::Handle;

extern "C" {

int64_t acx_vgreedy_bytes(int32_t L, int64_t max_nodes_each) { return batch::bytes<vgreedy::Engine>(L, max_nodes_each); }

void* acx_vgreedy_create(int32_t L, int64_t n_searches, int64_t max_nodes_each, int32_t cyclical) {
    return batch::create<vgreedy::Engine>(L, n_searches, max_nodes_each, cyclical);
}

void acx_vgreedy_destroy(void* h) { batch::destroy<vgreedy::Engine>(h); }

int acx_vgreedy_begin(void* h, const int32_t* states, const int64_t* budgets, int64_t n, void* stream) {
    Handle* S = static_cast<Handle*>(h);
    if (!S || !states || !budgets || n < 0 || n > S->n_cap) return ACX_E_ARG;
    vgreedy::Args& a = S->a;
    a.n = n;
    if (n == 0) return ACX_OK;
    hipStream_t st = (hipStream_t)stream;
    if (!batch::new_epoch(S, st)) return ACX_E_LAUNCH;
    a.states = states;
    a.budgets = budgets;
    acx::bfs::by_nw(a.L, vgreedy::Begin{a, st});
    return hipGetLastError() == hipSuccess ? ACX_OK : ACX_E_LAUNCH;
}

int acx_vgreedy_pop(void* h, int64_t* pair, void* stream) {
    Handle* S = static_cast<Handle*>(h);
    if (!S || !pair) return ACX_E_ARG;
    const vgreedy::Args& a = S->a;
    hipStream_t st = (hipStream_t)stream;
    if (a.n > 0) acx::bfs::by_nw(a.L, vgreedy::Pop{a, st});
    vgreedy::vgreedy_offsets_kernel<<<dim3(1), dim3(1024), 0, st>>>(a, pair);
    return hipGetLastError() == hipSuccess ? ACX_OK : ACX_E_LAUNCH;
}

int acx_vgreedy_gather(void* h, uint64_t* keys, int64_t M, void* stream) {
    Handle* S = static_cast<Handle*>(h);
    if (!S || M < 0 || (M > 0 && !keys)) return ACX_E_ARG;
    const vgreedy::Args& a = S->a;
    if (a.n == 0 || M == 0) return ACX_OK;
    vgreedy::vgreedy_gather_kernel<<<dim3((unsigned)a.n), dim3(vgreedy::GT), 0, (hipStream_t)stream>>>(a, keys, M);
    return hipGetLastError() == hipSuccess ? ACX_OK : ACX_E_LAUNCH;
}

int acx_vgreedy_push(void* h, const float* scores, int64_t M, void* stream) {
    Handle* S = static_cast<Handle*>(h);
    if (!S || M < 0 || (M > 0 && !scores)) return ACX_E_ARG;
    const vgreedy::Args& a = S->a;
    if (a.n == 0 || M == 0) return ACX_OK;
    vgreedy::vgreedy_push_kernel<<<dim3((unsigned)a.n), dim3(vgreedy::GT), 0, (hipStream_t)stream>>>(a, scores, M);
    return hipGetLastError() == hipSuccess ? ACX_OK : ACX_E_LAUNCH;
}

int acx_vgreedy_finish(void* h, int32_t* status, int64_t* nodes, int64_t* steps, int32_t* min_length,
                       int64_t* path_len, void* stream) {
    Handle* S = static_cast<Handle*>(h);
    if (!S || !status || !nodes || !steps || !min_length || !path_len) return ACX_E_ARG;
    const vgreedy::Args& a = S->a;
    if (a.n == 0) return ACX_OK;
    vgreedy::vgreedy_finish_kernel<<<dim3((unsigned)((a.n + acx::bfs::TPB - 1) / acx::bfs::TPB)), dim3(acx::bfs::TPB), 0,
                                     (hipStream_t)stream>>>(a, status, nodes, steps, min_length, path_len);
    return hipGetLastError() == hipSuccess ? ACX_OK : ACX_E_LAUNCH;
}

int acx_vgreedy_paths(void* h, int64_t n, const int64_t* offsets, int32_t* actions, int32_t* totals, int64_t cap,
                      void* stream) {
    return batch::paths<vgreedy::Engine>(h, n, offsets, actions, totals, cap, stream);
}

}  // extern "C"
