// acx_mgreedy.hip -- greedy search over a batch of presentations in one launch: one workgroup of
// one wave (64 threads) owns one search from its root to its verdict, frontier included.  The
// searches are independent, so no workgroup ever waits on another; inside a workgroup the phases
// of a pop are separated by __syncthreads().
//
// Reference: ac_solver/search/greedy.py:15-121.  Per popped node, in the reference's per-child
// order (replay_children in acx_frontier.h states the same order for the host engines): a raising
// move ends the search before any other test on that child (utils.py:264-266); a new minimum is
// counted, duplicates included (:86-89); success (total == 2) is tested before the visited test
// (:91-100); the visited test and the append follow (:102-113); the budget test
// len(tree_nodes) >= max_nodes comes once, after the 12th child (:115-119), so a pop overshoots
// the budget by up to 11 nodes.  On the budget exit or an empty frontier the reference returns
// the last popped node's path plus (11, total of its last child) (:121).
//
// A search's memory is a private slice of each of the handle's arrays, R = B + 11 rows
// (B = max_nodes_each; the overshoot):
//   store  (R, kw) uint64   node keys in append order (node 0 is the root);
//   meta   (R) uint32       parent index << 4 | action (the path reader walks it);
//   depth  (R) uint32       path length of each node;
//   hk     (R) uint64       the frontier, an implicit min-heap of fan-out 64: entry i's children
//   hid    (R) uint32       are 64 i + 1 .. 64 i + 64; hk = prio_k0 of the node (acx_prio.h: total |
//                           depth | the first 8 letter ranks), hid = its index;
//   table  (nb * 8) uint64  the visited set (acx_visited.h), nb = ceil((R + 12) / 4) buckets --
//                           load <= 1/2 of R nodes + the 12 children in flight -- chosen by range
//                           reduction of the hash.
// Bytes per search (acx_mgreedy_bytes):
//   (8 kw + 20) (B + 11) + 64 ceil((B + 23) / 4) + 32,   kw = acx_key_words(L).
//
// A pop runs, with a barrier between:
//   take    (acx_heap.h) the minimum is entry 0; the last entry sifts down from the root.  Only
//           when several children tie on the smallest hk are their keys read from the store --
//           once, into LDS -- and compared (Order, below).  The visited set makes full ties
//           impossible, so the order is total and the pop order is the reference's;
//   expand  (acx_pop.h) lane a < 12 makes child a and writes its key to LDS;
//   insert  lane a below the first raising child / success: visited::insert with code n_nodes + a
//           -- one mbfs round with a single parent: a code below n_nodes names a stored node, a code
//           n_nodes + a a child of this pop, and of two actions that yield the same child the
//           first holds the entry, the other is told (`lost`), as the sequential reference has it;
//   append  (acx_pop.h) the survivors go to rows n_nodes.. and to the heap's end, in action order;
//   push    (acx_heap.h; no verdict, budget not reached) the new leaves are sifted up, ties
//           decided on the keys still in LDS.
// Every loop is bounded: pops by the rows (each pop removes one of at most R appended nodes),
// sifts by the heap height, probes by nb, the path walk by the node's depth.
//
// The heap, the store and the table are shared by the lanes across phases: table reads are
// workgroup-scope atomic loads and the rewrite an atomic store (a pop's code means another child a
// pop later, so no stale value may be read); everything else is plain loads and stores ordered by
// the barriers.  The frame around the pop -- the root and its refusal statuses, the table view,
// the result record, the path reader and the reusable handle behind acx_mgreedy_* -- is
// acx_batch.h, shared with acx_mbfs.hip; the heap and the pop's common phases are shared with
// acx_vgreedy.hip.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "acx.h"
#include "acx_moves.h"

#include "acx_batch.h"
#include "acx_bfs_common.h"
#include "acx_heap.h"
#include "acx_pop.h"
#include "acx_prio.h"
#include "acx_visited.h"

namespace acx {
namespace mgreedy {

using namespace acx::bfs;
using namespace acx::pop;
using batch::Buckets;

// greedy returns a path unless a move raised
constexpr uint32_t WITH_PATH = 1u << ACX_BFS_EXHAUSTED | 1u << ACX_BFS_FOUND | 1u << ACX_BFS_BUDGET;

// The heap's order (acx_heap.h): hk, then the states (prio_cmp_states).  Distinct states, so the
// order is total and every lane ends with the same winner.  The lanes that tie on hk are decided
// on their full keys in LDS, kw words at keys + lane * kw: STAGE, the take, copies them there from
// the store first (once per level, between two barriers: keys is free for the next level); the
// push finds the new leaves' keys where expand left them.
template <bool STAGE>
struct Order {
    const uint64_t* store;
    int kw, L;
    uint64_t* keys;

    __device__ __forceinline__ bool less(uint64_t ka, uint32_t va, uint64_t kb, uint32_t vb) const {
        if (ka != kb) return ka < kb;
        if (va == vb || va == NONE || vb == NONE) return false;
        return prio_cmp_states(store + (uint64_t)va * kw, store + (uint64_t)vb * kw, L) < 0;
    }

    __device__ __forceinline__ uint32_t winner(unsigned long long tied, int lane, uint32_t v) const {
        if (__popcll(tied) == 1) return (uint32_t)__builtin_ctzll(tied);  // (uniform)
        if constexpr (STAGE) {
            if ((tied >> lane) & 1ull)
                for (int j = 0; j < kw; ++j) keys[lane * kw + j] = store[(uint64_t)v * kw + j];
            __syncthreads();
        }
        uint32_t b = (tied >> lane) & 1ull ? (uint32_t)lane : NONE;
#pragma unroll 1
        for (int o = 1; o < WAVE; o <<= 1) {
            const uint32_t ob = (uint32_t)__shfl_xor((int)b, o, WAVE);
            if (ob != NONE && (b == NONE || prio_cmp_states(keys + ob * kw, keys + b * kw, L) < 0)) b = ob;
        }
        if constexpr (STAGE) __syncthreads();
        return b;
    }
};

template <int NW>
__global__ __launch_bounds__(GT) void mgreedy_kernel(Args a) {
    __shared__ uint64_t ck[12 * (NW + 1)];  // the pop's child keys, kw words each
    __shared__ uint64_t tk[WAVE * (NW + 1)];  // full keys of heap entries whose hk tie (take)
    __shared__ uint32_t slot[12];   // table index of the entry a child holds
    __shared__ uint32_t ctot[12];   // child total
    __shared__ uint32_t lost[12];   // an earlier child of the pop took that entry

    const int lane = threadIdx.x;
    const int64_t q = blockIdx.x;
    const int L = a.L, kw = a.kw;
    const bool cyc = a.cyc != 0;
    uint64_t* store = a.store + q * a.rows * kw;
    uint32_t* meta = a.meta + q * a.rows;
    uint32_t* depth = a.depth + q * a.rows;
    uint64_t* hk = a.hk + q * a.rows;
    uint32_t* hid = a.hid + q * a.rows;
    uint64_t* table = a.table + q * (int64_t)a.nb * BUCKET;

    const batch::Root root = batch::root_setup<GT, NW>(a, q, store, meta, table);
    if (root.refused) return;
    const int64_t max_nodes = root.max_nodes;
    if (lane == 0) {
        depth[0] = 0;
        hk[0] = prio_k0(root.key, L, (int)root.total0, 0);
        hid[0] = 0;
    }
    __syncthreads();

    int64_t n_nodes = 1, parents = 0, hn = 1;  // hn: entries of the heap
    int64_t end_node = 0;
    int32_t status = ACX_MBFS_OVERFLOW, last_act = 0, last_tot = 0;
    uint32_t running = root.total0;

    for (int64_t pop = 0; pop < a.rows; ++pop) {
        // take: the minimum leaves, the last entry sifts down from the root
        const uint32_t id = hid[0];
        --hn;
        heap::take(hk, hid, hn, lane, Order<true>{store, kw, L, tk});
        const uint32_t dpar = depth[id];

        // expand
        const Children ch = expand<NW>(store, id, ck, lost, lane, L, kw, cyc, [&](uint32_t t) { ctot[lane] = t; });
        const uint32_t first_err = ch.first_err, first_suc = ch.first_suc, end0 = ch.end0, tot = ch.tot;
        __syncthreads();

        // insert: the success / raising child ends the search, later children are not looked at
        const uint64_t NB = (uint64_t)n_nodes;
        visited::Outcome ins = visited::SEEN;
        if (lane < 12 && (uint32_t)lane < end0) {
            const uint64_t code = NB + (uint64_t)lane;
            const Key<NW + 1> key = kload<NW + 1>(ck + lane * kw, kw);
            ins = visited::insert(
                Buckets{table, a.nb}, a.ep, code, khash<NW + 1>(key, kw),
                [&](uint64_t vc) {
                    return vc < NB ? keq<NW + 1>(store + vc * kw, key, kw) : keq<NW + 1>(ck + (vc - NB) * kw, key, kw);
                },
                [&](uint32_t sl, uint64_t displaced) {  // a later child of the pop that held it learns it lost
                    slot[lane] = sl;
                    const uint64_t lc = displaced - NB;
                    if (displaced != visited::NO_CODE && lc < 12u) lost[lc] = 1;
                });
        }
        __syncthreads();
        if (__ballot(ins == visited::FULL)) break;  // (uniform) cannot happen at load <= 1/2

        // append the survivors in action order; a survivor's heap entry goes to the heap's end in
        // the same order (a leaf until the push below)
        const bool alive = ins == visited::HELD && !lost[lane];  // (HELD: a lane below 12)
        const uint64_t myk = alive ? prio_k0(ck + lane * kw, L, (int)tot, (int)(dpar + 1)) : ~0ull;
        const Survivors sv = survivors(alive, lane);
        const int64_t hpos = hn + sv.rank;
        append(alive, sv.rank, lane, id, dpar, n_nodes, a.rows, kw, ck, slot, store, meta, depth, table,
               [&](int64_t pos) {  // (hpos <= pos)
                   hk[hpos] = myk;
                   hid[hpos] = (uint32_t)pos;
               });
        const uint32_t cnt = sv.cnt;
        running = min(running, wave_min((uint32_t)lane < ch.seen_to ? tot : NONE));
        parents += 1;
        end_node = id;
        if (end0 != NONE) {  // the nodes appended before the ending child count (len(tree_nodes))
            n_nodes += cnt;
            if (first_err < first_suc) {
                status = ACX_BFS_MOVE_ERROR;
            } else {
                status = ACX_BFS_FOUND;
                last_act = (int32_t)first_suc;
                last_tot = 2;
            }
            break;
        }
        last_act = 11;
        last_tot = (int32_t)ctot[11];
        if (n_nodes + cnt >= max_nodes) {
            n_nodes += cnt;
            status = ACX_BFS_BUDGET;
            break;
        }
        if (hn + cnt == 0) {  // the frontier ran dry
            status = ACX_BFS_EXHAUSTED;
            break;
        }
        __syncthreads();

        // push: the survivors are leaves at the heap's end; their keys are still in LDS (ck) for the ties
        heap::push(hk, hid, hn, sv.m, cnt, alive, hpos, myk, n_nodes, lane, Order<false>{store, kw, L, ck});
        hn += cnt;
        n_nodes += cnt;
    }

    if (lane == 0) {
        // [(-1, total0)] + the edges to end_node + (last_act, last_tot)
        batch::write_result(a, q, Res{status, last_act, end_node, last_tot, 0, n_nodes}, parents, running,
                            batch::has_path(WITH_PATH, status) ? (int64_t)depth[end_node] + 2 : 0);
    }
}

// what the handle (acx_batch.h) needs of this engine
struct Engine {
    using Args = pop::Args;
    static constexpr uint32_t WITH_PATH = mgreedy::WITH_PATH;
    static constexpr bool ROOT_ENTRY = true;
    static int64_t rows_for(int64_t B) { return pop::rows_for(B); }
    static uint32_t buckets_for(int64_t B) { return pop::buckets_for(B); }
    template <class F>
    static void arrays(Args& a, F f) { pop::arrays(a, f, a.hk, 8, a.hid, 4); }
    template <int NW>
    static void launch(const Args& a, int64_t n, hipStream_t st) {
        mgreedy_kernel<NW><<<dim3((unsigned)n), dim3(GT), 0, st>>>(a);
    }
};

}  // namespace mgreedy
}  // namespace acx

using acx::mgreedy::Engine;
namespace batch = acx::batch;

extern "C" {

int64_t acx_mgreedy_bytes(int32_t L, int64_t max_nodes_each) { return batch::bytes<Engine>(L, max_nodes_each); }

void* acx_mgreedy_create(int32_t L, int64_t n_searches, int64_t max_nodes_each, int32_t cyclical) {
    return batch::create<Engine>(L, n_searches, max_nodes_each, cyclical);
}

void acx_mgreedy_destroy(void* h) { batch::destroy<Engine>(h); }

int acx_mgreedy_run(void* h, const int32_t* states, const int64_t* budgets, int64_t n, int32_t* status, int64_t* nodes,
                    int64_t* parents, int32_t* min_length, int64_t* path_len, void* stream) {
    return batch::run<Engine>(h, states, budgets, n, status, nodes, parents, min_length, path_len, stream);
}

int acx_mgreedy_paths(void* h, int64_t n, const int64_t* offsets, int32_t* actions, int32_t* totals, int64_t cap,
                      void* stream) {
    return batch::paths<Engine>(h, n, offsets, actions, totals, cap, stream);
}

}  // extern "C"
