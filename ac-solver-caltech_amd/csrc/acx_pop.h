// acx_pop.h -- what a step of the one-wave-per-search engines has in common (acx_mgreedy.hip,
// acx_vgreedy.hip, acx_mcts.hip): the engine picks a node -- the heap engines, mgreedy and vgreedy,
// the least entry of the search's heap; mcts the leaf of a descent of its tree -- makes the node's 12
// children, looks at them in the reference's per-child order and appends the new ones.
//
// Here: the slice's shape (rows_for, buckets_for, arrays), expand, survivors and append.  Args'
// hk / hid and acx_heap.h are the heap engines' only; mcts has its records and its trail in their
// place.  The insert between expand and append stays written in each kernel: as a shared routine
// it cost mgreedy_kernel<8> 14 VGPRs (profiles/batch_shared/kernel_resources.md), and, shared by
// the two scored engines alone, mcts_select_kernel<8> 12 (87 -> 99: a wave per SIMD less;
// profiles/mcts/kernel_resources.md); greedy also differs in which lanes insert.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "acx.h"
#include "acx_moves.h"

#include "acx_batch.h"
#include "acx_bfs_common.h"
#include "acx_visited.h"

namespace acx {
namespace pop {

using namespace acx::bfs;
using batch::Res;
using visited::BUCKET;

constexpr int GT = WAVE;       // threads per search: one wave (the ballots below rely on it)
constexpr int OVERSHOOT = 11;  // nodes a pop can append past the budget
static_assert(GT == WAVE, "one wave per search");

struct Args : batch::Args {  // (depth is batch::Args's)
    uint64_t* hk;
    uint32_t* hid;
};

// rows of a search's slice at budgets up to B (the budget is tested once per pop, after the 12th
// child), and its buckets: load <= 1/2 with those rows and the 12 children in flight
inline int64_t rows_for(int64_t B) { return B + OVERSHOOT; }
inline uint32_t buckets_for(int64_t B) { return (uint32_t)((2 * (rows_for(B) + 12) + BUCKET - 1) / BUCKET); }

// a slice's arrays, for the engine's Engine::arrays (acx_batch.h); o1, o2: the engine's own two, of
// b1, b2 bytes per row (the heap engines' hk, hid; mcts's rec, trail)
template <class A, class F, class O1, class O2>
void arrays(A& a, F f, O1*& o1, size_t b1, O2*& o2, size_t b2) {
    const size_t R = (size_t)a.rows;
    f(a.store, 8 * (size_t)a.kw * R, false);
    f(a.meta, 4 * R, false);
    f(a.depth, 4 * R, false);
    f(o1, b1 * R, false);
    f(o2, b2 * R, false);
    f(a.table, 8 * (size_t)BUCKET * a.nb, true);
    f(a.res, sizeof(Res), true);
}

// a pop's children: the first raising one and the first success (NONE: there is none); the ones
// the reference looks at -- below end0 they meet the visited set, below seen_to they count for
// min_length; the lane's own child's total (NONE: the move raised, or a lane without a child)
struct Children {
    uint32_t first_err, first_suc, end0, seen_to, tot;
};

// expand node `id`: lane a < 12 clears lost[a], makes child a, writes its key to ck + a * kw and
// hands its total to own(tot)
template <int NW, class Own>
__device__ __forceinline__ Children expand(const uint64_t* store, uint32_t id, uint64_t* ck, uint32_t* lost, int lane,
                                           int L, int kw, bool cyc, Own own) {
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
        own(tot);
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
    return Children{first_err, first_suc, min(first_err, first_suc),
                    first_suc < first_err ? first_suc + 1 : min(first_err, 12u), tot};
}

// the survivors of a pop: their lanes, their number, and the lane's rank among them
struct Survivors {
    uint32_t m, cnt, rank;
};

__device__ __forceinline__ Survivors survivors(bool alive, int lane) {
    const uint32_t m = (uint32_t)__ballot(alive);
    return Survivors{m, (uint32_t)__popc(m), (uint32_t)__popc(m & ((1u << (lane & 31)) - 1u))};
}

// append the survivors (`alive`: this lane's child is one, the rank-th) of node id's pop in action
// order; a survivor in row pos then calls own(pos)
template <class Own>
__device__ __forceinline__ void append(bool alive, uint32_t rank, int lane, uint32_t id, uint32_t dpar, int64_t n_nodes,
                                       int64_t rows, int kw, const uint64_t* ck, const uint32_t* slot, uint64_t* store,
                                       uint32_t* meta, uint32_t* depth, uint64_t* table, Own own) {
    if (!alive) return;
    const int64_t pos = n_nodes + rank;
    if (pos >= rows) return;  // (never: n_nodes < max_nodes <= B before the pop)
    for (int k = 0; k < kw; ++k) store[pos * kw + k] = ck[lane * kw + k];
    meta[pos] = (id << 4) | (uint32_t)lane;
    depth[pos] = dpar + 1;
    own(pos);
    batch::recode_entry(table, slot[lane], (uint64_t)pos);
}

}  // namespace pop
}  // namespace acx
