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
//   take    the minimum is entry 0; the last entry sifts down from the root: per level the 64
//           children are one coalesced load (lane = child) and a wave minimum of hk by shuffles,
//           5 levels at most (64^4 > 2^24 nodes).  Only when several children tie on the smallest
//           hk are their keys read from the store -- once, into LDS -- and compared
//           (prio_cmp_states).  The visited set makes full ties impossible, so the order is total
//           and the pop order is the reference's;
//   expand  lane a < 12 makes child a (child_of, acx_bfs_common.h) and writes its key to LDS;
//           the first raising child and the first success come from wave ballots;
//   insert  lane a below the first of them: visited::insert with code n_nodes + a -- one mbfs
//           round with a single parent: a code below n_nodes names a stored node, a code
//           n_nodes + a a child of this pop, and of two actions that yield the same child the
//           first holds the entry, the other is told (`lost`), as the sequential reference has it;
//   append  the survivors go to rows n_nodes.. in action order with parent << 4 | action and
//           their depth, and their table entries are rewritten from the pop's code to the row;
//   push    (no verdict, budget not reached) the survivors are already leaves at the heap's end,
//           under at most two parents; per parent, while the smallest new leaf (wave minimum,
//           ties decided on the keys still in LDS) beats the entry in the parent's slot, lane 0
//           sifts it up, at most ceil(log64 n) steps; a leaf that does not beat it stays.
// Every loop is bounded: pops by the rows (each pop removes one of at most R appended nodes),
// sifts by the heap height, probes by nb, the path walk by the node's depth.
//
// The heap, the store and the table are shared by the lanes across phases: table reads are
// workgroup-scope atomic loads and the rewrite an atomic store (a pop's code means another child a
// pop later, so no stale value may be read); everything else is plain loads and stores ordered by
// the barriers.  The frame around the pop -- the root and its refusal statuses, the table view,
// the result record, the path reader and the reusable handle behind acx_mgreedy_* -- is
// acx_batch.h, shared with acx_mbfs.hip.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "acx.h"
#include "acx_moves.h"

#include "acx_batch.h"
#include "acx_bfs_common.h"
#include "acx_prio.h"
#include "acx_visited.h"

namespace acx {
namespace mgreedy {

using namespace acx::bfs;
using batch::Buckets;
using batch::Res;
using visited::BUCKET;

constexpr int GT = WAVE;        // threads per search: one wave (the ballots below rely on it)
constexpr int FAN = 64;         // heap fan-out = lanes of the wave
constexpr int LEVELS = 5;       // 1 + 64 + 64^2 + 64^3 + 64^4 > 2^24 + 11 entries
constexpr int OVERSHOOT = 11;   // nodes a pop can append past the budget
static_assert(GT == WAVE && FAN == WAVE, "one wave per search");

struct Args : batch::Args {  // (depth is batch::Args's)
    uint64_t* hk;
    uint32_t* hid;
};

// greedy returns a path unless a move raised
constexpr uint32_t WITH_PATH = 1u << ACX_BFS_EXHAUSTED | 1u << ACX_BFS_FOUND | 1u << ACX_BFS_BUDGET;

__device__ __forceinline__ uint64_t shfl_xor64(uint64_t v, int o) {
    const uint32_t lo = (uint32_t)__shfl_xor((int)(uint32_t)v, o, WAVE);
    const uint32_t hi = (uint32_t)__shfl_xor((int)(uint32_t)(v >> 32), o, WAVE);
    return (uint64_t)lo | ((uint64_t)hi << 32);
}

// heap order: (ka, node va) before (kb, node vb).  A lane without an entry holds (~0, NONE): no
// node's hk is all ones (a total is at most 2 ACX_MAX_L < 511).
__device__ __forceinline__ bool entry_less(uint64_t ka, uint32_t va, uint64_t kb, uint32_t vb, const uint64_t* store,
                                           int kw, int L) {
    if (ka != kb) return ka < kb;
    if (va == vb || va == NONE || vb == NONE) return false;
    return prio_cmp_states(store + (uint64_t)va * kw, store + (uint64_t)vb * kw, L) < 0;
}

__device__ __forceinline__ uint64_t wave_min64(uint64_t v) {
#pragma unroll
    for (int o = 1; o < WAVE; o <<= 1) {
        const uint64_t w = shfl_xor64(v, o);
        v = w < v ? w : v;
    }
    return v;
}

// The lane holding the wave's smallest entry, given the lanes `tied` (more than one) whose hk is
// the wave's minimum: their full keys, kw words at keys + lane * kw (LDS), decide.  Distinct
// states, so every lane ends with the same winner.
__device__ __forceinline__ uint32_t tie_winner(unsigned long long tied, int lane, const uint64_t* keys, int kw, int L) {
    uint32_t b = (tied >> lane) & 1ull ? (uint32_t)lane : NONE;
#pragma unroll 1
    for (int o = 1; o < WAVE; o <<= 1) {
        const uint32_t ob = (uint32_t)__shfl_xor((int)b, o, WAVE);
        if (ob != NONE && (b == NONE || prio_cmp_states(keys + ob * kw, keys + b * kw, L) < 0)) b = ob;
    }
    return b;
}

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
        if (hn > 0) {
            const uint64_t xk = hk[hn];
            const uint32_t xv = hid[hn];
            int64_t i = 0;
            for (int lvl = 0; lvl < LEVELS; ++lvl) {
                const int64_t c0 = (int64_t)FAN * i + 1;
                if (c0 >= hn) break;
                const int64_t c = c0 + lane;
                const bool has = c < hn;
                uint64_t k = has ? hk[c] : ~0ull;
                uint32_t v = has ? hid[c] : NONE;
                // the smallest hk by shuffles alone; the full keys only of the lanes that tie on
                // it, read once into LDS (lane 0 holds an entry: c0 < hn)
                const uint64_t kmin = wave_min64(k);
                const unsigned long long tied = __ballot(has && k == kmin);
                uint32_t cl = (uint32_t)__builtin_ctzll(tied);
                if (__popcll(tied) > 1) {  // (uniform)
                    if ((tied >> lane) & 1ull)
                        for (int j = 0; j < kw; ++j) tk[lane * kw + j] = store[(uint64_t)v * kw + j];
                    __syncthreads();
                    cl = tie_winner(tied, lane, tk, kw, L);
                    __syncthreads();  // tk is free for the next level
                }
                k = kmin;
                v = (uint32_t)__shfl((int)v, (int)cl, WAVE);
                if (!entry_less(k, v, xk, xv, store, kw, L)) break;
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
            ctot[lane] = tot;
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

        // append the survivors in action order
        const bool alive = ins == visited::HELD && !lost[lane];  // (HELD: a lane below 12)
        const uint32_t m = (uint32_t)__ballot(alive);
        const uint32_t cnt = __popc(m);
        // a survivor's heap entry, at the heap's end in action order (a leaf until the push below)
        const uint32_t rank = __popc(m & ((1u << (lane & 31)) - 1u));
        const int64_t hpos = hn + rank;
        const uint64_t myk = alive ? prio_k0(ck + lane * kw, L, (int)tot, (int)(dpar + 1)) : ~0ull;
        if (alive) {
            const int64_t pos = n_nodes + rank;
            if (pos < a.rows) {  // (always: n_nodes < max_nodes <= B before the pop; hpos <= pos)
                for (int k = 0; k < kw; ++k) store[pos * kw + k] = ck[lane * kw + k];
                meta[pos] = (id << 4) | (uint32_t)lane;
                depth[pos] = dpar + 1;
                hk[hpos] = myk;
                hid[hpos] = (uint32_t)pos;
                batch::recode_entry(table, slot[lane], (uint64_t)pos);
            }
        }
        running = min(running, wave_min((uint32_t)lane < seen_to ? tot : NONE));
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

        // push: the survivors are leaves under at most two heap parents (12 < 64).  Per parent: while
        // the smallest of its new leaves beats the entry in the parent's slot, lane 0 sifts that
        // leaf up from its slot (the parent's entry moves into the leaf; what settles in the
        // parent's slot is smaller than what was there, so the leaves already dealt with stay in
        // order); the others are looked at again.  Mostly one wave minimum per parent instead of
        // one sift per survivor.  The children's keys are still in LDS (ck) for the ties.
        if (hn + cnt > 1) {
            const int64_t pa = ((hn > 1 ? hn : 1) - 1) / FAN, pb = (hn + (int64_t)cnt - 2) / FAN;
            for (int64_t p = pa; p <= pb; ++p) {  // (uniform, at most 2)
                bool cand = alive && hpos >= 1 && (hpos - 1) / FAN == p;
                for (int it = 0; it < 12; ++it) {  // (uniform) each round retires one new leaf
                    const uint64_t xk = wave_min64(cand ? myk : ~0ull);
                    const unsigned long long tied = __ballot(cand && myk == xk);
                    if (!tied) break;
                    uint32_t w = (uint32_t)__builtin_ctzll(tied);
                    if (__popcll(tied) > 1) w = tie_winner(tied, lane, ck, kw, L);
                    const uint32_t wr = __popc(m & ((1u << w) - 1u));
                    const uint32_t xv = (uint32_t)(n_nodes + wr);
                    if (!entry_less(xk, xv, hk[p], hid[p], store, kw, L)) break;
                    if (lane == 0) {
                        int64_t i = hn + wr;
                        for (int lvl = 0; lvl < LEVELS && i > 0; ++lvl) {
                            const int64_t par = (i - 1) / FAN;
                            const uint64_t pk = hk[par];
                            const uint32_t pv = hid[par];
                            if (!entry_less(xk, xv, pk, pv, store, kw, L)) break;
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
    using Args = mgreedy::Args;
    static constexpr uint32_t WITH_PATH = mgreedy::WITH_PATH;
    static constexpr bool ROOT_ENTRY = true;
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
    }
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
