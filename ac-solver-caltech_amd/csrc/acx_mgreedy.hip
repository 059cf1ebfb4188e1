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
// The heap, the store and the table are shared by the lanes across phases.  Table reads are
// workgroup-scope atomic loads and the rewrite an atomic store, as in acx_mbfs.hip (a pop's code
// means another child a pop later, so no stale value may be read); everything else is plain
// loads and stores ordered by the barriers.  Nothing needs a wider scope: a search's memory is
// touched by its own workgroup alone.  A handle is reusable: table entries carry the run's epoch
// (visited::next_epoch), and every other array is written before it is read.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <new>

#include "acx.h"
#include "acx_moves.h"

#include "acx_bfs_common.h"
#include "acx_prio.h"
#include "acx_visited.h"

namespace acx {
namespace mgreedy {

using namespace acx::bfs;
using visited::BUCKET;

constexpr int GT = WAVE;        // threads per search: one wave (the ballots below rely on it)
constexpr int FAN = 64;         // heap fan-out = lanes of the wave
constexpr int LEVELS = 5;       // 1 + 64 + 64^2 + 64^3 + 64^4 > 2^24 + 11 entries
constexpr int OVERSHOOT = 11;   // nodes a pop can append past the budget
constexpr int64_t MAX_NODES_EACH = 1ll << 24;
constexpr int RKW = ACX_MAX_L / 16 + 2;  // words of the largest key, rounded up
static_assert(GT == WAVE && FAN == WAVE, "one wave per search");

// what the path reader needs of a finished search: the path is the one to `end_node` (the success
// child's parent, or the last popped node) plus (last_act, last_tot)
struct Res {
    int32_t status, last_act;
    int64_t end_node;
    int32_t last_tot, pad;
    int64_t nodes;
};

struct Args {
    const int32_t* states;   // (n, 2L)
    const int64_t* budgets;  // (n)
    uint64_t* store;
    uint32_t* meta;
    uint32_t* depth;
    uint64_t* hk;
    uint32_t* hid;
    uint64_t* table;
    Res* res;
    int32_t* status;
    int64_t* nodes;
    int64_t* parents;
    int32_t* min_length;
    int64_t* path_len;
    int64_t maxb;  // B: the largest budget a search may have
    int64_t rows;  // R = B + 11
    uint32_t nb;   // buckets per search
    uint64_t ep;   // this run's epoch, shifted (visited::next_epoch)
    int L, kw, cyc;
};

// a table entry as the workgroup last wrote it (acx_mbfs.hip: workgroup scope is the whole of it)
__device__ __forceinline__ uint64_t wload(const uint64_t* p) {
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}

struct Buckets {
    using Index = uint32_t;
    uint64_t* table;
    uint32_t nb;
    __device__ __forceinline__ Index buckets() const { return nb; }
    __device__ __forceinline__ Index first(uint64_t h) const { return __umulhi((uint32_t)h, nb); }
    __device__ __forceinline__ Index next(Index b) const { return b + 1 == nb ? 0 : b + 1; }
    __device__ __forceinline__ uint64_t* bucket(Index b) const { return table + (uint64_t)b * BUCKET; }
    __device__ __forceinline__ void load(const uint64_t* bk, uint64_t (&e)[BUCKET]) const {
#pragma unroll
        for (int j = 0; j < BUCKET; ++j) e[j] = wload(bk + j);
    }
};

static inline int64_t rows_for(int64_t B) { return B + OVERSHOOT; }
static inline uint32_t buckets_for(int64_t B) { return (uint32_t)((2 * (rows_for(B) + 12) + BUCKET - 1) / BUCKET); }

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
    __shared__ uint64_t rk[RKW];
    __shared__ uint32_t slot[12];   // table index of the entry a child holds
    __shared__ uint32_t ctot[12];   // child total
    __shared__ uint32_t lost[12];   // an earlier child of the pop took that entry
    __shared__ uint32_t s_n[2], s_bad;

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

    // the root: packed by the wave (acx_key.h format), checked against the packed domain
    if (lane < RKW) rk[lane] = 0;
    if (lane < 2) s_n[lane] = 0;
    if (lane == 0) s_bad = 0;
    __syncthreads();
    {
        const int32_t* st = a.states + q * 2 * L;
        for (int t = lane; t < 2 * L; t += GT) {
            const int32_t v = st[t];
            const int h = t >= L, i = t - h * L;
            bool bad = v < -2 || v > 2;
            if (v == 0) {
                bad = i + 1 < L && st[t + 1] != 0;  // zeros only as right padding
            } else if (!bad) {
                const int bit = 2 * t;
                atomicOr((unsigned long long*)&rk[bit >> 6], (unsigned long long)(key_code(v) << (bit & 63)));
                atomicAdd(&s_n[h], 1u);
            }
            if (bad) s_bad = 1;
        }
    }
    __syncthreads();
    int64_t max_nodes = a.budgets[q];
    if (max_nodes < 1) max_nodes = 1;  // the reference still expands the root once
    const uint32_t total0 = s_n[0] + s_n[1];
    const bool dom = s_bad || s_n[0] == 0 || s_n[1] == 0;
    if (dom || max_nodes > a.maxb) {
        if (lane == 0) {
            const int32_t st = dom ? ACX_MBFS_DOMAIN : ACX_MBFS_OVERFLOW;
            a.status[q] = st;
            a.nodes[q] = 0;
            a.parents[q] = 0;
            a.min_length[q] = 0;
            a.path_len[q] = 0;
            a.res[q] = Res{st, 0, 0, 0, 0, 0};
        }
        return;
    }
    if (lane == 0) {
        const uint64_t lens = (uint64_t)s_n[0] | ((uint64_t)s_n[1] << 8);
        const int bit = 4 * L;
        rk[bit / 64] |= lens << (bit % 64);
        if (bit % 64 > 48 && bit / 64 + 1 < kw) rk[bit / 64 + 1] |= lens >> (64 - bit % 64);
    }
    __syncthreads();
    if (lane < kw) store[lane] = rk[lane];
    if (lane == 0) {
        const Key<NW + 1> key = kload<NW + 1>(rk, kw);
        const uint64_t h = khash<NW + 1>(key, kw);
        const Buckets tb{table, a.nb};
        __hip_atomic_store(tb.bucket(tb.first(h)), visited::entry(a.ep, 0, visited::fp_of(h)), __ATOMIC_RELAXED,
                           __HIP_MEMORY_SCOPE_WORKGROUP);  // node 0
        meta[0] = 0;
        depth[0] = 0;
        hk[0] = prio_k0(rk, L, (int)total0, 0);
        hid[0] = 0;
    }
    __syncthreads();

    int64_t n_nodes = 1, parents = 0, hn = 1;  // hn: entries of the heap
    int64_t end_node = 0;
    int32_t status = ACX_MBFS_OVERFLOW, last_act = 0, last_tot = 0;
    uint32_t running = total0;

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
                uint64_t* ent = table + slot[lane];
                const uint64_t v = wload(ent);
                __hip_atomic_store(ent, visited::entry_recode(v, (uint64_t)pos), __ATOMIC_RELAXED,
                                   __HIP_MEMORY_SCOPE_WORKGROUP);
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
        const bool path = status == ACX_BFS_EXHAUSTED || status == ACX_BFS_FOUND || status == ACX_BFS_BUDGET;
        // [(-1, total0)] + the edges to end_node + (last_act, last_tot)
        a.status[q] = status;
        a.nodes[q] = status < 0 ? 0 : n_nodes;
        a.parents[q] = parents;
        a.min_length[q] = (int32_t)running;
        a.path_len[q] = path ? (int64_t)depth[end_node] + 2 : 0;
        a.res[q] = Res{status, last_act, end_node, last_tot, 0, n_nodes};
    }
}

// the reference's path of every search that returned one: thread per search, written at offsets[q]
__global__ __launch_bounds__(TPB) void mgreedy_path_kernel(Args a, int64_t n, const int64_t* offsets, int32_t* actions,
                                                           int32_t* totals, int64_t out_cap) {
    const int64_t q = (int64_t)blockIdx.x * TPB + threadIdx.x;
    if (q >= n) return;
    const Res r = a.res[q];
    if (r.status != ACX_BFS_EXHAUSTED && r.status != ACX_BFS_FOUND && r.status != ACX_BFS_BUDGET) return;
    if (r.end_node < 0 || r.end_node >= a.rows) return;
    const uint64_t* store = a.store + q * a.rows * a.kw;
    const uint32_t* meta = a.meta + q * a.rows;
    const int64_t d = (a.depth + q * a.rows)[r.end_node];
    const int64_t off = offsets[q];
    if (off < 0 || off + d + 2 > out_cap) return;
    actions[off] = -1;
    totals[off] = key_total(store, a.L);
    int64_t pos = off + d;
    for (int64_t i = r.end_node; i != 0 && i < a.rows && pos > off; i = meta[i] >> 4, --pos) {
        actions[pos] = (int32_t)(meta[i] & 15u);
        totals[pos] = key_total(store + i * a.kw, a.L);
    }
    actions[off + d + 1] = r.last_act;
    totals[off + d + 1] = r.last_tot;
}

struct Batch {
    int64_t n_cap = 0;
    int epoch = 0;  // the last run's epoch (0: tables all zero)
    size_t table_bytes = 0;
    Args a{};

    ~Batch() {
        void* ptrs[] = {a.store, a.meta, a.depth, a.hk, a.hid, a.table, a.res};
        for (void* p : ptrs)
            if (p) (void)hipFree(p);
    }
};

struct RunLaunch {
    Batch* S;
    hipStream_t st;
    int64_t n;
    template <int NW>
    void go() { mgreedy_kernel<NW><<<dim3((unsigned)n), dim3(GT), 0, st>>>(S->a); }
};

}  // namespace mgreedy
}  // namespace acx

using namespace acx::mgreedy;

extern "C" {

int64_t acx_mgreedy_bytes(int32_t L, int64_t max_nodes_each) {
    if (L < 1 || L > ACX_MAX_L || max_nodes_each < 1 || max_nodes_each > MAX_NODES_EACH) return ACX_E_ARG;
    const size_t kw = (size_t)acx_key_words(L), R = (size_t)rows_for(max_nodes_each);
    return (int64_t)((8 * kw + 20) * R + (size_t)buckets_for(max_nodes_each) * BUCKET * 8 + sizeof(Res));
}

void* acx_mgreedy_create(int32_t L, int64_t n_searches, int64_t max_nodes_each, int32_t cyclical) {
    if (L < 1 || L > ACX_MAX_L || n_searches < 1 || n_searches > (1ll << 24) || max_nodes_each < 1 ||
        max_nodes_each > MAX_NODES_EACH)
        return nullptr;
    Batch* S = new (std::nothrow) Batch();
    if (!S) return nullptr;
    Args& a = S->a;
    a.L = L;
    a.kw = acx_key_words(L);
    a.cyc = cyclical != 0;
    a.maxb = max_nodes_each;
    a.rows = rows_for(max_nodes_each);
    a.nb = buckets_for(max_nodes_each);
    S->n_cap = n_searches;
    const size_t n = (size_t)n_searches, R = (size_t)a.rows;
    S->table_bytes = n * a.nb * BUCKET * 8;
    bool ok = hipMalloc((void**)&a.store, n * R * a.kw * 8) == hipSuccess &&
              hipMalloc((void**)&a.meta, n * R * 4) == hipSuccess &&
              hipMalloc((void**)&a.depth, n * R * 4) == hipSuccess &&
              hipMalloc((void**)&a.hk, n * R * 8) == hipSuccess &&
              hipMalloc((void**)&a.hid, n * R * 4) == hipSuccess &&
              hipMalloc((void**)&a.table, S->table_bytes) == hipSuccess &&
              hipMalloc((void**)&a.res, n * sizeof(Res)) == hipSuccess &&
              hipMemset(a.table, 0, S->table_bytes) == hipSuccess &&
              hipMemset(a.res, 0, n * sizeof(Res)) == hipSuccess;
    if (!ok) {
        (void)hipGetLastError();
        delete S;
        return nullptr;
    }
    return S;
}

void acx_mgreedy_destroy(void* h) { delete static_cast<Batch*>(h); }

int acx_mgreedy_run(void* h, const int32_t* states, const int64_t* budgets, int64_t n, int32_t* status, int64_t* nodes,
                    int64_t* parents, int32_t* min_length, int64_t* path_len, void* stream) {
    Batch* S = static_cast<Batch*>(h);
    if (!S || !states || !budgets || !status || !nodes || !parents || !min_length || !path_len) return ACX_E_ARG;
    if (n < 0 || n > S->n_cap) return ACX_E_ARG;
    if (n == 0) return ACX_OK;
    hipStream_t st = (hipStream_t)stream;
    Args& a = S->a;
    if (!acx::visited::next_epoch(S->epoch, a.table, S->table_bytes, st, a.ep)) return ACX_E_LAUNCH;
    a.states = states;
    a.budgets = budgets;
    a.status = status;
    a.nodes = nodes;
    a.parents = parents;
    a.min_length = min_length;
    a.path_len = path_len;
    RunLaunch rl{S, st, n};
    by_nw(a.L, rl);
    return hipGetLastError() == hipSuccess ? ACX_OK : ACX_E_LAUNCH;
}

int acx_mgreedy_paths(void* h, int64_t n, const int64_t* offsets, int32_t* actions, int32_t* totals, int64_t cap,
                      void* stream) {
    Batch* S = static_cast<Batch*>(h);
    if (!S || !offsets || !actions || !totals || n < 0 || n > S->n_cap || cap < 0) return ACX_E_ARG;
    if (n == 0) return ACX_OK;
    mgreedy_path_kernel<<<dim3((unsigned)((n + TPB - 1) / TPB)), dim3(TPB), 0, (hipStream_t)stream>>>(
        S->a, n, offsets, actions, totals, cap);
    return hipGetLastError() == hipSuccess ? ACX_OK : ACX_E_LAUNCH;
}

}  // extern "C"
