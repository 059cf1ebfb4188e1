// acx_mbfs.hip -- breadth-first search over a batch of presentations in one launch: one workgroup
// of 256 threads owns one search from its root to its verdict.  The searches are independent, so
// no workgroup ever waits on another; inside a workgroup the phases of a round are separated by
// __syncthreads() alone.
//
// Reference: ac_solver/search/breadth_first.py:15-97, with the semantics acx_bfs.hip states in its
// header comment (FIFO parents, actions 0..11, success tested before the visited test, the budget
// tested after each parent, a raising move ends the search) -- the results equal acx_bfs_run's.
//
// A search's memory is a private slice of each of the handle's arrays:
//   store  (B, kw) uint64   node keys in discovery order = FIFO order (node 0 is the root), so the
//                           queue is the store itself and `head` is the next parent's index;
//   meta   (B) uint32       parent index << 4 | action of each node (the path reader walks it);
//   table  (nb * 8) uint64  the visited set (acx_visited.h: buckets of 8 entries), nb buckets with
//                           8 nb >= 2 (B + 11 + 768) -- load <= 1/2 -- chosen by range reduction
//                           of the hash (no power-of-two rounding);
//   scratch (768, kw) uint64  only for L > 64: the round's child keys (below).
// B = max_nodes_each.  Bytes per search (acx_mbfs_bytes):
//   8 kw B + 4 B + 64 ceil((B + 779) / 4) + 32 [+ 6144 kw when L > 64],   kw = acx_key_words(L).
//
// A round takes the next P <= 64 parents (nodes head .. head + P) and runs, with a barrier between:
//   expand  lane = parent, wave w makes actions 3w..3w+2 (child_of, acx_bfs_common.h); the
//           768 child keys go to LDS in sequential order s = 12 p + a (L <= 64: at most 30 KiB;
//           above that 54 KiB of LDS would halve the workgroups per CU, so they go to the
//           search's scratch in HBM); first success and first raising child by LDS atomicMin;
//   insert  thread per child s below the first success / raising child: visited::insert; a code
//           below n (the nodes before the round) names a stored node, a code n + s a child of this
//           round, so the full key is compared in the store or in the round's keys.  The first
//           occurrence holds the entry, the child it replaced is told (`lost`).  A probe that has
//           walked all nb buckets sets the overflow status;
//   decide  wave 0: survivors per parent, their prefix sum, the first parent after which
//           len(tree_nodes) >= max_nodes, and the reference's verdict for the round
//           (chunk_verdict, acx_bfs_verdict.h: raising child / success / budget cut, the earliest
//           in sequential order; otherwise the next round, or queue exhaustion);
//   commit  (no verdict yet) the survivors' keys are appended in (parent, action) order with
//           their meta word, and each survivor's table entry is rewritten from its round code to
//           its node index; the running minimum takes the child totals up to the ending event.
// A round with a verdict appends nothing, so a search holds fewer than max_nodes nodes and the
// store needs B rows.  Every loop is bounded: rounds by max_nodes (each expands >= 1 of fewer than
// max_nodes nodes), probes by nb, the path walks by the node count.
//
// Table reads are workgroup-scope atomic loads and the rewrite an atomic store: a round code means
// another node a round later, so no stale value may be read (node codes in acx_bfs.hip are
// permanent, which is why its plain bucket loads are safe there).  Nothing needs a wider scope:
// a search's memory is touched by its own workgroup alone.  A handle is reusable: entries
// carry the run's epoch (visited::next_epoch).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <new>

#include "acx.h"
#include "acx_moves.h"

#include "acx_bfs_common.h"
#include "acx_bfs_verdict.h"
#include "acx_visited.h"

namespace acx {
namespace mbfs {

using namespace acx::bfs;
using visited::BUCKET;

constexpr int RP = 64;          // parents per round
constexpr int RC = 12 * RP;     // children per round
constexpr int64_t MAX_NODES_EACH = 1ll << 24;
constexpr int RKW = ACX_MAX_L / 16 + 2;  // words of the largest key, rounded up

// what the path reader needs of a finished search
struct Res {
    int32_t status, succ_act;
    int64_t succ_node;  // the parent of the success child
    int64_t nodes, pad;
};

struct Args {
    const int32_t* states;   // (n, 2L)
    const int64_t* budgets;  // (n)
    uint64_t* store;
    uint32_t* meta;
    uint64_t* table;
    uint64_t* scratch;
    Res* res;
    int32_t* status;
    int64_t* nodes;
    int64_t* parents;
    int32_t* min_length;
    int64_t* path_len;
    int64_t cap;  // B: node rows per search
    uint32_t nb;  // buckets per search
    uint64_t ep;  // this run's epoch, shifted (visited::next_epoch)
    int L, kw, cyc;
};

// a table entry as the workgroup last wrote it: only this workgroup touches its search's table, so
// workgroup scope is the whole of it (an agent-scope load or fence would go through, or write back,
// the L2 on every round for nobody's benefit)
__device__ __forceinline__ uint64_t wload(const uint64_t* p) {
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}

// one search's visited set: nb buckets, the first by range reduction of the hash; a bucket line
// is read entry by entry with wload (a round code means another node a round later, so no stale
// value may be read)
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

// edges from the root to node `v` of a search (meta: parent index << 4 | action), at most cap
__device__ __forceinline__ int64_t path_depth(const uint32_t* meta, int64_t v, int64_t cap) {
    int64_t d = 0;
    for (int64_t i = v; i != 0 && d < cap; i = meta[i] >> 4) ++d;
    return d;
}

static inline uint32_t buckets_for(int64_t cap) { return (uint32_t)((2 * (cap + 11 + RC) + BUCKET - 1) / BUCKET); }

template <int NW>
__global__ __launch_bounds__(TPB) void mbfs_kernel(Args a) {
    constexpr bool LDS_KEYS = NW <= 4;
    __shared__ uint64_t kl[LDS_KEYS ? RC * (NW + 1) : 1];
    __shared__ uint64_t rk[RKW];
    __shared__ uint32_t slot[RC];    // table index of the entry a child holds
    __shared__ uint16_t ctot[RC];    // child total, 0xffff: the move raised (or no such child)
    __shared__ uint8_t cand[RC];     // the child holds its state's entry after its own probe
    __shared__ uint8_t lost[RC];     // an earlier child of the round took that entry
    __shared__ uint32_t pmask[RP], pexcl[RP];
    __shared__ uint32_t s_succ, s_err, s_min, s_over, s_bad;
    __shared__ uint32_t s_n[2];
    __shared__ uint32_t s_dec[4];    // verdict kind, children looked at, last parent, new nodes

    const int tid = threadIdx.x, lane = tid & (WAVE - 1), wid = tid / WAVE;
    const int64_t q = blockIdx.x;
    const int L = a.L, kw = a.kw;
    const bool cyc = a.cyc != 0;
    uint64_t* store = a.store + q * a.cap * kw;
    uint32_t* meta = a.meta + q * a.cap;
    uint64_t* table = a.table + q * (int64_t)a.nb * BUCKET;
    uint64_t* ck;
    if constexpr (LDS_KEYS) ck = kl;
    else ck = a.scratch + q * (int64_t)RC * kw;

    // the root: packed by the block (acx_key.h format), checked against the packed domain
    if (tid < RKW) rk[tid] = 0;
    if (tid < 2) s_n[tid] = 0;
    if (tid == 0) s_bad = s_over = 0;
    __syncthreads();
    if (tid < 2 * L) {
        const int32_t* st = a.states + q * 2 * L;
        const int32_t v = st[tid];
        const int h = tid >= L, i = tid - h * L;
        bool bad = v < -2 || v > 2;
        if (v == 0) {
            bad = i + 1 < L && st[tid + 1] != 0;  // zeros only as right padding
        } else if (!bad) {
            const int bit = 2 * tid;
            atomicOr((unsigned long long*)&rk[bit >> 6], (unsigned long long)(key_code(v) << (bit & 63)));
            atomicAdd(&s_n[h], 1u);
        }
        if (bad) s_bad = 1;
    }
    __syncthreads();
    int64_t max_nodes = a.budgets[q];
    if (max_nodes < 1) max_nodes = 1;  // the reference still expands the root once
    const uint32_t total0 = s_n[0] + s_n[1];
    const bool dom = s_bad || s_n[0] == 0 || s_n[1] == 0;
    if (dom || max_nodes > a.cap) {
        if (tid == 0) {
            const int32_t st = dom ? ACX_MBFS_DOMAIN : ACX_MBFS_OVERFLOW;
            a.status[q] = st;
            a.nodes[q] = 0;
            a.parents[q] = 0;
            a.min_length[q] = 0;
            a.path_len[q] = 0;
            a.res[q] = Res{st, 0, 0, 0, 0};
        }
        return;
    }
    if (tid == 0) {
        const uint64_t lens = (uint64_t)s_n[0] | ((uint64_t)s_n[1] << 8);
        const int bit = 4 * L;
        rk[bit / 64] |= lens << (bit % 64);
        if (bit % 64 > 48 && bit / 64 + 1 < kw) rk[bit / 64 + 1] |= lens >> (64 - bit % 64);
    }
    __syncthreads();
    if (tid < kw) store[tid] = rk[tid];
    if (tid == 0) {
        const Key<NW + 1> key = kload<NW + 1>(rk, kw);
        const uint64_t h = khash<NW + 1>(key, kw);
        const Buckets tb{table, a.nb};
        __hip_atomic_store(tb.bucket(tb.first(h)), visited::entry(a.ep, 0, visited::fp_of(h)), __ATOMIC_RELAXED,
                           __HIP_MEMORY_SCOPE_WORKGROUP);  // node 0
        meta[0] = 0;
    }
    __syncthreads();

    int64_t head = 0, n_nodes = 1, parents = 0, succ_node = 0;
    int32_t status = ACX_MBFS_OVERFLOW, succ_act = 0;
    uint32_t running = total0;

    for (int64_t round = 0; round <= max_nodes; ++round) {
        const int P = (int)(n_nodes - head < RP ? n_nodes - head : RP);
        const int nch = 12 * P;
        for (int c = tid; c < RC; c += TPB) {
            cand[c] = 0;
            lost[c] = 0;
            ctot[c] = 0xffffu;
        }
        if (tid == 0) s_succ = s_err = NONE;
        __syncthreads();

        // expand
        {
            uint32_t succ = NONE, err = NONE;
            if (lane < P) {
                PresRegs<NW> pr;
                load_key<NW>(store + (head + lane) * kw, kw, L, pr);
                const bool clean = is_clean<NW>(pr.w0, pr.n0, pr.w1, pr.n1, cyc);
#pragma unroll 1
                for (int j = 0; j < 3; ++j) {
                    const int act = wid * 3 + j;
                    const uint32_t s = (uint32_t)lane * 12u + (uint32_t)act;
                    PresRegs<NW> c;
                    const int e = child_of<NW>(pr, clean, act, L, cyc, c);
                    if (e != ACX_ERR_NONE) {
                        err = min(err, s);
                    } else {
                        const uint32_t tot = (uint32_t)(c.n0 + c.n1);
                        if (tot == 2) succ = min(succ, s);
                        ctot[s] = (uint16_t)tot;
                    }
                    uint64_t key[NW + 1];
                    make_key<NW>(L, c, key);
#pragma unroll
                    for (int k = 0; k < NW + 1; ++k)
                        if (k < kw) ck[s * kw + k] = key[k];
                }
            }
            succ = wave_min(succ);
            err = wave_min(err);
            if (lane == 0) {
                if (succ != NONE) atomicMin(&s_succ, succ);
                if (err != NONE) atomicMin(&s_err, err);
            }
        }
        __syncthreads();

        // insert: the success / raising child ends the search, later children are not looked at
        const uint32_t end0 = min(s_succ, s_err);
        const uint64_t NB = (uint64_t)n_nodes;
        for (int c = tid; c < nch; c += TPB) {
            if ((uint32_t)c >= end0) continue;
            const uint64_t code = NB + (uint64_t)c;
            const Key<NW + 1> key = kload<NW + 1>(ck + c * kw, kw);
            const visited::Outcome ins = visited::insert(
                Buckets{table, a.nb}, a.ep, code, khash<NW + 1>(key, kw),
                [&](uint64_t vc) {
                    return vc < NB ? keq<NW + 1>(store + vc * kw, key, kw) : keq<NW + 1>(ck + (vc - NB) * kw, key, kw);
                },
                [&](uint32_t sl, uint64_t displaced) {  // a later child of the round that held it learns it lost
                    slot[c] = sl;
                    const uint64_t lc = displaced - NB;
                    if (displaced != visited::NO_CODE && lc < (uint64_t)RC) lost[lc] = 1;
                });
            if (ins == visited::FULL) s_over = 1;
            cand[c] = ins == visited::HELD;
        }
        __syncthreads();
        if (s_over) break;  // (uniform) cannot happen at load <= 1/2

        // decide
        if (wid == 0) {
            uint32_t m = 0;
            if (lane < P) {
#pragma unroll
                for (int act = 0; act < 12; ++act) {
                    const int c = lane * 12 + act;
                    if (cand[c] && !lost[c]) m |= 1u << act;
                }
            }
            const uint32_t cnt = __popc(m);
            const uint32_t x = wave_incl_sum(cnt, lane);
            pmask[lane] = m;
            pexcl[lane] = x - cnt;
            const uint32_t total = __shfl(x, WAVE - 1, WAVE);
            // the first parent after which len(tree_nodes) >= max_nodes
            const unsigned long long cutb = __ballot(lane < P && n_nodes + (int64_t)x >= max_nodes);
            const uint32_t cutp = cutb ? (uint32_t)__builtin_ctzll(cutb) : NONE;
            const uint32_t at_cut = __shfl(x, cutb ? (int)cutp : 0, WAVE);
            const Verdict v = chunk_verdict(s_succ, s_err, cutp, (uint32_t)P);
            if (lane == 0) {
                s_dec[0] = (uint32_t)v.kind;
                s_dec[1] = v.looked;
                s_dec[2] = v.last_p;
                s_dec[3] = v.kind == ACX_BFS_BUDGET ? at_cut : total;
                s_min = NONE;
            }
        }
        __syncthreads();
        const uint32_t kind = s_dec[0], s_end = s_dec[1], last_p = s_dec[2], newn = s_dec[3];

        // commit
        if (kind == 0) {
            for (int c = tid; c < nch; c += TPB) {
                const int p = c / 12, act = c - 12 * p;
                const uint32_t m = pmask[p];
                if (!((m >> act) & 1u)) continue;
                const int64_t pos = n_nodes + pexcl[p] + __popc(m & ((1u << act) - 1u));
                if (pos >= a.cap) continue;  // (never: a round without a verdict ends below max_nodes)
                for (int k = 0; k < kw; ++k) store[pos * kw + k] = ck[c * kw + k];
                meta[pos] = ((uint32_t)(head + p) << 4) | (uint32_t)act;
                uint64_t* ent = table + slot[c];
                const uint64_t v = wload(ent);
                __hip_atomic_store(ent, visited::entry_recode(v, (uint64_t)pos), __ATOMIC_RELAXED,
                                   __HIP_MEMORY_SCOPE_WORKGROUP);
            }
        }
        {
            uint32_t m = NONE;
            for (int c = tid; c < nch; c += TPB)
                if ((uint32_t)c < s_end) m = min(m, (uint32_t)ctot[c]);
            m = wave_min(m);
            if (lane == 0 && m != NONE) atomicMin(&s_min, m);
        }
        __syncthreads();
        running = min(running, s_min);
        if (kind != 0) {
            parents += (int64_t)last_p + 1;
            n_nodes += newn;
            status = (int32_t)kind;
            if (kind == ACX_BFS_FOUND) {
                succ_node = head + (s_end - 1) / 12;
                succ_act = (int32_t)((s_end - 1) % 12);
            }
            break;
        }
        parents += P;
        n_nodes += newn;
        head += P;
        if (head >= n_nodes) {  // the queue ran dry: (False, None)
            status = ACX_BFS_EXHAUSTED;
            break;
        }
    }

    if (tid == 0) {
        // [(-1, total0)] + the edges to the parent + (action, 2)
        const int64_t plen = status == ACX_BFS_FOUND ? path_depth(meta, succ_node, a.cap) + 2 : 0;
        a.status[q] = status;
        a.nodes[q] = status < 0 ? 0 : n_nodes;
        a.parents[q] = parents;
        a.min_length[q] = (int32_t)running;
        a.path_len[q] = plen;
        a.res[q] = Res{status, succ_act, succ_node, n_nodes, 0};
    }
}

// the reference's path of every found search: thread per search, written at offsets[q]
__global__ __launch_bounds__(TPB) void mbfs_path_kernel(Args a, int64_t n, const int64_t* offsets, int32_t* actions,
                                                        int32_t* totals, int64_t out_cap) {
    const int64_t q = (int64_t)blockIdx.x * TPB + threadIdx.x;
    if (q >= n) return;
    const Res r = a.res[q];
    if (r.status != ACX_BFS_FOUND) return;
    const uint64_t* store = a.store + q * a.cap * a.kw;
    const uint32_t* meta = a.meta + q * a.cap;
    const int64_t d = path_depth(meta, r.succ_node, a.cap);
    const int64_t off = offsets[q];
    if (off < 0 || off + d + 2 > out_cap) return;
    actions[off] = -1;
    totals[off] = key_total(store, a.L);
    int64_t pos = off + d;
    for (int64_t i = r.succ_node; i != 0 && pos > off; i = meta[i] >> 4, --pos) {
        actions[pos] = (int32_t)(meta[i] & 15u);
        totals[pos] = key_total(store + i * a.kw, a.L);
    }
    actions[off + d + 1] = r.succ_act;
    totals[off + d + 1] = 2;
}

struct Batch {
    int64_t n_cap = 0;
    int epoch = 0;  // the last run's epoch (0: tables all zero)
    size_t table_bytes = 0;
    Args a{};

    ~Batch() {
        void* ptrs[] = {a.store, a.meta, a.table, a.scratch, a.res};
        for (void* p : ptrs)
            if (p) (void)hipFree(p);
    }
};

struct RunLaunch {
    Batch* S;
    hipStream_t st;
    int64_t n;
    template <int NW>
    void go() { mbfs_kernel<NW><<<dim3((unsigned)n), dim3(TPB), 0, st>>>(S->a); }
};

static size_t scratch_bytes(int L, int kw) { return L > 64 ? (size_t)RC * kw * 8 : 0; }

}  // namespace mbfs
}  // namespace acx

using namespace acx::mbfs;

extern "C" {

int64_t acx_mbfs_bytes(int32_t L, int64_t max_nodes_each) {
    if (L < 1 || L > ACX_MAX_L || max_nodes_each < 1 || max_nodes_each > MAX_NODES_EACH) return ACX_E_ARG;
    const int kw = acx_key_words(L);
    return (int64_t)(8 * (size_t)kw * max_nodes_each + 4 * (size_t)max_nodes_each +
                     (size_t)buckets_for(max_nodes_each) * BUCKET * 8 + sizeof(Res) + scratch_bytes(L, kw));
}

void* acx_mbfs_create(int32_t L, int64_t n_searches, int64_t max_nodes_each, int32_t cyclical) {
    if (L < 1 || L > ACX_MAX_L || n_searches < 1 || n_searches > (1ll << 24) || max_nodes_each < 1 ||
        max_nodes_each > MAX_NODES_EACH)
        return nullptr;
    Batch* S = new (std::nothrow) Batch();
    if (!S) return nullptr;
    Args& a = S->a;
    a.L = L;
    a.kw = acx_key_words(L);
    a.cyc = cyclical != 0;
    a.cap = max_nodes_each;
    a.nb = buckets_for(max_nodes_each);
    S->n_cap = n_searches;
    const size_t n = (size_t)n_searches;
    S->table_bytes = n * a.nb * BUCKET * 8;
    const size_t sb = scratch_bytes(L, a.kw);
    bool ok = hipMalloc((void**)&a.store, n * (size_t)a.cap * a.kw * 8) == hipSuccess &&
              hipMalloc((void**)&a.meta, n * (size_t)a.cap * 4) == hipSuccess &&
              hipMalloc((void**)&a.table, S->table_bytes) == hipSuccess &&
              hipMalloc((void**)&a.res, n * sizeof(Res)) == hipSuccess &&
              (sb == 0 || hipMalloc((void**)&a.scratch, n * sb) == hipSuccess) &&
              hipMemset(a.table, 0, S->table_bytes) == hipSuccess &&
              hipMemset(a.res, 0, n * sizeof(Res)) == hipSuccess;
    if (!ok) {
        (void)hipGetLastError();
        delete S;
        return nullptr;
    }
    return S;
}

void acx_mbfs_destroy(void* h) { delete static_cast<Batch*>(h); }

int acx_mbfs_run(void* h, const int32_t* states, const int64_t* budgets, int64_t n, int32_t* status, int64_t* nodes,
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

int acx_mbfs_paths(void* h, int64_t n, const int64_t* offsets, int32_t* actions, int32_t* totals, int64_t cap,
                   void* stream) {
    Batch* S = static_cast<Batch*>(h);
    if (!S || !offsets || !actions || !totals || n < 0 || n > S->n_cap || cap < 0) return ACX_E_ARG;
    if (n == 0) return ACX_OK;
    mbfs_path_kernel<<<dim3((unsigned)((n + TPB - 1) / TPB)), dim3(TPB), 0, (hipStream_t)stream>>>(S->a, n, offsets,
                                                                                                 actions, totals, cap);
    return hipGetLastError() == hipSuccess ? ACX_OK : ACX_E_LAUNCH;
}

}  // extern "C"
