// acx_batch.h -- the frame of the batched engines (acx_mbfs.hip, acx_mgreedy.hip, acx_beam.hip): one
// workgroup owns one search, from its root to its verdict, on a private slice of each of the
// handle's arrays.  An engine adds what happens between the root and the verdict (mbfs: rounds of
// 64 parents, acx_round.h; beam: the same rounds over its beam, a step per launch with the caller's
// scorer between; mgreedy: a pop off its heap) and a description of itself (`Engine`, below);
// everything here is the same for all three:
//   device  the table view (workgroup-scope reads: only the owning workgroup touches a search's
//           memory, and a round / pop code means another child a round later, so no stale value
//           may be read), the root (packed, checked, refused or stored as node 0), the rewrite of a
//           survivor's table entry, the result record, the path reader;
//   host    the handle behind the C functions of an engine (include/acx.h: _bytes, _create, _run
//           -- beam: its step calls instead --, _paths, _destroy), sized, allocated and freed from
//           the engine's one list of arrays.
// A handle is reusable: table entries carry the run's epoch (visited::next_epoch), and every other
// array is written before it is read.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <new>

#include "acx.h"
#include "acx_bfs_common.h"
#include "acx_visited.h"

namespace acx {
namespace batch {

using namespace acx::bfs;
using visited::BUCKET;

constexpr int64_t MAX_NODES_EACH = 1ll << 24;
constexpr int64_t MAX_SEARCHES = 1ll << 24;
constexpr int RKW = ACX_MAX_L / 16 + 2;  // words of the largest key, rounded up

// what the path reader needs of a finished search: the path is the one to `end_node` (the success
// child's parent; greedy without a success: the last popped node) plus (last_act, last_tot)
struct Res {
    int32_t status, last_act;
    int64_t end_node;
    int32_t last_tot, pad;
    int64_t nodes;
};

// what every engine's kernel is given; an engine's own arrays follow in its derived struct.  The
// order is the one the kernels' registers were measured with (with depth before table and maxb
// before rows, mbfs_kernel<2> took 94 VGPRs instead of 93).
struct Args {
    const int32_t* states;   // (n, 2L)
    const int64_t* budgets;  // (n)
    uint64_t* store;         // (rows, kw) node keys, node 0 the root
    uint32_t* meta;          // (rows) parent index << 4 | action
    uint64_t* table;         // (nb * 8) the visited set
    uint32_t* depth;         // (rows) path length of each node, or null: the path reader walks meta
    Res* res;
    int32_t* status;
    int64_t* nodes;
    int64_t* parents;
    int32_t* min_length;
    int64_t* path_len;
    int64_t rows;  // node rows per search
    uint32_t nb;   // buckets per search
    uint64_t ep;   // this run's epoch, shifted (visited::next_epoch)
    int L, kw, cyc;
    int64_t maxb;  // B: the largest budget a search may have
};

// a table entry as the workgroup last wrote it: only this workgroup touches its search's table, so
// workgroup scope is the whole of it (an agent-scope load or fence would go through, or write back,
// the L2 on every round for nobody's benefit)
__device__ __forceinline__ uint64_t wload(const uint64_t* p) {
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}

// one search's visited set: nb buckets, the first by range reduction of the hash; a bucket line
// is read entry by entry with wload
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

// does a search that ended with `status` return a path (with_path: bit s set for status s)
__host__ __device__ __forceinline__ bool has_path(uint32_t with_path, int32_t status) {
    return status >= 0 && status < 32 && ((with_path >> status) & 1u);
}

// the record of search q for the path reader and its five outputs (one thread).  The record goes
// first: with it last, the greedy batch of 1,190 measured 0.3 ms slower than before this routine
// was shared (52.3 against 52.0 ms, three sessions), with it first as fast as before.
__device__ __forceinline__ void write_result(const Args& a, int64_t q, const Res& r, int64_t parents,
                                             uint32_t min_length, int64_t path_len) {
    a.res[q] = r;
    a.status[q] = r.status;
    a.nodes[q] = r.status < 0 ? 0 : r.nodes;
    a.parents[q] = parents;
    a.min_length[q] = (int32_t)min_length;
    a.path_len[q] = path_len;
}

struct Root {
    bool refused;         // the search has its status and all-zero outputs: return
    int64_t max_nodes;    // its budget, at least 1
    uint32_t total0;      // the root's total length
    const uint64_t* key;  // the packed root (LDS)
};

// The root of search q, by a workgroup of THREADS threads: the (2L) int32 row is packed (acx_key.h
// format) and checked against the packed domain -- letters in +-1, +-2, zeros only as right
// padding, no empty relator; a row outside it gets ACX_MBFS_DOMAIN, a budget above the handle's
// ACX_MBFS_OVERFLOW, and neither is searched.  Otherwise node 0 is in the store, the table and
// meta once the caller's next barrier has passed.
template <int THREADS, int NW>
__device__ __forceinline__ Root root_setup(const Args& a, int64_t q, uint64_t* store, uint32_t* meta, uint64_t* table) {
    __shared__ uint64_t rk[RKW];
    __shared__ uint32_t s_n[2], s_bad;
    static_assert(THREADS >= RKW, "one thread per key word");
    const int tid = threadIdx.x, L = a.L, kw = a.kw;
    if (tid < RKW) rk[tid] = 0;
    if (tid < 2) s_n[tid] = 0;
    if (tid == 0) s_bad = 0;
    __syncthreads();
    const int32_t* st = a.states + q * 2 * L;
    for (int t = tid; t < 2 * L; t += THREADS) {  // (once with 256 threads: 2 ACX_MAX_L = 256)
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
    __syncthreads();
    int64_t max_nodes = a.budgets[q];
    if (max_nodes < 1) max_nodes = 1;  // the reference still expands the root once
    const uint32_t total0 = s_n[0] + s_n[1];
    const bool dom = s_bad || s_n[0] == 0 || s_n[1] == 0;
    if (dom || max_nodes > a.maxb) {
        if (tid == 0) write_result(a, q, Res{dom ? ACX_MBFS_DOMAIN : ACX_MBFS_OVERFLOW, 0, 0, 0, 0, 0}, 0, 0, 0);
        return Root{true, max_nodes, total0, rk};
    }
    if (tid == 0) {  // the length field at bit 4L may straddle a word
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
    return Root{false, max_nodes, total0, rk};
}

// a survivor's entry, from its round code to its node index
__device__ __forceinline__ void recode_entry(uint64_t* table, uint32_t slot, uint64_t pos) {
    uint64_t* ent = table + slot;
    __hip_atomic_store(ent, visited::entry_recode(wload(ent), pos), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}

// edges from the root to node `v` of a search (meta: parent index << 4 | action), at most cap
__device__ __forceinline__ int64_t path_depth(const uint32_t* meta, int64_t v, int64_t cap) {
    int64_t d = 0;
    for (int64_t i = v; i != 0 && d < cap; i = meta[i] >> 4) ++d;
    return d;
}

// The reference's path of every search whose status is in `with_path` (bit s: status s): thread
// per search, written at offsets[q]: [(-1, total0)] (root_entry: the searches of breadth_first.py
// and greedy.py start their paths with it, value_guided_search.py's do not) + the edges to
// end_node + (last_act, last_tot).  A node's depth is read from a.depth, or, without one, counted
// along meta.
static __global__ __launch_bounds__(TPB) void path_kernel(Args a, uint32_t with_path, bool root_entry, int64_t n,
                                                          const int64_t* offsets, int32_t* actions, int32_t* totals,
                                                          int64_t out_cap) {
    const int64_t q = (int64_t)blockIdx.x * TPB + threadIdx.x;
    if (q >= n) return;
    const Res r = a.res[q];
    if (!has_path(with_path, r.status)) return;
    if (r.end_node < 0 || r.end_node >= a.rows) return;
    const uint64_t* store = a.store + q * a.rows * a.kw;
    const uint32_t* meta = a.meta + q * a.rows;
    const int64_t d = a.depth ? (int64_t)(a.depth + q * a.rows)[r.end_node] : path_depth(meta, r.end_node, a.rows);
    int64_t off = offsets[q];
    if (off < 0 || off + d + 1 + root_entry > out_cap) return;
    if (root_entry) {
        actions[off] = -1;
        totals[off] = key_total(store, a.L);
        ++off;
    }
    int64_t pos = off + d - 1;
    for (int64_t i = r.end_node; i != 0 && i < a.rows && pos >= off; i = meta[i] >> 4, --pos) {
        actions[pos] = (int32_t)(meta[i] & 15u);
        totals[pos] = key_total(store + i * a.kw, a.L);
    }
    actions[off + d] = r.last_act;
    totals[off + d] = r.last_tot;
}

// ---------------------------------------------------------------------------------------------
// host: the handle of an engine E, which states
//   Args                     its kernel's arguments, derived from batch::Args;
//   WITH_PATH, ROOT_ENTRY    the statuses whose searches return a path (bit s: status s), and
//                            whether a path starts with the root's (-1, total0);
//   rows_for(B), buckets_for(B)   node rows and table buckets per search at budgets up to B;
//   arrays(a, f)             its arrays, once: f(pointer in a, bytes per search, zeroed at create)
//                            for each -- _bytes, _create and the destructor all go through it;
//   launch<NW>(a, n, st)     its kernel over n searches, for run() (beam, whose step is several
//                            calls, has none and starts its kernels itself after new_epoch()).
// An engine with shape parameters of its own (beam: max_width) sets them in its Args, calls
// shape() and then bytes_of() / create_from(); the others call bytes() / create().
// ---------------------------------------------------------------------------------------------
template <class E>
struct Handle {
    int64_t n_cap = 0;
    int epoch = 0;  // the last run's epoch (0: tables all zero)
    typename E::Args a{};
    void* cache = nullptr;       // the scored engines': an attached solution cache (acx_cache.h), not owned,
    void* cache_hits = nullptr;  // and the attachment's hit records, one per search

    ~Handle() {
        if (cache_hits) (void)hipFree(cache_hits);
        E::arrays(a, [](auto*& p, size_t, bool) {
            if (p) (void)hipFree(p);
        });
    }
};

// the shape of a handle's slices; false: L or B out of range
template <class E>
static bool shape(typename E::Args& a, int32_t L, int64_t B, int32_t cyclical) {
    if (L < 1 || L > ACX_MAX_L || B < 1 || B > MAX_NODES_EACH) return false;
    a.L = L;
    a.kw = acx_key_words(L);
    a.cyc = cyclical != 0;
    a.maxb = B;
    a.rows = E::rows_for(B);
    a.nb = E::buckets_for(B);
    return true;
}

// bytes per search of a shaped handle
template <class E>
static int64_t bytes_of(typename E::Args a) {
    size_t sum = 0;
    E::arrays(a, [&](auto*&, size_t b, bool) { sum += b; });
    return (int64_t)sum;
}

template <class E>
static int64_t bytes(int32_t L, int64_t B) {
    typename E::Args a{};
    return shape<E>(a, L, B, 0) ? bytes_of<E>(a) : ACX_E_ARG;
}

// a handle of shape `a` for n_searches searches, or null
template <class E>
static void* create_from(const typename E::Args& a, int64_t n_searches) {
    if (n_searches < 1 || n_searches > MAX_SEARCHES) return nullptr;
    Handle<E>* S = new (std::nothrow) Handle<E>();
    if (!S) return nullptr;
    S->a = a;
    S->n_cap = n_searches;
    const size_t n = (size_t)n_searches;
    bool ok = true;
    E::arrays(S->a, [&](auto*& p, size_t b, bool zero) {
        ok = ok && (b == 0 || (hipMalloc((void**)&p, n * b) == hipSuccess &&
                               (!zero || hipMemset(p, 0, n * b) == hipSuccess)));
    });
    if (!ok) {
        (void)hipGetLastError();
        delete S;
        return nullptr;
    }
    return S;
}

template <class E>
static void* create(int32_t L, int64_t n_searches, int64_t B, int32_t cyclical) {
    typename E::Args a{};
    return shape<E>(a, L, B, cyclical) ? create_from<E>(a, n_searches) : nullptr;
}

// a run's epoch for the handle's tables (visited::next_epoch); false: the launch failed
template <class E>
static bool new_epoch(Handle<E>* S, hipStream_t st) {
    return visited::next_epoch(S->epoch, S->a.table, (size_t)S->n_cap * S->a.nb * BUCKET * 8, st, S->a.ep);
}

template <class E>
static int run(void* h, const int32_t* states, const int64_t* budgets, int64_t n, int32_t* status, int64_t* nodes,
               int64_t* parents, int32_t* min_length, int64_t* path_len, void* stream) {
    Handle<E>* S = static_cast<Handle<E>*>(h);
    if (!S || !states || !budgets || !status || !nodes || !parents || !min_length || !path_len) return ACX_E_ARG;
    if (n < 0 || n > S->n_cap) return ACX_E_ARG;
    if (n == 0) return ACX_OK;
    hipStream_t st = (hipStream_t)stream;
    typename E::Args& a = S->a;
    if (!new_epoch(S, st)) return ACX_E_LAUNCH;
    a.states = states;
    a.budgets = budgets;
    a.status = status;
    a.nodes = nodes;
    a.parents = parents;
    a.min_length = min_length;
    a.path_len = path_len;
    by_nw(a.L, [&](auto nw) { E::template launch<decltype(nw)::value>(a, n, st); });
    return hipGetLastError() == hipSuccess ? ACX_OK : ACX_E_LAUNCH;
}

template <class E>
static int paths(void* h, int64_t n, const int64_t* offsets, int32_t* actions, int32_t* totals, int64_t cap,
                 void* stream) {
    Handle<E>* S = static_cast<Handle<E>*>(h);
    if (!S || !offsets || !actions || !totals || n < 0 || n > S->n_cap || cap < 0) return ACX_E_ARG;
    if (n == 0) return ACX_OK;
    path_kernel<<<dim3((unsigned)((n + TPB - 1) / TPB)), dim3(TPB), 0, (hipStream_t)stream>>>(
        S->a, E::WITH_PATH, E::ROOT_ENTRY, n, offsets, actions, totals, cap);
    return hipGetLastError() == hipSuccess ? ACX_OK : ACX_E_LAUNCH;
}

template <class E>
static void destroy(void* h) {
    delete static_cast<Handle<E>*>(h);
}

}  // namespace batch
}  // namespace acx
