// acx_greedy.hip -- greedy_search (ac_solver/search/greedy.py:15-121) with the visited set on the
// device and the expansion rounds driven from C++.
//
// The reference pops the smallest (total, path length, state tuple) node, expands it with 12
// ACMove calls, tests each child (min length, success = total 2) and pushes the unseen ones.  The
// pop order is inherently sequential; what moves to the GPU is everything around it:
//   * expansion -- every round, the smallest frontier nodes not yet expanded (a second heap of
//     the unexpanded nodes) are expanded speculatively in one launch, lane per (parent, action),
//     from their packed keys; each child's key hash is computed there too;
//   * the visited set -- the keys of all committed nodes live in HBM with a bucketed hash table
//     (as in the device BFS); the expansion kernel probes it, so every child that is already a
//     node (as of that round) comes back marked with the node's id and the host never looks it
//     up.  Nodes the host appends are committed to the device table by the next round's launch,
//     beside its expansion (one launch per round: the expansion trusts only the entries of
//     earlier launches, and the host checks the children against the nodes committed with it).
// The host replays the reference's order exactly: pops while the frontier's top has cached
// children; a child the device did not know is checked only against the nodes appended since
// its round (the in-flight conflicts), kept in a host table of the last 2^16..2^17 appended
// nodes (two generations of tagged entries); children cached before the last 2^16 appends are
// retired and their parent re-expanded with a later batch, which bounds that table.
// The key format is acx_key.h; the priority key, the heaps, the in-flight table (Recent), the
// per-child replay and the result readers are acx_frontier.h, shared with acx_search.cpp.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <chrono>
#include <new>
#include <vector>

#include "acx.h"
#include "acx_moves.h"

#include "acx_bfs_common.h"
#include "acx_frontier.h"
#include "acx_visited.h"

namespace acx {
namespace greedy {

using bfs::fmix64;
using bfs::Key;
using bfs::keq;
using bfs::khash;
using bfs::kload;
using visited::BUCKET;  // the table shares acx_visited.h's bucket and fingerprint format; entries
using visited::FP_MASK;  // are (id + 1) << 24 | fp with no epoch, probed and committed below

constexpr int64_t AGE = 1 << 16;  // a cached expansion stays usable while fewer nodes than this have been
                                  // appended since its probe (bounds the in-flight table: two
                                  // generations of AGE nodes, 2 x 1 MB of tagged entries, cache-
                                  // resident).  Aged caches are retired at round starts, so their
                                  // nodes are re-expanded with the next batches instead of costing
                                  // a round each at the top of the frontier (r02u: ~40k rounds)
static int64_t g_age_override = 0;  // tests only (acx_internal_greedy_age): a smaller AGE
static int64_t g_dcap_override = 0;  // tests only (acx_internal_greedy_init_cap): a smaller INIT_DCAP
constexpr int64_t INIT_DCAP = (int64_t)1 << 22;  // nodes of the first device store (doubled as needed)
constexpr int DEFAULT_BATCH = 64;  // parents per round (tools/greedy_sweep.py: 64-128 best on AK(3) /
                                   // Miller-Schupp at 10^6 nodes; larger rounds mostly expand nodes
                                   // that are never popped)

struct DevArgs {
    const uint64_t* parents;  // (n, kw) keys of the round's parents
    uint64_t* ckeys;          // (n, 12, kw) child keys (error sentinel: both length bytes 0xFF)
    uint64_t* chash;          // (n, 12) child key hashes
    int64_t* cknown;          // (n, 12) id of the node the child equals, -1 if none (as of this round)
    uint64_t* nkeys;          // (cap, kw) node keys by id
    const uint64_t* commit;   // (hi - lo, kw) keys of the nodes being committed
    uint64_t* table;          // buckets of 8: (id + 1) << 24 | fp24
    uint64_t bmask;
    int64_t lo, hi;           // commit: node ids [lo, hi)
    int n, L, kw, cyc;
    // round completion (greedy_round_kernel): blocks done so far (device word, back to 0 by the
    // last block) and the host-visible word the last block sets to `seq` -- the host sees the
    // round's outputs (pinned memory) without waiting for the stream
    uint32_t* blocks_done;
    uint32_t* done_flag;
    uint32_t seq;
};

// lane per (parent, action): one move, the child's key, its hash, its id if it is a node below
// a.lo (the nodes committed by earlier launches; greedy_round_kernel commits [lo, hi) in the same
// launch, and those entries are skipped: their keys may still be in flight, and the host checks
// every id >= lo itself)
template <int NW>
__device__ __forceinline__ void expand_lane(const DevArgs& a, int t) {
    if (t >= a.n * ACT) return;
    const int p = t / ACT, act = t - p * ACT;
    PresRegs<NW> pr, q;
    load_key<NW>(a.parents + (int64_t)p * a.kw, a.kw, a.L, pr);
    const bool cyc = a.cyc != 0;
    const int e = bfs::child_of<NW>(pr, is_clean<NW>(pr.w0, pr.n0, pr.w1, pr.n1, cyc), act, a.L, cyc, q);
    if (e != ACX_ERR_NONE) {
        q.n0 = 0xff;
        q.n1 = 0xff;
    }
    uint64_t key[NW + 1];
    make_key<NW>(a.L, q, key);
    uint64_t* dst = a.ckeys + (int64_t)t * a.kw;
#pragma unroll
    for (int k = 0; k < NW + 1; ++k)
        if (k < a.kw) dst[k] = key[k];
    Key<NW + 1> kk;
#pragma unroll
    for (int k = 0; k < NW + 1; ++k) kk.w[k] = k < a.kw ? key[k] : 0ull;
    const uint64_t h = khash<NW + 1>(kk, a.kw);
    a.chash[t] = h;
    int64_t known = -1;
    if (e == ACX_ERR_NONE) {
        const uint32_t fp = (uint32_t)(h >> 40);
        uint64_t b = h & a.bmask;
        for (uint64_t it = 0; it <= a.bmask && known < 0; ++it) {
            const uint64_t* bk = a.table + b * BUCKET;
            bool empty = false;
#pragma unroll
            for (int j = 0; j < BUCKET; ++j) {
                const uint64_t v = bk[j];
                if (v == 0) {
                    empty = true;
                    break;
                }
                if (((uint32_t)v & FP_MASK) == fp) {
                    const int64_t id = (int64_t)(v >> 24) - 1;
                    if (id < a.lo && keq<NW + 1>(a.nkeys + id * a.kw, kk, a.kw)) {
                        known = id;
                        break;
                    }
                }
            }
            if (empty) break;
            b = (b + 1) & a.bmask;
        }
    }
    a.cknown[t] = known;
}

// commit the node ids [lo, hi): store their keys and enter them in the table (all distinct, new)
template <int KWM>
__device__ __forceinline__ void commit_lane(const DevArgs& a, int64_t id) {
    if (id >= a.hi) return;
    const Key<KWM> k = kload<KWM>(a.commit + (id - a.lo) * a.kw, a.kw);
#pragma unroll
    for (int i = 0; i < KWM; ++i)
        if (i < a.kw) a.nkeys[id * a.kw + i] = k.w[i];
    const uint64_t h = khash<KWM>(k, a.kw);
    const uint64_t my = ((uint64_t)(id + 1) << 24) | (uint32_t)(h >> 40);
    uint64_t b = h & a.bmask;
    for (uint64_t it = 0; it <= a.bmask; ++it) {
        uint64_t* bk = a.table + b * BUCKET;
        for (int j = 0; j < BUCKET; ++j)
            if (atomicCAS((unsigned long long*)(bk + j), 0ull, (unsigned long long)my) == 0ull) return;
        b = (b + 1) & a.bmask;
    }
}

template <int KWM>
__global__ __launch_bounds__(256) void greedy_commit_kernel(DevArgs a) {
    commit_lane<KWM>(a, a.lo + (int64_t)blockIdx.x * 256 + threadIdx.x);
}

// one round in one launch: blocks [0, cblocks) commit the nodes [lo, hi) appended since the last
// round, the others expand the round's parents against the nodes committed before (ids < lo).
// The two halves touch disjoint key-store rows; a probe that meets a concurrent table insert
// sees the slot empty or holding an id >= lo (skipped), and either way reaches every older entry.
// Every block then releases its writes at system scope and counts itself done; the last one sets
// done_flag = seq, so the host can take the outputs (and reuse the staging buffers, which the
// commit blocks read) as soon as the last block is through, ahead of the stream's own completion.
template <int NW>
__global__ __launch_bounds__(256) void greedy_round_kernel(DevArgs a, int cblocks) {
    if ((int)blockIdx.x < cblocks)
        commit_lane<NW + 1>(a, a.lo + (int64_t)blockIdx.x * 256 + threadIdx.x);
    else
        expand_lane<NW>(a, ((int)blockIdx.x - cblocks) * 256 + threadIdx.x);
    if (a.done_flag == nullptr) return;
    __syncthreads();
    if (threadIdx.x == 0) {
        __threadfence_system();
        const uint32_t old = __hip_atomic_fetch_add(a.blocks_done, 1u, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT);
        if (old + 1u == gridDim.x) {
            __hip_atomic_store(a.blocks_done, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            __hip_atomic_store(a.done_flag, a.seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
        }
    }
}

// host restatement of bfs::khash (the kernels' hash): the host tables index by it
static inline uint64_t host_hash(const uint64_t* k, int kw) {
    uint64_t h = 0x9e3779b97f4a7c15ull;
    for (int i = 0; i < kw; ++i) h = fmix64(h ^ k[i]) + 0x632be59bd9b4e019ull;
    return test_hash::finish(fmix64(h));
}

static inline int64_t now_ns() {
    return std::chrono::duration_cast<std::chrono::nanoseconds>(std::chrono::steady_clock::now().time_since_epoch())
        .count();
}

struct Engine : Outcome {
    int L = 0, kw = 0, pk = 0, cyc = 0, dev = 0;
    int64_t max_nodes = 0, cap = 0;
    int64_t dcap = 0;  // nodes the device key store / visited set hold now (grown by doubling)
    uint64_t tsize = 0;
    int batch_cap = DEFAULT_BATCH;
    int64_t age = AGE;
    // nodes (ids in discovery order)
    std::vector<uint64_t> keys;
    std::vector<int64_t> parent;
    std::vector<int8_t> action;
    std::vector<int16_t> total;
    std::vector<int32_t> depth;
    std::vector<int32_t> cache_slot;  // -1: no cached children
    // cached children: per slot 12 keys, hashes, device-known ids, and the round of the probe
    std::vector<uint64_t> c_keys, c_hash;
    std::vector<int64_t> c_known;
    std::vector<int32_t> c_round;
    std::vector<int32_t> free_slots;
    // the recently appended nodes (the in-flight set)
    struct NodeKey {
        const Engine* E;
        const uint64_t* operator()(int64_t id) const { return &E->keys[(size_t)id * E->kw]; }
    };
    Recent<NodeKey> recent;
    std::vector<int64_t> n_at_round;  // round r: its kernel knew the ids below this; the host checks the rest
    int64_t committed = 0;            // ids < committed are in the device table
    int round = 0;
    int64_t st_rounds = 0, st_expanded = 0, ns_select = 0, ns_gpu = 0, ns_replay = 0, st_known = 0;
    // why each round's replay stopped: the top node was appended during that replay / was an
    // older node outside the round's batch / had children cached too long ago
    int64_t st_stop_new = 0, st_stop_old = 0, st_stop_aged = 0;
    int64_t ns_wait = 0, ns_cache = 0;  // inside the round trip: polling for the GPU / caching children
    int64_t st_retired = 0;             // cached expansions retired unused because they aged
    // staging: pinned host buffers the kernels read (parents + committed keys) and write (child
    // keys, hashes, known ids) directly, so a round is 2 launches and a completion poll -- no
    // copies, no blocking synchronisation
    hipStream_t stream = nullptr;
    DevArgs d{};
    uint64_t *h_in = nullptr, *h_out = nullptr;    // pinned, host view
    uint64_t *hd_in = nullptr, *hd_out = nullptr;  // the same memory, device view
    uint32_t *h_flag = nullptr, *hd_flag = nullptr;  // the rounds' completion word (pinned)
    uint32_t* d_blocks = nullptr;                    // the rounds' block count (device)
    uint32_t round_seq = 0;                          // the last round's completion value
    int64_t commit_cap = 0;

    // wait for the stream by polling (hipStreamSynchronize may sleep on an interrupt: tens of us
    // per round at ~1500 rounds per 10^6-node search)
    int wait() const {
        hipError_t e;
        while ((e = hipStreamQuery(stream)) == hipErrorNotReady) {
        }
        return e == hipSuccess ? ACX_OK : ACX_E_LAUNCH;
    }
    // a round: until its last block has set the completion word (greedy_round_kernel), or the
    // stream is through (checked every 256 polls: a launch that failed never sets the word)
    int wait_round(uint32_t seq) const {
        for (uint32_t i = 1;; ++i) {
            if (__atomic_load_n(h_flag, __ATOMIC_ACQUIRE) == seq) return ACX_OK;
            if ((i & 255u) == 0u) {
                const hipError_t e = hipStreamQuery(stream);
                if (e == hipSuccess) return ACX_OK;
                if (e != hipErrorNotReady) return ACX_E_LAUNCH;
            }
        }
    }

    ~Engine() {
        if (stream) (void)hipStreamSynchronize(stream);
        void* dp[] = {d.nkeys, d.table, d_blocks};
        for (void* p : dp)
            if (p) (void)hipFree(p);
        void* hp[] = {h_in, h_out, h_flag};
        for (void* p : hp)
            if (p) (void)hipHostFree(p);
        if (stream) (void)hipStreamDestroy(stream);
    }

    bool init(int L_, int64_t max_nodes_, int cyc_, int batch) {
        L = L_;
        kw = acx_key_words(L);
        pk = prio_words(L);
        frontier.init(pk, &pkeys);
        unexpanded.init(pk, &pkeys);
        cyc = cyc_;
        max_nodes = max_nodes_;
        cap = max_nodes + 12;
        batch_cap = batch > 0 ? batch : DEFAULT_BATCH;
        age = g_age_override > 0 ? g_age_override : AGE;  // a power of two
        if (hipGetDevice(&dev) != hipSuccess) return false;
        if (hipStreamCreateWithFlags(&stream, hipStreamNonBlocking) != hipSuccess) return false;
        commit_cap = 4 * (int64_t)batch_cap * ACT + 64;
        const size_t nb = (size_t)batch_cap;
        const size_t in_words = (nb + (size_t)commit_cap) * kw, out_words = nb * ACT * (kw + 2);
        d.L = L;
        d.kw = kw;
        d.cyc = cyc;
        bool ok = hipHostMalloc((void**)&h_in, in_words * 8, hipHostMallocMapped) == hipSuccess &&
                  hipHostMalloc((void**)&h_out, out_words * 8, hipHostMallocMapped) == hipSuccess &&
                  hipHostGetDevicePointer((void**)&hd_in, h_in, 0) == hipSuccess &&
                  hipHostGetDevicePointer((void**)&hd_out, h_out, 0) == hipSuccess &&
                  hipHostMalloc((void**)&h_flag, 64, hipHostMallocMapped) == hipSuccess &&
                  hipHostGetDevicePointer((void**)&hd_flag, h_flag, 0) == hipSuccess &&
                  hipMalloc((void**)&d_blocks, 64) == hipSuccess && hipMemset(d_blocks, 0, 64) == hipSuccess;
        if (ok) *h_flag = 0u;
        // the device store starts at min(budget, INIT_DCAP) nodes and doubles as the search grows
        // (the reference's set grows with the search: a large budget on a search that ends early
        // must not fail on an up-front allocation)
        ok = ok && grow(std::min<int64_t>(cap, g_dcap_override > 0 ? g_dcap_override : INIT_DCAP));
        if (!ok) (void)hipGetLastError();
        return ok;
    }

    // (re)allocate the device key store for n >= dcap nodes and a visited set of load <= 1/2,
    // keeping the committed nodes: their keys are copied and re-entered in the new table
    bool grow(int64_t n) {
        uint64_t ts = 1024;
        while (ts < 2 * (uint64_t)n) ts <<= 1;
        uint64_t *nk = nullptr, *tb = nullptr;
        if (hipMalloc((void**)&nk, (size_t)n * kw * 8) != hipSuccess) return false;
        if (hipMalloc((void**)&tb, ts * 8) != hipSuccess) {
            (void)hipFree(nk);
            return false;
        }
        bool ok = hipMemsetAsync(tb, 0, ts * 8, stream) == hipSuccess;
        if (ok && committed > 0)
            ok = hipMemcpyAsync(nk, d.nkeys, (size_t)committed * kw * 8, hipMemcpyDeviceToDevice, stream) == hipSuccess;
        if (ok && wait() == ACX_OK) {
            if (d.nkeys) (void)hipFree(d.nkeys);
            if (d.table) (void)hipFree(d.table);
        } else {
            (void)hipFree(nk);
            (void)hipFree(tb);
            return false;
        }
        d.nkeys = nk;
        d.table = tb;
        d.bmask = ts / BUCKET - 1;
        dcap = n;
        tsize = ts;
        if (committed > 0) {  // re-enter every committed node (the commit kernel rewrites its own key)
            d.commit = d.nkeys;
            d.lo = 0;
            d.hi = committed;
            commit_launch();
            if (hipGetLastError() != hipSuccess || wait() != ACX_OK) return false;
        }
        return true;
    }
    void commit_launch();

    // the nodes' heap keys (pk words per node id, prio_key), written once when a node is appended
    std::vector<uint64_t> pkeys;
    BucketHeap frontier;  // every node not popped yet: the reference's to_explore (pop order)
    // cached expansions in round order, to retire the ones that aged (their node then counts as
    // unexpanded again and is picked up by select() with the other smallest unexpanded nodes)
    std::vector<std::pair<int32_t, int64_t>> cache_fifo;
    size_t fifo_head = 0;
    BucketHeap unexpanded;  // the frontier nodes without usable cached children (expansion order)

    int64_t add_node(const uint64_t* k, uint64_t h, int64_t par, int act, int tot, int dep) {
        const int64_t id = (int64_t)parent.size();
        keys.insert(keys.end(), k, k + kw);
        parent.push_back(par);
        action.push_back((int8_t)act);
        total.push_back((int16_t)tot);
        depth.push_back(dep);
        cache_slot.push_back(-1);
        recent.insert(id, h);
        pkeys.resize(pkeys.size() + pk);
        uint64_t* pkey = &pkeys[(size_t)id * pk];
        prio_key(k, L, kw, pk, tot, dep, pkey);
        frontier.push(pkey[0], id);
        unexpanded.push(pkey[0], id);
        return id;
    }

    // A cached expansion is usable while the whole visit stays inside the in-flight table's
    // reach: the visit appends up to ACT nodes, and an append that starts a new generation
    // keeps only the `age` ids before it (Recent::insert), so every id >= `from` must still be
    // there after the visit's last append: parent.size() + ACT - from <= age.
    bool usable(int64_t id) const {
        const int32_t s = cache_slot[id];
        return s >= 0 && (int64_t)parent.size() + ACT - n_at_round[c_round[s]] <= age;
    }
    void drop_cache(int64_t id) {
        const int32_t s = cache_slot[id];
        if (s >= 0) {
            free_slots.push_back(s);
            cache_slot[id] = -1;
        }
    }

    // ---------------------------------------------------------------- one popped node
    // a child is already a node if the device knew it as of the probe, or it was appended since
    bool visit(int64_t id) {
        const int32_t s = cache_slot[id];
        const int64_t* kn = &c_known[(size_t)s * ACT];
        const int64_t from = n_at_round[c_round[s]];
        const bool ended = replay_children(
            &c_keys[(size_t)s * ACT * kw], &c_hash[(size_t)s * ACT], L, kw, *this, id, (int64_t)parent.size(),
            (int64_t)frontier.size(), max_nodes,
            [&](const uint64_t* k, uint64_t h, int a) {
                if (kn[a] >= 0) {
                    ++st_known;
                    return true;
                }
                return recent.find(k, h, from) >= 0;
            },
            [&](const uint64_t* k, uint64_t h, int a, int len) { add_node(k, h, id, a, len, depth[id] + 1); });
        drop_cache(id);
        return ended;
    }

    void push_unexpanded(int64_t id) { unexpanded.push(pkeys[(size_t)id * pk], id); }

    // the smallest frontier nodes without usable cached children (greedy expands them next)
    void select(std::vector<int64_t>& out) {
        out.clear();
        // retire the caches that aged since the last round: their nodes are unexpanded again
        const int64_t nn = (int64_t)parent.size();
        while (fifo_head < cache_fifo.size() && nn + ACT - n_at_round[cache_fifo[fifo_head].first] > age) {
            const auto [r, id] = cache_fifo[fifo_head++];
            const int32_t sl = cache_slot[id];
            if (sl >= 0 && c_round[sl] == r) {
                ++st_retired;
                drop_cache(id);
                push_unexpanded(id);
            }
        }
        if (fifo_head > 4096 && fifo_head * 2 > cache_fifo.size()) {
            cache_fifo.erase(cache_fifo.begin(), cache_fifo.begin() + (ptrdiff_t)fifo_head);
            fifo_head = 0;
        }
        while (!unexpanded.empty() && (int)out.size() < batch_cap) {
            out.push_back(unexpanded.top());
            unexpanded.pop();
        }
    }

    int expand_round(const std::vector<int64_t>& batch);

    int run(const int32_t* pres) {
        // the root: the (unreduced) input presentation itself (greedy.py:36-68)
        uint64_t root[ACX_MAX_L / 16 + 2];
        pack_key(pres, L, kw, root);
        int tot0 = 0;
        for (int i = 0; i < 2 * L; ++i) tot0 += pres[i] != 0;
        min_length = tot0;
        keys.assign(root, root + kw);
        parent.assign(1, -1);
        action.assign(1, -1);
        total.assign(1, (int16_t)tot0);
        depth.assign(1, 0);
        cache_slot.assign(1, -1);
        // every per-node array at its final size up front (no reallocation copies mid-search)
        const size_t nres = (size_t)std::min<int64_t>(cap, 1 << 26);
        keys.reserve(nres * kw);
        parent.reserve(nres);
        action.reserve(nres);
        total.reserve(nres);
        depth.reserve(nres);
        cache_slot.reserve(nres);
        recent = Recent<NodeKey>(age, kw, NodeKey{this});
        recent.insert(0, host_hash(root, kw));
        pkeys.assign(pk, 0ull);
        pkeys.reserve(nres * pk);
        prio_key(root, L, kw, pk, tot0, 0, pkeys.data());
        frontier.push(pkeys[0], 0);
        unexpanded.push(pkeys[0], 0);
        std::vector<int64_t> batch;
        while (status == 0) {
            const int64_t t0 = now_ns();
            const int64_t n_sel = (int64_t)parent.size();
            if (frontier.empty()) {  // to_explore ran empty (greedy.py:71)
                status = 2;
                break;
            }
            select(batch);
            const int64_t t1 = now_ns();
            ns_select += t1 - t0;
            const int e = expand_round(batch);
            if (e != ACX_OK) return e;
            const int64_t t2 = now_ns();
            ns_gpu += t2 - t1;
            ++round;
            // replay: pop while the top has usable cached children (greedy.py:71-119)
            while (status == 0) {
                if (frontier.empty()) {
                    status = 2;
                    break;
                }
                const int64_t id = frontier.top();
                if (!usable(id)) {
                    if (cache_slot[id] >= 0) {  // expanded before the last AGE appends: expand again
                        ++st_stop_aged;
                        drop_cache(id);
                        push_unexpanded(id);
                    } else if (id >= n_sel) {
                        ++st_stop_new;
                    } else {
                        ++st_stop_old;
                    }
                    break;
                }
                frontier.pop();
                visit(id);
            }
            ns_replay += now_ns() - t2;
        }
        return ACX_OK;
    }
};

void Engine::commit_launch() {
    const int64_t n = d.hi - d.lo;
    bfs::by_nw(L, [&](auto nw) {
        greedy_commit_kernel<decltype(nw)::value + 1><<<dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream>>>(d);
    });
}

int Engine::expand_round(const std::vector<int64_t>& batch) {
    const int n = (int)batch.size();
    const int64_t n_nodes = (int64_t)parent.size();
    if (n_nodes > dcap && !grow(std::min<int64_t>(cap, std::max<int64_t>(2 * dcap, n_nodes)))) return ACX_E_LAUNCH;
    // staging in: the batch's parent keys, then the keys of the nodes appended since the last
    // round.  The last commit_cap of those are committed by the round's own launch, beside the
    // expansion (greedy_round_kernel), which therefore knows only the ids below them: the host
    // checks the children against every node from there on (n_at_round)
    for (int i = 0; i < n; ++i) memcpy(h_in + (size_t)i * kw, &keys[(size_t)batch[i] * kw], 8 * kw);
    int64_t lo = committed;
    d.commit = hd_in + (size_t)n * kw;
    while (n_nodes - lo > commit_cap) {  // a backlog beyond one launch's staging: commit ahead
        memcpy(h_in + (size_t)n * kw, &keys[(size_t)lo * kw], (size_t)commit_cap * kw * 8);
        d.lo = lo;
        d.hi = lo + commit_cap;
        commit_launch();
        lo += commit_cap;
        if (hipGetLastError() != hipSuccess || wait() != ACX_OK) return ACX_E_LAUNCH;  // h_in is reused
    }
    if (n_nodes > lo) memcpy(h_in + (size_t)n * kw, &keys[(size_t)lo * kw], (size_t)(n_nodes - lo) * kw * 8);
    d.lo = lo;
    d.hi = n_nodes;
    committed = n_nodes;
    n_at_round.push_back(lo);
    d.n = n;
    d.parents = hd_in;
    d.ckeys = hd_out;
    d.chash = hd_out + (size_t)n * ACT * kw;
    d.cknown = reinterpret_cast<int64_t*>(d.chash + (size_t)n * ACT);
    if (n == 0 && n_nodes == lo) return ACX_OK;
    d.blocks_done = d_blocks;
    d.done_flag = hd_flag;
    d.seq = ++round_seq;
    const int cb = (int)((d.hi - d.lo + 255) / 256);
    bfs::by_nw(L, [&](auto nw) {
        greedy_round_kernel<decltype(nw)::value>
            <<<dim3((unsigned)(cb + (n * ACT + 255) / 256)), dim3(256), 0, stream>>>(d, cb);
    });
    if (n == 0) return hipGetLastError() == hipSuccess ? wait_round(d.seq) : ACX_E_LAUNCH;
    const int64_t tw = now_ns();
    if (hipGetLastError() != hipSuccess || wait_round(d.seq) != ACX_OK) return ACX_E_LAUNCH;
    const int64_t tc = now_ns();
    ns_wait += tc - tw;
    const uint64_t* ck = h_out;
    const uint64_t* ch = h_out + (size_t)n * ACT * kw;
    const int64_t* kn = reinterpret_cast<const int64_t*>(ch + (size_t)n * ACT);
    for (int i = 0; i < n; ++i) {
        int32_t s;
        if (!free_slots.empty()) {
            s = free_slots.back();
            free_slots.pop_back();
        } else {
            s = (int32_t)c_round.size();
            c_round.push_back(0);
            c_keys.resize(c_keys.size() + (size_t)ACT * kw);
            c_hash.resize(c_hash.size() + ACT);
            c_known.resize(c_known.size() + ACT);
        }
        memcpy(&c_keys[(size_t)s * ACT * kw], ck + (size_t)i * ACT * kw, (size_t)ACT * kw * 8);
        memcpy(&c_hash[(size_t)s * ACT], ch + (size_t)i * ACT, ACT * 8);
        memcpy(&c_known[(size_t)s * ACT], kn + (size_t)i * ACT, ACT * 8);
        c_round[s] = round;
        cache_slot[batch[i]] = s;
        cache_fifo.emplace_back(round, batch[i]);
    }
    ns_cache += now_ns() - tc;
    ++st_rounds;
    st_expanded += n;
    return ACX_OK;
}

}  // namespace greedy
}  // namespace acx

using namespace acx;
using namespace acx::greedy;

extern "C" {

int acx_greedy_run(const int32_t* presentation, int32_t L, int64_t max_nodes, int32_t cyclical, int32_t batch,
                   void** out_handle) {
    if (!presentation || !out_handle || L < 1 || L > ACX_MAX_L || max_nodes < 1 || max_nodes > (1ll << 38))
        return ACX_E_ARG;
    *out_handle = nullptr;
    Engine* E = new (std::nothrow) Engine();
    if (!E) return ACX_E_LAUNCH;
    if (!E->init(L, max_nodes, cyclical != 0, batch)) {
        delete E;
        return ACX_E_LAUNCH;
    }
    const int st = E->run(presentation);
    *out_handle = E;
    return st;
}

void acx_greedy_destroy(void* h) { delete static_cast<Engine*>(h); }

// tests only (not in acx.h): searches started afterwards use 2^log2_age as the cache age limit
// (0: the default AGE), so the retirement of aged caches is exercised harder at test sizes
void acx_internal_greedy_age(int32_t log2_age) { g_age_override = log2_age > 0 ? (int64_t)1 << log2_age : 0; }
// tests only: searches started afterwards begin with a 2^log2_cap-node device store (0: INIT_DCAP),
// so the store's regrowth mid-search is exercised at test sizes
void acx_internal_greedy_init_cap(int32_t log2_cap) { g_dcap_override = log2_cap > 0 ? (int64_t)1 << log2_cap : 0; }
// tests only (host code, no GPU): the heap priority key of a packed key at L (out: the key's
// words, (40 + 6L + 63) / 64 of them), through the fast path (generic = 0, L <= 40) or the
// per-group one; returns the number of words, -1 on bad arguments
int32_t acx_internal_greedy_prio_key(int32_t L, const uint64_t* key, int32_t total, int32_t depth, uint64_t* out,
                                     int32_t generic) {
    if (L < 1 || L > ACX_MAX_L || !key || !out) return -1;
    const int pk = prio_words(L);
    prio_key(key, L, acx_key_words(L), pk, total, depth, out, generic != 0);
    return pk;
}

// 0 running, 1 success, 2 failed, 3 move error; budget_hit, min_length, nodes (len(tree_nodes))
int32_t acx_greedy_status(void* h, int32_t* budget_hit, int32_t* min_length, int64_t* n_nodes) {
    Engine* E = static_cast<Engine*>(h);
    return read_status(*E, (int64_t)E->parent.size(), budget_hit, min_length, n_nodes);
}

int64_t acx_greedy_path(void* h, int32_t* actions, int32_t* totals, int64_t cap) {
    Engine* E = static_cast<Engine*>(h);
    return read_path(*E, E->parent.data(), E->action.data(), E->total.data(), actions, totals, cap);
}

// out[0] rounds, [1] parents expanded, [2] parents popped, [3] children the device knew,
// [4..6] host ns selecting / in the GPU round trip / replaying, [7..9] replays that stopped at a
// node appended during the replay / at an older unexpanded node / at an aged cache, [10..11] ns
// of the round trips spent polling for the GPU / caching children, [12] cached expansions
// retired unused because they aged
void acx_greedy_stats(void* h, int64_t* out) {
    Engine* E = static_cast<Engine*>(h);
    out[0] = E->st_rounds;
    out[1] = E->st_expanded;
    out[2] = (int64_t)E->popped.size();
    out[3] = E->st_known;
    out[4] = E->ns_select;
    out[5] = E->ns_gpu;
    out[6] = E->ns_replay;
    out[7] = E->st_stop_new;
    out[8] = E->st_stop_old;
    out[9] = E->st_stop_aged;
    out[10] = E->ns_wait;
    out[11] = E->ns_cache;
    out[12] = E->st_retired;
}

int64_t acx_greedy_min_trace(void* h, int32_t* out, int64_t cap) {
    Engine* E = static_cast<Engine*>(h);
    return read_array(E->trace.data(), (int64_t)E->trace.size(), out, cap);
}

int64_t acx_greedy_popped(void* h, int64_t* ids, int64_t cap) {
    Engine* E = static_cast<Engine*>(h);
    return read_array(E->popped.data(), (int64_t)E->popped.size(), ids, cap);
}

int64_t acx_greedy_node_keys(void* h, uint64_t* out, int64_t cap) {
    Engine* E = static_cast<Engine*>(h);
    return read_array(E->keys.data(), (int64_t)E->parent.size(), out, cap, E->kw);
}

int32_t acx_greedy_found(void* h, int32_t* first_letters, int64_t* explored) {
    Engine* E = static_cast<Engine*>(h);
    return read_found(*E, E->L, first_letters, explored);
}

}  // extern "C"
