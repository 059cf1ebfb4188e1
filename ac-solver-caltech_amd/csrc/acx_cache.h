// acx_cache.h -- the solution cache's key algebra and its read-only probe (acx_cache.hip holds the
// table's owner: the fill, the growth and the C functions).
//
// The reference (value_search/value_guided_search.py:100-153, _check_cache_with_rotations) looks a
// state up as itself, then with relator 0 rotated left by k = 1 .. n0 - 1 letters, then with
// relator 1 rotated by k = 1 .. n1 - 1: the *variants* of the state, numbered in that order
//   v = 0                      the state
//   v = 1 .. c0                relator 0 rotated by k = v
//   v = c0 + 1 .. c0 + c1      relator 1 rotated by k = v - c0
// with c_h = n_h - 1, or 0 for a relator of one letter or one whose first and last letters cancel
// (:129-133).  Only one relator is ever rotated.  The backfill (:156-250) inserts the same
// variants of every state of a solved path in the same order, so both sides enumerate through
// variant_counts / variant_at below.
//
// The first part is plain inline functions for the host compiler and for hipcc
// (tests/cache_key_check.cpp compiles it alone); the probe after it is device code.
#pragma once
#include <stdint.h>

#include "acx_key.h"

namespace acx {
namespace cache {

// the m bits (1 <= m <= 64) of a key from bit position `bit` on; they may straddle two words, and
// bit + m lies inside the key
ACX_HD inline uint64_t key_bits(const uint64_t* k, int bit, int m) {
    const int w = bit >> 6, o = bit & 63;
    uint64_t v = k[w] >> o;
    if (o + m > 64) v |= k[w + 1] << (64 - o);
    return m == 64 ? v : v & ((1ull << m) - 1ull);
}

// word w of the key `in` whose relator h, of n letters, is rotated left by k letters (0 <= k < n;
// k = 0: the key's own word): letter i of the rotated relator is letter (i + k) mod n.  The 2-bit
// letters of relator h are the bits 2hL .. 2hL + 2n of the key, so the rotation is one of a bit
// field that begins and ends anywhere in the key's words (L = 18: relator 1 straddles words 0 and
// 1; L = 128: a relator spans four words).  Every other bit -- the other relator, the two count
// bytes -- is copied.
ACX_HD inline uint64_t key_rot_word(const uint64_t* in, int L, int h, int n, int k, int w) {
    const uint64_t v = in[w];
    const int lo = 2 * h * L, hi = lo + 2 * n;
    const int b0 = 64 * w;
    const int s = b0 > lo ? b0 : lo, e = b0 + 64 < hi ? b0 + 64 : hi;  // the field's bits in this word
    if (k == 0 || s >= e) return v;
    const int m = e - s;
    int src = s - lo + 2 * k;  // output bit lo + j is input bit lo + (j + 2k) mod 2n
    if (src >= 2 * n) src -= 2 * n;
    const int first = m < 2 * n - src ? m : 2 * n - src;  // up to the field's end, then from its start
    uint64_t f = key_bits(in, lo + src, first);
    if (first < m) f |= key_bits(in, lo, m - first) << first;
    const uint64_t mask = (m == 64 ? ~0ull : (1ull << m) - 1ull) << (s - b0);
    return (v & ~mask) | (f << (s - b0));
}

// rotations of relator h the reference visits: n - 1, or 0 (one letter; cancelling ends)
ACX_HD inline int rot_count(const uint64_t* key, int L, int h) {
    const int n = key_len(key, L, h);
    if (n <= 1) return 0;
    if (key_code_at(key, L, h, 0) == (key_code_at(key, L, h, n - 1) ^ 1u)) return 0;
    return n - 1;
}

// a state's variants: c[h] = rot_count of relator h; returns their number, 1 + c[0] + c[1]
ACX_HD inline int variant_counts(const uint64_t* key, int L, int c[2]) {
    c[0] = rot_count(key, L, 0);
    c[1] = rot_count(key, L, 1);
    return 1 + c[0] + c[1];
}

// variant v (0 <= v < 1 + c0 + c1): the relator it rotates and by how many letters (v = 0: 0, 0)
ACX_HD inline void variant_at(int c0, int v, int& rel, int& k) {
    rel = v > c0;
    k = rel ? v - c0 : v;
}

// An entry's order code is its row in the cache's key store: rows are handed out in the order the
// reference's sequential backfill would insert -- call, path, step, variant -- so the smaller row
// of two equal states is the reference's entry.  What a row stands for is kept beside its key:
//   meta = path ordinal << 32 | step << 9 | rel << 8 | k      (step < 2^23, k < 2^8)
constexpr int META_STEP_BITS = 23;
ACX_HD inline uint64_t meta_pack(uint64_t ordinal, uint64_t step, int rel, int k) {
    return (ordinal << 32) | (step << 9) | ((uint64_t)rel << 8) | (uint64_t)k;
}

}  // namespace cache
}  // namespace acx

#ifdef __HIPCC__
#include <hip/hip_runtime.h>

#include "acx_bfs_common.h"
#include "acx_visited.h"

namespace acx {
namespace cache {

using namespace acx::bfs;
using visited::BUCKET;

constexpr uint64_t EP = 1ull << visited::EP_SHIFT;  // the one epoch of a cache's table: 0 is an empty slot
constexpr int64_t MISS = -1;

// what a probe needs of a cache: the table (nb buckets of 8 entries, acx_visited.h's format), the
// key store the entries' codes index, and its rows.  Read-only while searches run: plain loads.
struct View {
    const uint64_t* table;
    const uint64_t* store;
    int64_t rows;
    uint32_t nb;
};

// the key `in` with relator h (n letters) rotated by k, in registers
template <int KWM>
__device__ __forceinline__ Key<KWM> rotated(const uint64_t* in, int kw, int L, int h, int n, int k) {
    Key<KWM> r;
#pragma unroll
    for (int w = 0; w < KWM; ++w) r.w[w] = w < kw ? key_rot_word(in, L, h, n, k, w) : 0ull;
    return r;
}

// the entry (row) of the state `key`, or MISS.  Entries are never removed, so the first empty slot
// on the probe path ends the search; the walk is bounded by the table's buckets.
template <int KWM>
__device__ __forceinline__ int64_t find(const View& c, const Key<KWM>& key, int kw) {
    const uint64_t hash = khash<KWM>(key, kw);
    const uint32_t fp = visited::fp_of(hash);
    uint32_t b = __umulhi((uint32_t)hash, c.nb);
    for (uint32_t it = 0; it < c.nb; ++it, b = b + 1 == c.nb ? 0 : b + 1) {
        const uint64_t* bk = c.table + (uint64_t)b * BUCKET;
#pragma unroll
        for (int j = 0; j < BUCKET; ++j) {
            const uint64_t v = bk[j];
            if (v == 0) return MISS;
            if (visited::entry_fp(v) != fp) continue;
            const uint64_t row = visited::entry_code(v);
            if ((int64_t)row < c.rows && keq<KWM>(c.store + row * kw, key, kw)) return (int64_t)row;
        }
    }
    return MISS;
}

// the reference's _check_cache_with_rotations of one state by one wave: `key` (kw words, LDS or
// global, the same for every lane) is the state; the lanes take its variants 64 at a time, rounds
// in order (at most ceil(255 / 64) = 4), and the first hit of the first round that has one is the
// reference's.  Every lane returns the same (entry or MISS, rel, k).
struct Hit {
    int64_t entry;
    int32_t rel, k;
};

template <int KWM>
__device__ __forceinline__ Hit probe(const View& c, const uint64_t* key, int kw, int L, int lane) {
    int cnt[2];
    const int total = variant_counts(key, L, cnt);
    const int n0 = key_len(key, L, 0), n1 = key_len(key, L, 1);
    for (int base = 0; base < total; base += WAVE) {
        const int v = base + lane;
        int64_t e = MISS;
        int rel = 0, k = 0;
        if (v < total) {
            variant_at(cnt[0], v, rel, k);
            e = find<KWM>(c, rotated<KWM>(key, kw, L, rel, rel ? n1 : n0, k), kw);
        }
        const unsigned long long hit = __ballot(e != MISS);
        if (hit) {
            const int src = __builtin_ctzll(hit);
            const uint32_t lo = (uint32_t)__shfl((int)(uint32_t)e, src, WAVE);
            const uint32_t hi = (uint32_t)__shfl((int)(uint32_t)((uint64_t)e >> 32), src, WAVE);
            return Hit{(int64_t)(((uint64_t)hi << 32) | lo), __shfl(rel, src, WAVE), __shfl(k, src, WAVE)};
        }
    }
    return Hit{MISS, 0, 0};
}

// ---------------------------------------------------------------------------------------------
// A cache attached to a handle of a scored engine (acx_{vgreedy,beam,mcts}_set_cache).  The
// engine's begin and make kernels, and the fused one, have a second instantiation that takes an
// Attach (last; the fused kernel: second) and probes where the reference looks (the engine's file says where); the instantiation
// without a cache is the device code it was.  The probe is called from the kernels and not folded into pop::expand:
// acx_pop.h records what a shared routine between expand and append cost these kernels.
// The hit records belong to the attachment, one per search of the handle, not to the engines'
// slices: the engines' bytes formulas do not change.
// ---------------------------------------------------------------------------------------------
struct Attach {
    View view;
    Hit* hit;  // (n_cap)
};

// what a kernel template with the parameters `At... at` -- nothing, or an Attach -- hands its
// body: body<NW, sizeof...(At) != 0>(.., attach_of(at...)).  The instantiation without a cache takes
// no such argument.
__device__ __forceinline__ Attach attach_of() { return Attach{}; }
__device__ __forceinline__ const Attach& attach_of(const Attach& at) { return at; }

// search q ends on a cache hit (one thread): the path reader returns the path to `node` plus
// (act, tot), the state that hit; a root hit (plen == 0) returns no path at all -- the record
// then carries a status without a path, as a trivial MCTS root does
template <class A, class S>
__device__ __forceinline__ void ended_cached(const A& a, int64_t q, S* st, const Attach& c, const Hit& h, int32_t act,
                                             int64_t node, uint32_t tot, int64_t n_nodes, int64_t steps, int64_t plen) {
    a.res[q] = {plen ? ACX_BFS_CACHED : ACX_BFS_BUDGET, act, node, (int32_t)tot, 0, n_nodes};
    a.status[q] = ACX_BFS_CACHED;
    a.nodes[q] = n_nodes;
    a.parents[q] = steps;
    a.min_length[q] = 2;  // the reference reports 2 on every hit
    a.path_len[q] = plen;
    c.hit[q] = h;
    st->done = 1;
    st->n_nodes = n_nodes;
    st->steps = steps;
    st->cand_n = 0;
    a.counts[q] = 0;
}

static __global__ __launch_bounds__(TPB) void hits_kernel(const Hit* hit, int64_t n, int64_t* entry, int32_t* rel,
                                                          int32_t* k) {
    const int64_t q = (int64_t)blockIdx.x * TPB + threadIdx.x;
    if (q >= n) return;
    entry[q] = hit[q].entry;
    rel[q] = hit[q].rel;
    k[q] = hit[q].k;
}

// the cache's handle (acx_cache.hip owns it)
struct Handle {
    int L = 0, kw = 0;
    int64_t cap = 0, rows = 0;
    uint32_t nb = 0;
    uint64_t* store = nullptr;
    uint64_t* meta = nullptr;
    uint64_t* table = nullptr;
    uint64_t* count = nullptr;  // [0] distinct states, [1] an insert found the table full

    ~Handle() {
        for (uint64_t* p : {store, meta, table, count})
            if (p) (void)hipFree(p);
    }
    View view() const { return View{table, store, rows, nb}; }
};

// host: the bodies of an engine's acx_*_set_cache and acx_*_cache_hits.  H is its batch::Handle,
// which keeps the attached cache and the hit records (freed with it).
template <class H>
static int set_cache(void* h, void* cache) {
    H* S = static_cast<H*>(h);
    Handle* C = static_cast<Handle*>(cache);
    if (!S || (C && C->L != S->a.L)) return ACX_E_ARG;
    if (C && !S->cache_hits) {
        if (hipMalloc(&S->cache_hits, sizeof(Hit) * (size_t)S->n_cap) != hipSuccess) {
            (void)hipGetLastError();
            S->cache_hits = nullptr;
            return ACX_E_LAUNCH;
        }
    }
    S->cache = C;
    return ACX_OK;
}

// the attachment of a handle as its kernels take it (read when a call begins: the cache may have
// grown since it was attached); false: none.  scored::launch_by_cache (acx_scored.h) is its reader.
template <class H>
static bool attached(const H* S, Attach& out) {
    if (!S->cache) return false;
    out = Attach{static_cast<const Handle*>(S->cache)->view(), static_cast<Hit*>(S->cache_hits)};
    return true;
}

template <class H>
static int read_hits(void* h, int64_t n, int64_t* entry, int32_t* rel, int32_t* k, void* stream) {
    H* S = static_cast<H*>(h);
    if (!S || !S->cache || !S->cache_hits || !entry || !rel || !k || n < 0 || n > S->n_cap) return ACX_E_ARG;
    if (n == 0) return ACX_OK;
    hits_kernel<<<dim3((unsigned)((n + TPB - 1) / TPB)), dim3(TPB), 0, (hipStream_t)stream>>>(
        static_cast<const Hit*>(S->cache_hits), n, entry, rel, k);
    return hipGetLastError() == hipSuccess ? ACX_OK : ACX_E_LAUNCH;
}

}  // namespace cache
}  // namespace acx
#endif  // __HIPCC__
