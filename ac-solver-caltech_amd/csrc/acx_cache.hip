// acx_cache.hip -- the solution cache of the searches scored by a caller's model: a device-resident
// hash set of packed state keys for one L that outlives a call (C-ABI acx_cache_* in
// include/acx.h; acx/search/_cache.py is its owner on the host).
//
// Reference: value_search/value_guided_search.py:100-250.  backfill_solution_cache replays a solved
// path, and for every state S_i before the last it sets cache[S_i] = path[i:] if S_i is absent, then
// (expand_rotations) does the same for every rotation variant of S_i in the order of acx_cache.h.
// "If absent" makes the dict depend on the insertion order: calls, then paths, then steps, then
// variants.
//
// Memory, for a capacity of C rows (acx_cache_bytes):
//   store  (C, kw) uint64   the key of every variant ever emitted, in the reference's insertion
//                           order: row r is the r-th "if absent" test of the cache's lifetime;
//   meta   (C) uint64       what row r stands for (path ordinal, step, relator, k: acx_cache.h), so
//                           that the host resolves an entry to its path only when someone asks;
//   table  (nb * 8) uint64  the set, in acx_visited.h's buckets and entry format, an entry's code
//                           being its row; nb = ceil(C / 4), so the load stays <= 1/2 however many
//                           of the rows are distinct states;
//   count  (2) uint64       distinct states held; a flag raised by an insert that found no slot.
// A row whose state was already held stays in the store as a loser (its key is what key_eq of a
// later probe never reads: no entry names it).  That spends store rows on duplicates and buys an
// insert with no compaction pass and codes that need no translation: the row order is the
// reference's order.
//
// Parallel shape of a fill.  A path's states exist only by replaying it, one move after another, so
// a path is sequential; paths are independent.  One wave takes one path: every lane replays it in
// its own registers with the engines' move code (acx_moves.h, through child_of as pop::expand does),
// which costs what one lane replaying would (the wave is SIMD) and leaves the state in every lane
// without LDS traffic; after each move the lanes spread over the state's variants (up to 255 at
// L = 128: four rounds of 64) and write their rotated keys.  A thread per path would replay as
// fast but then write a state's up to 255 variants one after another.
//   count   cache_replay_kernel<NW, false>: variants per path, and the step at which a move raises;
//           the host sums them (one number per path crosses, nothing per entry), refuses the call
//           if a path raised, and grows the cache before anything is written;
//   emit    cache_replay_kernel<NW, true>: the same replay, now writing rows voff[p].. of the store;
//   insert  cache_insert_kernel: thread per new row, visited::insert with code = row.  An equal
//           state's entry is taken by atomicMin, so the least row -- the reference's first
//           insertion -- holds it whatever order the lanes run in, within a call and across calls.
//           It is a launch of its own because key_eq reads other rows' keys: all are written.
// Growth: acx_cache_reserve doubles the capacity until the rows fit; the store and meta are copied,
// and cache_rehash_kernel (thread per old slot) re-inserts every entry, code kept, into the new
// table of twice the buckets.
//
// Every loop is bounded: the replay by the path's length, the variant rounds by 1 + 2 (ACX_MAX_L -
// 1) variants, an insert's and a probe's walk by the table's buckets, the packing by 2L letters.
// While a fill runs, table lines are read with agent-scope atomic loads and written by atomics
// only; the lookup and the searches run in later launches and use plain loads.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <new>

#include "acx.h"
#include "acx_moves.h"

#include "acx_bfs_common.h"
#include "acx_cache.h"
#include "acx_visited.h"

namespace acx {
namespace cache {

constexpr int GT = WAVE;  // threads per path / per looked-up state: one wave
constexpr int64_t MAX_ROWS = 1ll << 33;  // codes stay below acx_visited.h's 2^34
constexpr int RKW = ACX_MAX_L / 16 + 2;

inline uint32_t buckets_for(int64_t cap) { return (uint32_t)((2 * cap + BUCKET - 1) / BUCKET); }

// the table while a fill runs (acx_visited.h's Table)
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
        for (int j = 0; j < BUCKET; ++j) e[j] = tload(bk + j);
    }
};

// The (2L) int32 row `st` packed into rk (RKW words of LDS) by one wave; false for every lane: the
// row is outside the packed domain (letters in +-1, +-2, zeros only as right padding, no empty
// relator).  rk is complete after the call.
__device__ __forceinline__ bool pack_row(const int32_t* st, int L, int kw, uint64_t* rk, uint32_t* s_n, int lane) {
    if (lane < RKW) rk[lane] = 0;
    if (lane < 2) s_n[lane] = 0;
    wsync();
    bool bad = false;
    for (int t = lane; t < 2 * L; t += GT) {
        const int32_t v = st[t];
        const int h = t >= L, i = t - h * L;
        if (v < -2 || v > 2) bad = true;
        else if (v == 0) bad = bad || (i + 1 < L && st[t + 1] != 0);
        else {
            const int bit = 2 * t;
            atomicOr((unsigned long long*)&rk[bit >> 6], (unsigned long long)(key_code(v) << (bit & 63)));
            atomicAdd(&s_n[h], 1u);
        }
    }
    wsync();
    bad = __ballot(bad) != 0 || s_n[0] == 0 || s_n[1] == 0;
    if (lane == 0) {  // the length field at bit 4L may straddle a word
        const uint64_t lens = (uint64_t)s_n[0] | ((uint64_t)s_n[1] << 8);
        const int bit = 4 * L;
        rk[bit / 64] |= lens << (bit % 64);
        if (bit % 64 > 48 && bit / 64 + 1 < kw) rk[bit / 64 + 1] |= lens >> (64 - bit % 64);
    }
    wsync();
    return !bad;
}

struct FillArgs {
    const int32_t* states;   // (P, 2L) the paths' presentations
    const int64_t* poff;     // (P + 1) offsets of the paths' actions
    const int32_t* actions;  // the paths' actions, concatenated
    const int64_t* voff;     // (P + 1) emit: rows of each path, relative to row0
    int64_t* counts;         // (P) count: variants of each path
    int32_t* err;            // (P) count: 0, 1 + the step whose move raises, or -1: a row outside the domain
    uint64_t* store;
    uint64_t* meta;
    int64_t P, row0, cap, ordinal0;
    int L, kw, cyc, expand, replay;
};

// one wave per path (see the header): count, or emit
template <int NW, bool EMIT>
__global__ __launch_bounds__(GT) void cache_replay_kernel(FillArgs a) {
    __shared__ uint64_t sk[RKW];
    __shared__ uint32_t s_n[2];
    const int lane = threadIdx.x;
    const int64_t p = blockIdx.x;
    const int L = a.L, kw = a.kw;
    const bool cyc = a.cyc != 0;
    const bool ok = pack_row(a.states + p * 2 * L, L, kw, sk, s_n, lane);
    if (!ok) {
        if (!EMIT && lane == 0) {
            a.counts[p] = 0;
            a.err[p] = -1;
        }
        return;
    }
    const int64_t a0 = a.poff[p], len = a.poff[p + 1] - a0;
    // a dict's entry (replay == 0) is its state alone, whatever its path holds
    const int64_t steps = a.replay ? len : 1;
    const int64_t room = EMIT ? a.voff[p + 1] - a.voff[p] : 0;
    const int64_t row_p = EMIT ? a.row0 + a.voff[p] : 0;
    PresRegs<NW> pr;
    load_key<NW>(sk, kw, L, pr);
    int64_t run = 0;
    int32_t err = 0;
    for (int64_t i = 0; i < steps; ++i) {
        if (i > 0) {  // S_i, packed where the lanes can index it
            wsync();
            if (lane == 0) store_key<NW>(sk, kw, L, pr);
            wsync();
        }
        int c[2] = {0, 0};
        int total = 1;
        if (a.expand) total = variant_counts(sk, L, c);
        if constexpr (EMIT) {
            for (int v = lane; v < total; v += GT) {
                int rel, k;
                variant_at(c[0], v, rel, k);
                const int64_t row = row_p + run + v;
                if (run + v >= room || row >= a.cap) continue;  // (never: the count sized them)
                const int n = rel ? pr.n1 : pr.n0;
                for (int w = 0; w < kw; ++w) a.store[row * kw + w] = key_rot_word(sk, L, rel, n, k, w);
                a.meta[row] = meta_pack((uint64_t)(a.ordinal0 + p), (uint64_t)i, rel, k);
            }
        }
        run += total;
        if (!a.replay) break;
        const bool clean = is_clean<NW>(pr.w0, pr.n0, pr.w1, pr.n1, cyc);
        PresRegs<NW> ch;
        if (child_of<NW>(pr, clean, a.actions[a0 + i], L, cyc, ch) != ACX_ERR_NONE) {
            err = (int32_t)(i < 0x7ffffffe ? i + 1 : 0x7fffffff);
            break;
        }
        pr = ch;
    }
    if (!EMIT && lane == 0) {
        a.counts[p] = run;
        a.err[p] = err;
    }
}

template <int KWM>
__global__ __launch_bounds__(TPB) void cache_insert_kernel(Buckets tb, const uint64_t* store, int64_t row0, int64_t n,
                                                           int64_t rows, int kw, uint64_t* count) {
    const int64_t t = (int64_t)blockIdx.x * TPB + threadIdx.x;
    if (t >= n) return;
    const uint64_t code = (uint64_t)(row0 + t);
    const Key<KWM> key = kload<KWM>(store + code * kw, kw);
    const visited::Outcome r = visited::insert(
        tb, EP, code, khash<KWM>(key, kw),
        [&](uint64_t vc) { return vc < (uint64_t)rows && keq<KWM>(store + vc * kw, key, kw); },
        [&](uint32_t, uint64_t displaced) {  // a claimed empty slot is a new state
            if (displaced == visited::NO_CODE) atomicAdd((unsigned long long*)count, 1ull);
        });
    if (r == visited::FULL) count[1] = 1;  // (never at load <= 1/2)
}

// thread per slot of the old table: its entry, code kept, into the new one
template <int KWM>
__global__ __launch_bounds__(TPB) void cache_rehash_kernel(const uint64_t* old, int64_t slots, Buckets tb,
                                                           const uint64_t* store, int64_t rows, int kw, uint64_t* count) {
    const int64_t t = (int64_t)blockIdx.x * TPB + threadIdx.x;
    if (t >= slots) return;
    const uint64_t v = old[t];
    if (v == 0) return;
    const uint64_t code = visited::entry_code(v);
    if (code >= (uint64_t)rows) return;  // (never)
    const Key<KWM> key = kload<KWM>(store + code * kw, kw);
    const visited::Outcome r = visited::insert(
        tb, EP, code, khash<KWM>(key, kw),
        [&](uint64_t vc) { return vc < (uint64_t)rows && keq<KWM>(store + vc * kw, key, kw); },
        [](uint32_t, uint64_t) {});
    if (r == visited::FULL) count[1] = 1;
}

// one wave per state: the reference's _check_cache_with_rotations (acx_cache.h's probe)
template <int KWM>
__global__ __launch_bounds__(GT) void cache_lookup_kernel(View c, const int32_t* states, int64_t n, int L, int kw,
                                                          int64_t* entry, int32_t* rel, int32_t* k) {
    __shared__ uint64_t sk[RKW];
    __shared__ uint32_t s_n[2];
    const int lane = threadIdx.x;
    const int64_t q = blockIdx.x;
    Hit h{MISS, 0, 0};
    if (pack_row(states + q * 2 * L, L, kw, sk, s_n, lane)) h = probe<KWM>(c, sk, kw, L, lane);
    if (lane == 0) {
        entry[q] = h.entry;
        rel[q] = h.rel;
        k[q] = h.k;
    }
}

static __global__ __launch_bounds__(TPB) void cache_rows_kernel(const uint64_t* store, const uint64_t* meta, int64_t rows,
                                                                int kw, const int64_t* entries, int64_t m, uint64_t* keys,
                                                                uint64_t* metas) {
    const int64_t t = (int64_t)blockIdx.x * TPB + threadIdx.x;
    if (t >= m) return;
    const int64_t r = entries[t];
    const bool ok = r >= 0 && r < rows;
    for (int w = 0; w < kw; ++w) keys[t * kw + w] = ok ? store[r * kw + w] : 0ull;
    metas[t] = ok ? meta[r] : ~0ull;
}

// the rows the table's entries name, in slot order, at most cap of them; *n counts them all
static __global__ __launch_bounds__(TPB) void cache_entries_kernel(const uint64_t* table, int64_t slots, int64_t* out,
                                                                   int64_t cap, unsigned long long* n) {
    const int64_t t = (int64_t)blockIdx.x * TPB + threadIdx.x;
    if (t >= slots) return;
    const uint64_t v = table[t];
    if (v == 0) return;
    const unsigned long long pos = atomicAdd(n, 1ull);
    if ((int64_t)pos < cap) out[pos] = (int64_t)visited::entry_code(v);
}

// the replay of a call's paths: counting (acx_cache_count) or writing their rows (acx_cache_fill)
template <bool EMIT>
static void replay(int L, const FillArgs& a, hipStream_t st) {
    bfs::by_nw(L, [&](auto nw) {
        cache_replay_kernel<decltype(nw)::value, EMIT><<<dim3((unsigned)a.P), dim3(GT), 0, st>>>(a);
    });
}

static bool fill_args_ok(Handle* S, const int32_t* states, const int64_t* poff, const int32_t* actions, int64_t P) {
    return S && states && poff && actions && P >= 0 && P <= (1ll << 30);
}

}  // namespace cache
}  // namespace acx

namespace cache = acx::cache;
using acx::bfs::by_nw;
using cache::Handle;

extern "C" {

int64_t acx_cache_bytes(int32_t L, int64_t capacity) {
    if (L < 1 || L > ACX_MAX_L || capacity < 1 || capacity > cache::MAX_ROWS) return ACX_E_ARG;
    return (8 * (int64_t)acx_key_words(L) + 8) * capacity + 64 * (int64_t)cache::buckets_for(capacity) + 16;
}

void* acx_cache_create(int32_t L, int64_t capacity) {
    if (acx_cache_bytes(L, capacity) < 0) return nullptr;
    Handle* S = new (std::nothrow) Handle();
    if (!S) return nullptr;
    S->L = L;
    S->kw = acx_key_words(L);
    S->cap = capacity;
    S->nb = cache::buckets_for(capacity);
    const size_t tb = (size_t)S->nb * cache::BUCKET * 8;
    const bool ok = hipMalloc((void**)&S->store, 8 * (size_t)S->kw * capacity) == hipSuccess &&
                    hipMalloc((void**)&S->meta, 8 * (size_t)capacity) == hipSuccess &&
                    hipMalloc((void**)&S->table, tb) == hipSuccess && hipMemset(S->table, 0, tb) == hipSuccess &&
                    hipMalloc((void**)&S->count, 16) == hipSuccess && hipMemset(S->count, 0, 16) == hipSuccess;
    if (!ok) {
        (void)hipGetLastError();
        delete S;
        return nullptr;
    }
    return S;
}

void acx_cache_destroy(void* h) { delete static_cast<Handle*>(h); }

int acx_cache_info(void* h, int64_t* out, void* stream) {
    Handle* S = static_cast<Handle*>(h);
    if (!S || !out) return ACX_E_ARG;
    uint64_t cnt[2] = {0, 0};
    hipStream_t st = (hipStream_t)stream;
    if (hipMemcpyAsync(cnt, S->count, 16, hipMemcpyDeviceToHost, st) != hipSuccess ||
        hipStreamSynchronize(st) != hipSuccess)
        return ACX_E_LAUNCH;
    out[0] = (int64_t)cnt[0];
    out[1] = S->rows;
    out[2] = S->cap;
    out[3] = (int64_t)S->nb;
    out[4] = (int64_t)cnt[1];
    return ACX_OK;
}

int acx_cache_count(void* h, const int32_t* states, const int64_t* poff, const int32_t* actions, int64_t P,
                    int32_t cyclical, int32_t expand_rotations, int32_t replay, int64_t* counts, int32_t* err,
                    void* stream) {
    Handle* S = static_cast<Handle*>(h);
    if (!cache::fill_args_ok(S, states, poff, actions, P) || !counts || !err) return ACX_E_ARG;
    if (P == 0) return ACX_OK;
    cache::FillArgs a{states, poff, actions, nullptr, counts, err, nullptr, nullptr, P, 0, 0, 0,
                      S->L, S->kw, cyclical != 0, expand_rotations != 0, replay != 0};
    cache::replay<false>(S->L, a, (hipStream_t)stream);
    return hipGetLastError() == hipSuccess ? ACX_OK : ACX_E_LAUNCH;
}

int acx_cache_reserve(void* h, int64_t rows, void* stream) {
    Handle* S = static_cast<Handle*>(h);
    if (!S || rows < 0 || rows > cache::MAX_ROWS) return ACX_E_ARG;
    if (rows <= S->cap) return ACX_OK;
    int64_t cap = S->cap;
    while (cap < rows) cap *= 2;
    hipStream_t st = (hipStream_t)stream;
    const uint32_t nb = cache::buckets_for(cap);
    const size_t tb = (size_t)nb * cache::BUCKET * 8;
    uint64_t *store = nullptr, *meta = nullptr, *table = nullptr;
    bool ok = hipMalloc((void**)&store, 8 * (size_t)S->kw * cap) == hipSuccess &&
              hipMalloc((void**)&meta, 8 * (size_t)cap) == hipSuccess && hipMalloc((void**)&table, tb) == hipSuccess &&
              hipMemsetAsync(table, 0, tb, st) == hipSuccess;
    if (ok && S->rows > 0)
        ok = hipMemcpyAsync(store, S->store, 8 * (size_t)S->kw * S->rows, hipMemcpyDeviceToDevice, st) == hipSuccess &&
             hipMemcpyAsync(meta, S->meta, 8 * (size_t)S->rows, hipMemcpyDeviceToDevice, st) == hipSuccess;
    if (ok) {  // the entries, codes kept, into the new table; the rehash reads the new store's copy of the keys
        const int64_t slots = (int64_t)S->nb * cache::BUCKET;
        by_nw(S->L, [&](auto nw) {
            cache::cache_rehash_kernel<decltype(nw)::value + 1>
                <<<dim3((unsigned)((slots + acx::bfs::TPB - 1) / acx::bfs::TPB)), dim3(acx::bfs::TPB), 0, st>>>(
                    S->table, slots, cache::Buckets{table, nb}, store, S->rows, S->kw, S->count);
        });
        ok = hipGetLastError() == hipSuccess && hipStreamSynchronize(st) == hipSuccess;
    }
    if (ok) {  // installed only now: a failure above leaves the cache as it was
        uint64_t *old_store = S->store, *old_meta = S->meta, *old_table = S->table;
        S->store = store;
        S->meta = meta;
        S->table = table;
        S->nb = nb;
        S->cap = cap;
        store = old_store;  // freed below: nothing reads them once the stream has drained
        meta = old_meta;
        table = old_table;
    } else {
        (void)hipDeviceSynchronize();  // nothing of the new arrays is in flight when they are freed
    }
    for (uint64_t* p : {store, meta, table})
        if (p) (void)hipFree(p);
    if (!ok) (void)hipGetLastError();
    return ok ? ACX_OK : ACX_E_LAUNCH;
}

int acx_cache_fill(void* h, const int32_t* states, const int64_t* poff, const int32_t* actions, const int64_t* voff,
                   int64_t total, int64_t ordinal0, int64_t P, int32_t cyclical, int32_t expand_rotations,
                   int32_t replay, void* stream) {
    Handle* S = static_cast<Handle*>(h);
    if (!cache::fill_args_ok(S, states, poff, actions, P) || !voff || total < 0 || ordinal0 < 0 ||
        ordinal0 + P > (1ll << 32) || S->rows + total > S->cap)
        return ACX_E_ARG;
    if (P == 0 || total == 0) return ACX_OK;
    hipStream_t st = (hipStream_t)stream;
    cache::FillArgs a{states, poff, actions, voff, nullptr, nullptr, S->store, S->meta, P, S->rows, S->cap, ordinal0,
                      S->L, S->kw, cyclical != 0, expand_rotations != 0, replay != 0};
    cache::replay<true>(S->L, a, st);
    if (hipGetLastError() != hipSuccess) return ACX_E_LAUNCH;
    by_nw(S->L, [&](auto nw) {
        cache::cache_insert_kernel<decltype(nw)::value + 1>
            <<<dim3((unsigned)((total + acx::bfs::TPB - 1) / acx::bfs::TPB)), dim3(acx::bfs::TPB), 0, st>>>(
                cache::Buckets{S->table, S->nb}, S->store, S->rows, total, S->rows + total, S->kw, S->count);
    });
    S->rows += total;
    return hipGetLastError() == hipSuccess ? ACX_OK : ACX_E_LAUNCH;
}

int acx_cache_lookup(void* h, const int32_t* states, int64_t n, int64_t* entry, int32_t* rel, int32_t* k,
                     void* stream) {
    Handle* S = static_cast<Handle*>(h);
    if (!S || n < 0 || n > (1ll << 30) || (n > 0 && (!states || !entry || !rel || !k))) return ACX_E_ARG;
    if (n == 0) return ACX_OK;
    by_nw(S->L, [&](auto nw) {
        cache::cache_lookup_kernel<decltype(nw)::value + 1><<<dim3((unsigned)n), dim3(cache::GT), 0, (hipStream_t)stream>>>(
            S->view(), states, n, S->L, S->kw, entry, rel, k);
    });
    return hipGetLastError() == hipSuccess ? ACX_OK : ACX_E_LAUNCH;
}

int acx_cache_rows(void* h, const int64_t* entries, int64_t m, uint64_t* keys, uint64_t* metas, void* stream) {
    Handle* S = static_cast<Handle*>(h);
    if (!S || m < 0 || (m > 0 && (!entries || !keys || !metas))) return ACX_E_ARG;
    if (m == 0) return ACX_OK;
    cache::cache_rows_kernel<<<dim3((unsigned)((m + acx::bfs::TPB - 1) / acx::bfs::TPB)), dim3(acx::bfs::TPB), 0,
                               (hipStream_t)stream>>>(S->store, S->meta, S->rows, S->kw, entries, m, keys, metas);
    return hipGetLastError() == hipSuccess ? ACX_OK : ACX_E_LAUNCH;
}

int acx_cache_entries(void* h, int64_t* out, int64_t cap, int64_t* n, void* stream) {
    Handle* S = static_cast<Handle*>(h);
    if (!S || !n || cap < 0 || (cap > 0 && !out)) return ACX_E_ARG;
    hipStream_t st = (hipStream_t)stream;
    if (hipMemsetAsync(n, 0, 8, st) != hipSuccess) return ACX_E_LAUNCH;
    const int64_t slots = (int64_t)S->nb * cache::BUCKET;
    cache::cache_entries_kernel<<<dim3((unsigned)((slots + acx::bfs::TPB - 1) / acx::bfs::TPB)), dim3(acx::bfs::TPB), 0,
                                  st>>>(S->table, slots, out, cap, (unsigned long long*)n);
    return hipGetLastError() == hipSuccess ? ACX_OK : ACX_E_LAUNCH;
}

}  // extern "C"
