// acx_bfs_common.h -- pieces shared by the search engines on the device: the single-GPU BFS
// (acx_bfs.hip), the batched BFS (acx_mbfs.hip), the owner-partitioned multi-GPU BFS
// (acx_sbfs.hip) and the greedy search (acx_greedy.hip): packed-key compare / hash, the child
// step, wave and block scans, the budget-cut predicate.  The key format itself (field readers,
// pack_key) is acx_key.h, the visited-set format and insert acx_visited.h, the chunk verdict
// acx_bfs_verdict.h.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include <type_traits>

#include "acx.h"
#include "acx_key.h"
#include "acx_moves.h"
#include "acx_test_hash.h"

namespace acx {
namespace bfs {

constexpr uint64_t CHUNK = 1ull << 63;
constexpr uint32_t NONE = 0xffffffffu;
constexpr uint32_t SEEN = 0xffffffffu;  // slot index of a child whose state is already a node
constexpr int TPB = 256;


__host__ __device__ __forceinline__ uint64_t fmix64(uint64_t k) {
    k ^= k >> 33;
    k *= 0xff51afd7ed558ccdull;
    k ^= k >> 33;
    k *= 0xc4ceb9fe1a85ec53ull;
    k ^= k >> 33;
    return k;
}

template <int KWM>
struct Key {
    uint64_t w[KWM];
};

template <int KWM>
__device__ __forceinline__ Key<KWM> kload(const uint64_t* p, int kw) {
    Key<KWM> k;
#pragma unroll
    for (int i = 0; i < KWM; ++i) k.w[i] = i < kw ? p[i] : 0ull;
    return k;
}

template <int KWM>
__device__ __forceinline__ bool keq(const uint64_t* p, const Key<KWM>& k, int kw) {
    bool e = true;
#pragma unroll
    for (int i = 0; i < KWM; ++i)
        if (i < kw) e &= p[i] == k.w[i];
    return e;
}

template <int KWM>
__host__ __device__ __forceinline__ uint64_t khash(const Key<KWM>& k, int kw) {
    uint64_t h = 0x9e3779b97f4a7c15ull;
#pragma unroll
    for (int i = 0; i < KWM; ++i)
        if (i < kw) h = fmix64(h ^ k.w[i]) + 0x632be59bd9b4e019ull;
    return test_hash::finish(fmix64(h));  // the identity in the shipped build (acx_test_hash.h)
}

// n bytes (n % 4 == 0) device -> pinned host memory by a kernel (no DMA-engine copy: rocprofv3's
// memory-copy tracing never receives the completion of a device-to-host engine copy on this
// stack -- profiles/r04/bfs_trace_c: one undelivered callback per copy -- so the exports below
// write host memory from a kernel instead)
static __global__ void d2h_copy_kernel(uint32_t* __restrict__ dst, const uint32_t* __restrict__ src, size_t n4) {
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += (size_t)gridDim.x * blockDim.x)
        dst[i] = src[i];
}

// device -> pageable host memory on the caller's stream, through a pinned bounce buffer the
// workspace keeps (*pin, allocated on first use, BOUNCE bytes; freed with the workspace): no
// hipMemcpy on the null stream, no pageable destination, nothing freed while a copy may be
// in flight
constexpr size_t BOUNCE = 16u << 20;
static inline int copy_to_host(void* dst, const void* src, size_t n, hipStream_t st, void** pin) {
    if (n == 0) return ACX_OK;
    if (n % 4) return ACX_E_ARG;
    if (!*pin && hipHostMalloc(pin, BOUNCE, hipHostMallocDefault) != hipSuccess) {
        *pin = nullptr;
        return ACX_E_LAUNCH;
    }
    for (size_t off = 0; off < n; off += BOUNCE) {
        const size_t m = n - off < BOUNCE ? n - off : BOUNCE;
        d2h_copy_kernel<<<dim3(1024), dim3(256), 0, st>>>(static_cast<uint32_t*>(*pin),
                                                           reinterpret_cast<const uint32_t*>((const char*)src + off), m / 4);
        if (hipGetLastError() != hipSuccess || hipStreamSynchronize(st) != hipSuccess) return ACX_E_LAUNCH;
        memcpy((char*)dst + off, *pin, m);
    }
    return ACX_OK;
}

// LDS written by the wave's lanes is visible to the whole wave after this
__device__ __forceinline__ void wsync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

__device__ __forceinline__ uint32_t wave_min(uint32_t v) {
#pragma unroll
    for (int o = 1; o < WAVE; o <<= 1) v = min(v, (uint32_t)__shfl_xor((int)v, o, WAVE));
    return v;
}
__device__ __forceinline__ uint32_t wave_sum(uint32_t v) {
#pragma unroll
    for (int o = 1; o < WAVE; o <<= 1) v += (uint32_t)__shfl_xor((int)v, o, WAVE);
    return v;
}

__device__ __forceinline__ uint64_t tload(const uint64_t* p) {
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// inclusive prefix sum of x over the wave's lanes
__device__ __forceinline__ uint32_t wave_incl_sum(uint32_t x, int lane) {
#pragma unroll
    for (int o = 1; o < WAVE; o <<= 1) {
        const uint32_t y = __shfl_up(x, o, WAVE);
        if (lane >= o) x += y;
    }
    return x;
}

// exclusive prefix sum of v over a block of N threads (sh: N / 64 words); total in `tot`
template <int N>
__device__ __forceinline__ uint32_t block_excl_scan(uint32_t v, uint32_t* sh, uint32_t& tot) {
    const int lane = threadIdx.x & (WAVE - 1), wid = threadIdx.x / WAVE;
    const uint32_t x = wave_incl_sum(v, lane);
    if (lane == WAVE - 1) sh[wid] = x;
    __syncthreads();
    uint32_t off = 0;
    tot = 0;
#pragma unroll
    for (int i = 0; i < N / WAVE; ++i) {
        off += i < wid ? sh[i] : 0u;
        tot += sh[i];
    }
    return off + x - v;
}

// exclusive scan of x[0..n) in place by one block of 1024 threads (sh: 16 words; thread t takes
// a contiguous run of ceil(n / 1024) elements); returns the total.  each(i) is called once per
// element, by the thread that owns it, in the summing pass: a caller that folds a second array
// over the same indices shares that pass's memory round trips (a loop of its own after the scan
// cost bfs_scan_kernel 3 us per chunk, 16.3 -> 19.5 us)
template <class Each>
__device__ __forceinline__ uint32_t scan_array_1024(uint32_t* x, int n, uint32_t* sh, Each each) {
    const int per = (n + 1023) / 1024;
    const int b0 = threadIdx.x * per, b1 = min(n, b0 + per);
    uint32_t loc = 0;
    for (int i = b0; i < b1; ++i) {
        loc += x[i];
        each(i);
    }
    uint32_t tot;
    uint32_t run = block_excl_scan<1024>(loc, sh, tot);
    for (int i = b0; i < b1; ++i) {
        const uint32_t c = x[i];
        x[i] = run;
        run += c;
    }
    return tot;
}
__device__ __forceinline__ uint32_t scan_array_1024(uint32_t* x, int n, uint32_t* sh) {
    return scan_array_1024(x, n, sh, [](int) {});
}

// The node-budget cut falls after the first parent through which len(tree_nodes) reaches
// max_nodes: `base` / `incl` nodes appended by the chunk before / through the parent, need =
// max_nodes - len(tree_nodes) before the chunk.  The reference tests after every parent, so a
// budget that is already spent (need <= 0) cuts after the chunk's first parent.
__host__ __device__ __forceinline__ bool budget_cut_after(int64_t base, int64_t incl, int64_t need, bool first_parent) {
    return (base < need || first_parent) && incl >= need;
}

// the child of `parent` by move `act` (the parent's is_clean flag picks the move routine that
// skips the reductions a clean word cannot need); returns the move's ACX_ERR_*
template <int NW>
__device__ __forceinline__ int child_of(const PresRegs<NW>& parent, bool clean, int act, int L, bool cyc,
                                        PresRegs<NW>& child) {
    child = parent;
    return clean ? ac_move_clean<NW>(child.w0, child.n0, child.w1, child.n1, act, L, cyc)
                 : ac_move<NW>(child.w0, child.n0, child.w1, child.n1, act, L, cyc);
}

// a root's packed key, passed to its kernel by value (no host-to-device copy per search)
struct RootKey {
    uint64_t w[ACX_MAX_L / 16 + 2];
};

__device__ __forceinline__ uint32_t block_min(uint32_t v, uint32_t* sh) {
    const int lane = threadIdx.x & (WAVE - 1), wid = threadIdx.x / WAVE;
#pragma unroll
    for (int o = 1; o < WAVE; o <<= 1) v = min(v, (uint32_t)__shfl_xor((int)v, o, WAVE));
    if (lane == 0) sh[wid] = v;
    __syncthreads();
    uint32_t m = 0xffffffffu;
#pragma unroll
    for (int i = 0; i < TPB / WAVE; ++i) m = min(m, sh[i]);
    return m;
}

static inline int nw_for(int L) { return L <= 16 ? 1 : L <= 32 ? 2 : L <= 48 ? 3 : L <= 64 ? 4 : 8; }

// f(std::integral_constant<int, NW>{}) for the key-word count of L: a call site is a generic lambda
// that launches its kernel's instantiation, [&](auto nw) { k<decltype(nw)::value><<<..>>>(..); }
template <class F>
static void by_nw(int L, F&& f) {
    switch (nw_for(L)) {
        case 1: f(std::integral_constant<int, 1>{}); break;
        case 2: f(std::integral_constant<int, 2>{}); break;
        case 3: f(std::integral_constant<int, 3>{}); break;
        case 4: f(std::integral_constant<int, 4>{}); break;
        default: f(std::integral_constant<int, 8>{}); break;
    }
}

}  // namespace bfs
}  // namespace acx
