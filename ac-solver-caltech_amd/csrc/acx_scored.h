// acx_scored.h -- the step frame of the engines scored by the caller (acx_beam.hip, acx_vgreedy.hip,
// acx_mcts.hip): a search lives between launches, and a step of all searches is
//   make     the engine's kernel (beam: expand, vgreedy: pop, mcts: select): a live search's new nodes, rows
//            cand_base .. cand_base + cand_n of its store, are the step's candidates; then the
//            offsets kernel turns the per-search counts into offsets and their sum M;
//   gather   one contiguous copy per search into the caller's (M, kw) array, which the caller scores;
//   (the engine's own second kernel -- beam: select, vgreedy: push, mcts: backup -- reads
//   scores[offsets[q] ..]).
// A search that ends writes its results where it ends (ended) and has no candidates from then
// on; finish() copies the results out.
//
// An engine's Args has, besides its own arrays: state (n) its State, derived from scored::State;
// counts (n) int32; offsets (n + 1) int64; n, the searches of the running call.  Its Engine
// (acx_batch.h) adds GATHER_THREADS, MOST (the gather's guard: the most candidates of a search in a
// step; 0: none) and LIVE (the offsets kernel also counts the searches that have not ended).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "acx.h"

#include "acx_batch.h"
#include "acx_bfs_common.h"
#include "acx_cache.h"

namespace acx {
namespace scored {

using namespace acx::bfs;
using batch::Res;

// a search between two launches; an engine's own fields follow in its derived struct
struct State {
    int64_t n_nodes, max_nodes, steps, cand_base;
    int32_t done, cand_n;
    uint32_t running;  // min total of the root and the children looked at
    int32_t pad;
};

// bytes per search of the frame's arrays, with the engine's State
template <class S>
constexpr size_t RECORD = sizeof(Res) + sizeof(S) + 4 + 16 + 4 + 8 + 8 + 4 + 8;

// the arrays every scored engine has after its own, for its Engine::arrays (acx_batch.h)
template <class A, class F>
void arrays(A& a, F f) {
    f(a.state, sizeof(*a.state), true);  // (zeroed: done = 0 with no candidates before the first begin)
    f(a.counts, 4, true);
    f(a.offsets, 16, true);  // n + 1 entries
    f(a.status, 4, true);
    f(a.nodes, 8, true);
    f(a.parents, 8, true);  // steps
    f(a.min_length, 4, true);
    f(a.path_len, 8, true);
}

// search q has ended (one thread)
template <class A, class S>
__device__ __forceinline__ void ended(const A& a, int64_t q, S* st, int32_t status, int32_t act, int64_t node,
                                      int64_t n_nodes, int64_t steps, uint32_t running, int64_t plen) {
    batch::write_result(a, q, Res{status, act, node, 2, 0, n_nodes}, steps, running, plen);
    st->done = 1;
    st->n_nodes = n_nodes;
    st->steps = steps;
    st->cand_n = 0;
    a.counts[q] = 0;
}

// offsets = exclusive prefix sum of counts (n + 1 entries); out[0] = their sum M and, with LIVE,
// out[1] = the searches that have not ended: one block
template <class A, bool LIVE>
__global__ __launch_bounds__(1024) void offsets_kernel(A a, int64_t* out) {
    __shared__ uint32_t sh[1024 / WAVE];
    int64_t run = 0, live = 0;
    for (int64_t b = 0; b < a.n; b += 1024) {
        const int64_t i = b + threadIdx.x;
        const uint32_t v = i < a.n ? (uint32_t)a.counts[i] : 0u;
        uint32_t tot;
        const uint32_t ex = block_excl_scan<1024>(v, sh, tot);
        if (i < a.n) a.offsets[i] = run + ex;
        run += tot;
        __syncthreads();  // sh is rewritten
        if constexpr (LIVE) {
            uint32_t ltot;
            block_excl_scan<1024>(i < a.n && !a.state[i].done ? 1u : 0u, sh, ltot);
            live += ltot;
            __syncthreads();  // sh is rewritten by the next chunk
        }
    }
    if (threadIdx.x == 0) {
        a.offsets[a.n] = run;
        out[0] = run;
        if constexpr (LIVE) out[1] = live;
    }
}

// the candidates' keys of search q are consecutive rows of its store: one copy per search
template <class A, int THREADS, int MOST>
__global__ __launch_bounds__(THREADS) void gather_kernel(A a, uint64_t* keys, int64_t M) {
    const int64_t q = blockIdx.x;
    const int64_t n = a.counts[q], off = a.offsets[q], base = a.state[q].cand_base;
    if (n <= 0 || (MOST && n > MOST) || off < 0 || off + n > M || base < 0 || base + n > a.rows) return;
    const uint64_t* src = a.store + (q * a.rows + base) * a.kw;
    uint64_t* dst = keys + off * a.kw;
    for (int64_t t = threadIdx.x; t < n * a.kw; t += THREADS) dst[t] = src[t];
}

static __global__ __launch_bounds__(TPB) void results_kernel(batch::Args a, int64_t n, int32_t* status, int64_t* nodes,
                                                             int64_t* steps, int32_t* min_length, int64_t* path_len) {
    const int64_t q = (int64_t)blockIdx.x * TPB + threadIdx.x;
    if (q >= n) return;
    status[q] = a.status[q];
    nodes[q] = a.nodes[q];
    steps[q] = a.parents[q];
    min_length[q] = a.min_length[q];
    path_len[q] = a.path_len[q];
}

// host: the bodies of an engine's acx_*_begin, its make call, _gather, its take call and _finish.
// The launch of a kernel that probes the solution cache when one is attached to the handle
// (acx_cache.h): launch(nw, args, at...) starts the kernel's instantiation for decltype(nw)::value
// key words; `at...` is the handle's attachment or, without one, nothing, and the kernel's `At... at`
// takes it.  This is the one place that reads the attachment.
template <class E, class Launch>
static void launch_by_cache(const batch::Handle<E>* S, Launch launch) {
    cache::Attach at;
    if (cache::attached(S, at))
        by_nw(S->a.L, [&](auto nw) { launch(nw, S->a, at); });
    else
        by_nw(S->a.L, [&](auto nw) { launch(nw, S->a); });
}

// A run of n searches begins: own_ok is the engine's check of its own arguments, launch (above)
// starts its begin kernel
template <class E, class Launch>
static int begin(void* h, const int32_t* states, const int64_t* budgets, bool own_ok, int64_t n, void* stream,
                 Launch launch) {
    batch::Handle<E>* S = static_cast<batch::Handle<E>*>(h);
    if (!S || !states || !budgets || !own_ok || n < 0 || n > S->n_cap) return ACX_E_ARG;
    typename E::Args& a = S->a;
    a.n = n;
    if (n == 0) return ACX_OK;
    hipStream_t st = (hipStream_t)stream;
    if (!batch::new_epoch(S, st)) return ACX_E_LAUNCH;
    a.states = states;
    a.budgets = budgets;
    launch_by_cache(S, launch);
    return hipGetLastError() == hipSuccess ? ACX_OK : ACX_E_LAUNCH;
}

// the first half of a step: the engine's kernel (launch, as above) over the live searches, then the
// offsets; out takes M (and, for an engine with LIVE, the live count)
template <class E, class Launch>
static int make(void* h, int64_t* out, void* stream, Launch launch) {
    batch::Handle<E>* S = static_cast<batch::Handle<E>*>(h);
    if (!S || !out) return ACX_E_ARG;
    const typename E::Args& a = S->a;
    hipStream_t st = (hipStream_t)stream;
    if (a.n > 0) launch_by_cache(S, launch);
    offsets_kernel<typename E::Args, E::LIVE><<<dim3(1), dim3(1024), 0, st>>>(a, out);
    return hipGetLastError() == hipSuccess ? ACX_OK : ACX_E_LAUNCH;
}

// a step's (keys or scores, M) arguments; ACX_OK with *run = false: nothing to do
template <class E>
static int step_args(void* h, const void* rows, int64_t M, bool* run) {
    batch::Handle<E>* S = static_cast<batch::Handle<E>*>(h);
    *run = false;
    if (!S || M < 0 || (M > 0 && !rows)) return ACX_E_ARG;
    *run = S->a.n != 0 && M != 0;
    return ACX_OK;
}

template <class E>
static int gather(void* h, uint64_t* keys, int64_t M, void* stream) {
    bool run;
    if (const int e = step_args<E>(h, keys, M, &run); e != ACX_OK || !run) return e;
    const typename E::Args& a = static_cast<batch::Handle<E>*>(h)->a;
    gather_kernel<typename E::Args, E::GATHER_THREADS, E::MOST>
        <<<dim3((unsigned)a.n), dim3(E::GATHER_THREADS), 0, (hipStream_t)stream>>>(a, keys, M);
    return hipGetLastError() == hipSuccess ? ACX_OK : ACX_E_LAUNCH;
}

// the second half of a step: launch(args, stream) is the engine's second kernel over the scores
template <class E, class Launch>
static int take(void* h, const float* scores, int64_t M, void* stream, Launch launch) {
    bool run;
    if (const int e = step_args<E>(h, scores, M, &run); e != ACX_OK || !run) return e;
    launch(static_cast<batch::Handle<E>*>(h)->a, (hipStream_t)stream);
    return hipGetLastError() == hipSuccess ? ACX_OK : ACX_E_LAUNCH;
}

template <class E>
static int finish(void* h, int32_t* status, int64_t* nodes, int64_t* steps, int32_t* min_length, int64_t* path_len,
                  void* stream) {
    batch::Handle<E>* S = static_cast<batch::Handle<E>*>(h);
    if (!S || !status || !nodes || !steps || !min_length || !path_len) return ACX_E_ARG;
    const typename E::Args& a = S->a;
    if (a.n == 0) return ACX_OK;
    results_kernel<<<dim3((unsigned)((a.n + TPB - 1) / TPB)), dim3(TPB), 0, (hipStream_t)stream>>>(
        a, a.n, status, nodes, steps, min_length, path_len);
    return hipGetLastError() == hipSuccess ? ACX_OK : ACX_E_LAUNCH;
}

}  // namespace scored
}  // namespace acx
