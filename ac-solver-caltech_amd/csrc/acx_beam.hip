// acx_beam.hip -- beam search over a batch of presentations, scored by the caller: one workgroup
// owns one search, and a step of all searches is two launches with the caller's scorer between
// them.  The searches are independent, so no workgroup ever waits on another.
//
// Reference: value_search/value_guided_search.py:417-561 (beam_search) with time_limit=None; the
// solution cache is the second instantiation of the begin and expand kernels (begin_body /
// expand_body below; beam_expand_kernel<1 / 2 / 3 / 4 / 8, cache::Attach>: 84 / 90 / 92 / 94 / 136
// VGPRs, profiles/cache/kernel_resources.md, where its name has _cached before _kernel).  The root
// is node 0 and total_nodes starts at 1; while total_nodes < max_nodes a step makes the beam's
// children in sequential order s = 12 * (rank in the beam) + action, and for each in that order: a raising move ends the search (ACX_BFS_MOVE_ERROR); a child
// of total length 2 ends it, found, before the visited test; a child not yet visited becomes the
// next node and the step's next candidate; if that makes total_nodes >= max_nodes the expansion
// stops at that child (bfs tests after each parent: acx_bfs_verdict.h is not what happens here).
// A step without a candidate ends the search (ACX_BFS_EXHAUSTED); otherwise the new beam is the
// first `width` of a stable sort of the candidates by score.  After a budget cut the candidates are
// still scored and selected, and the next expand ends the search (ACX_BFS_BUDGET).
//
// A search's memory is a private slice of each of the handle's arrays, those of acx_mbfs.hip:
//   store  (B, kw) uint64   node keys in node_id order (node 0 is the root).  A step's candidates
//                           are its new nodes, rows cand_base .. cand_base + cand_n, so the gather
//                           copies them from here and there are no candidate slots to fill;
//   meta   (B) uint32       parent index << 4 | action;
//   table  (nb * 8) uint64  the visited set, 8 nb >= 2 (B + 11 + 768);
//   scratch (768, kw) uint64  only for L > 64: a pass's child keys;
//   beam   (max_width) uint32  the beam's node indices, best first;
//   state, res, the five results, the step's candidate count and its offset (140 bytes).
// Bytes per search (acx_beam_bytes):
//   8 kw B + 4 B + 64 ceil((B + 779) / 4) + 4 max_width + 140 [+ 6144 kw when L > 64].
//
// beam_expand_kernel<NW>: a step is ceil(beam / 64) passes, each a round (acx_round.h) over the
// next P <= 64 beam entries, read through the beam.  Its decide finds the cut: the child that holds
// the (max_nodes - total_nodes)-th survivor in sequential order, from the per-parent survivor
// masks, and only survivors up to it are committed (a pass with a budget verdict still commits).
// A pass is committed before the next begins, so a later pass meets the earlier ones' children as
// nodes.  A round code is n + s with n the node count when its pass began: every holder of a pass
// without a verdict is recoded to its node index (< the next pass's n) at commit, and a pass with
// a verdict (cut included) is the search's last insert, so no round code is ever read as a node
// index.
// beam_select_kernel<CAP>: the candidates' (score key, index) words (acx_beam_key.h) are sorted in
// LDS by a bitonic network over the next power of two, CAP = 1024, 4096 or 16384 words by the
// handle's max_width (8, 32, 128 KiB of LDS: the widest class holds one workgroup per CU, which is
// why a handle of narrow beams does not use it).
// The frame of a step -- the state's common fields, the offsets, the gather, the results copy and
// the host bodies of begin / expand / gather / finish -- is acx_scored.h, shared with acx_vgreedy.hip.
// Every loop is bounded: steps by the budget (a step without a verdict adds a node), passes by
// max_width / 64, probes by nb, the path walk by the node count.
//
// Registers and LDS (tools/kernel_resources.py; every figure: profiles/heap_shared/kernel_resources.md):
//   beam_expand_kernel<1 / 2 / 3 / 4 / 8>   82 / 88 / 90 / 92 / 126 VGPRs, 18,976 / 25,120 / 31,264 /
//       37,408 / 6,684 B of LDS: 5, 5, 5, 4, 4 waves per SIMD, as mbfs_kernel (<2> also has 24 B of
//       private memory per lane; the other widths have none);
//   beam_select_kernel<1024 / 4096 / 16384>   12 / 12 / 13 VGPRs, 8,200 / 32,776 / 131,080 B of LDS.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "acx.h"

#include "acx_beam_key.h"
#include "acx_cache.h"
#include "acx_round.h"
#include "acx_scored.h"

namespace acx {
namespace beam {

using namespace acx::round;
using scored::ended;

struct State : scored::State {
    int32_t beam_n, width;  // entries of the beam, and the most it may hold
};

struct Args : round::Args {
    State* state;
    uint32_t* beam;    // (max_width) per search
    int32_t* counts;   // (n) the step's candidates per search
    int64_t* offsets;  // (n + 1) their exclusive prefix sum
    int32_t max_width;
    int64_t n;  // searches of the running call
};

// The begin and expand kernels' bodies, with the solution cache's probe compiled in or not (CACHE;
// acx_cache.h): the kernels below are their two instantiations each.  With a cache
// (value_guided_search.py:460-464, 503-511) the root is probed before anything (a hit: nodes 1,
// steps 0), and in a pass every child below the first raising or trivial one is probed, as the
// reference does after a child's trivial test and before its visited test.  The first hit in
// sequential order then stands where a trivial child would: the children before it meet the visited
// set, a budget cut among them comes first (a cached child beyond the cut is never looked at), and
// nodes is total_nodes as counted up to that child.  Wave w probes children w, w + 4, ... below the
// least hit found so far.
template <int NW, bool CACHE>
__device__ __forceinline__ void begin_body(const Args& a, const int32_t* widths, const cache::Attach& at) {
    const int tid = threadIdx.x;
    const int64_t q = blockIdx.x;
    const int kw = a.kw;
    uint64_t* store = a.store + q * a.rows * kw;
    uint32_t* meta = a.meta + q * a.rows;
    uint64_t* table = a.table + q * (int64_t)a.nb * BUCKET;
    State* S = a.state + q;
    const batch::Root root = batch::root_setup<TPB, NW>(a, q, store, meta, table);
    cache::Hit hit{cache::MISS, 0, 0};
    if constexpr (CACHE) {
        if (!root.refused && tid < WAVE) hit = cache::probe<NW + 1>(at.view, root.key, kw, a.L, tid);
    }
    if (tid != 0) return;
    const int32_t w = widths[q];
    const bool wide = w < 1 || w > a.max_width;
    // (a search's results are written where it ends; until then, and for a width out of range:)
    if (!root.refused) batch::write_result(a, q, Res{ACX_MBFS_OVERFLOW, 0, 0, 0, 0, 0}, 0, 0, 0);
    *S = State{{1, root.max_nodes, 0, 1, root.refused || wide, 0, root.total0, 0}, 1, w};
    a.beam[q * a.max_width] = 0;
    a.counts[q] = 0;
    if constexpr (CACHE) {
        at.hit[q] = hit;
        if (hit.entry != cache::MISS && !wide) cache::ended_cached(a, q, S, at, hit, 0, 0, root.total0, 1, 0, 0);
    }
}

template <int NW, class... At>
__global__ __launch_bounds__(TPB) void beam_begin_kernel(Args a, const int32_t* widths, At... at) {
    begin_body<NW, sizeof...(At) != 0>(a, widths, cache::attach_of(at...));
}

template <int NW, bool CACHE>
__device__ __forceinline__ void expand_body(const Args& a, const cache::Attach& at) {
    __shared__ Lds r;
    __shared__ uint32_t s_dec[3];    // verdict kind, children looked at, new nodes

    const int tid = threadIdx.x, lane = tid & (WAVE - 1), wid = tid / WAVE;
    const int64_t q = blockIdx.x;
    const int L = a.L, kw = a.kw;
    const bool cyc = a.cyc != 0;
    State* S = a.state + q;
    if (S->done) return;  // (its count is 0 since it ended)
    uint64_t* store = a.store + q * a.rows * kw;
    uint32_t* meta = a.meta + q * a.rows;
    uint64_t* table = a.table + q * (int64_t)a.nb * BUCKET;
    const uint32_t* beam = a.beam + q * a.max_width;
    uint64_t* ck = keys_of<NW>(a, q);

    int64_t n_nodes = S->n_nodes, steps = S->steps;
    const int64_t max_nodes = S->max_nodes;
    const int beam_n = S->beam_n;
    uint32_t running = S->running;
    if (tid == 0) r.s_over = 0;
    __syncthreads();  // the state is read before thread 0 rewrites it
    if (n_nodes >= max_nodes || beam_n < 1) {  // the reference's loop condition
        if (tid == 0) ended(a, q, S, beam_n < 1 ? ACX_BFS_EXHAUSTED : ACX_BFS_BUDGET, 0, 0, n_nodes, steps, running, 0);
        return;
    }
    ++steps;
    const int64_t cand_base = n_nodes;
    int32_t status = 0, succ_act = 0;
    int64_t succ_node = 0;
    bool cached = false;  // the pass's "success" child is a cache hit
    cache::Hit hit{cache::MISS, 0, 0};
    uint32_t hit_tot = 0;

    for (int base = 0; base < beam_n; base += RP) {
        const int P = beam_n - base < RP ? beam_n - base : RP;
        const int nch = 12 * P;
        reset(r);
        __syncthreads();
        expand<NW>(r, ck, store, P, L, kw, cyc, [&](int p) {
            const int64_t pn = beam[base + p];
            return pn < a.rows ? pn : 0;
        });
        __syncthreads();
        if constexpr (CACHE) {
            __shared__ uint32_t s_hit;
            __shared__ cache::Hit s_rec;
            if (tid == 0) s_hit = NONE;
            __syncthreads();
            const uint32_t end0 = min(min(r.s_succ, r.s_err), (uint32_t)nch);
            for (uint32_t c = (uint32_t)wid; c < end0; c += TPB / WAVE) {
                if (c >= __hip_atomic_load(&s_hit, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP)) break;  // (uniform in the wave)
                const cache::Hit h = cache::probe<NW + 1>(at.view, ck + c * kw, kw, L, lane);
                if (h.entry == cache::MISS) continue;
                if (lane == 0) atomicMin(&s_hit, c);
                break;  // the wave's later children come after this one
            }
            __syncthreads();
            const uint32_t first = s_hit;
            cached = first != NONE;
            if (cached) {  // (uniform) the winner's wave probes it once more and keeps the record
                if (wid == (int)(first % (TPB / WAVE))) {
                    const cache::Hit h = cache::probe<NW + 1>(at.view, ck + first * kw, kw, L, lane);
                    if (lane == 0) s_rec = h;
                }
                if (tid == 0) r.s_succ = first;  // it stands where a trivial child would
                __syncthreads();
                hit = s_rec;
                hit_tot = r.ctot[first];
            }
        }
        insert<NW>(r, ck, store, table, a, n_nodes, nch, kw);
        __syncthreads();
        if (r.s_over) {  // (uniform) cannot happen at load <= 1/2
            status = ACX_MBFS_OVERFLOW;
            break;
        }

        // decide: the survivors per beam entry, and the child that holds the survivor with which
        // total_nodes reaches max_nodes (it lies below end0: only those were inserted)
        if (wid == 0) {
            uint32_t m = 0;
            if (lane < P) {
#pragma unroll
                for (int act = 0; act < 12; ++act) {
                    const int c = lane * 12 + act;
                    if (r.cand[c] && !r.lost[c]) m |= 1u << act;
                }
            }
            const uint32_t cnt = __popc(m);
            const uint32_t x = wave_incl_sum(cnt, lane);
            const uint32_t total = __shfl(x, WAVE - 1, WAVE);
            const int64_t need = max_nodes - n_nodes;  // > 0
            const unsigned long long cutb = __ballot((int64_t)x >= need);
            uint32_t cutc = NONE;
            if (cutb) {
                const int cutp = __builtin_ctzll(cutb);
                uint32_t act = 0;
                if (lane == cutp) {  // its (need - survivors before it)-th survivor
                    uint32_t mm = m;
                    for (int64_t k = need - (int64_t)(x - cnt); k > 1; --k) mm &= mm - 1;
                    act = (uint32_t)__builtin_ctz(mm);
                    m &= (2u << act) - 1u;
                } else if (lane > cutp) {
                    m = 0;
                }
                cutc = 12u * (uint32_t)cutp + (uint32_t)__shfl((int)act, cutp, WAVE);
            }
            r.pmask[lane] = m;
            r.pexcl[lane] = x - cnt;
            if (lane == 0) {
                const uint32_t s_succ = r.s_succ, s_err = r.s_err, end0 = min(s_succ, s_err);
                uint32_t kind = 0, looked = (uint32_t)nch;
                if (cutb) {
                    kind = ACX_BFS_BUDGET;
                    looked = cutc + 1;
                } else if (end0 != NONE) {  // (a move either raises or returns a child: err != succ)
                    kind = s_err < s_succ ? ACX_BFS_MOVE_ERROR : ACX_BFS_FOUND;
                    looked = s_err < s_succ ? s_err : s_succ + 1;
                }
                s_dec[0] = kind;
                s_dec[1] = looked;
                s_dec[2] = cutb ? (uint32_t)need : total;
                r.s_min = NONE;
            }
        }
        __syncthreads();
        const uint32_t kind = s_dec[0], s_end = s_dec[1], newn = s_dec[2];

        // the survivors (up to the cut) become nodes in sequential order
        if (kind == 0 || kind == ACX_BFS_BUDGET)
            commit<NW>(r, ck, store, meta, table, a, n_nodes, nch, kw, [&](int p) { return beam[base + p]; });
        min_upto(r, nch, s_end);
        __syncthreads();
        running = min(running, r.s_min);
        n_nodes += newn;
        if (kind != ACX_BFS_FOUND) cached = false;  // a budget cut came first: the hit is never looked at
        if (kind == ACX_BFS_FOUND || kind == ACX_BFS_MOVE_ERROR) {
            status = (int32_t)kind;
            if (kind == ACX_BFS_FOUND) {
                succ_node = beam[base + (s_end - 1) / 12];
                succ_act = (int32_t)((s_end - 1) % 12);
            }
            break;
        }
        if (kind == ACX_BFS_BUDGET) break;  // the candidates are still scored and selected
    }

    if (tid != 0) return;
    const int64_t cand_n = n_nodes - cand_base;
    if (status != 0) {
        // the edges to the success child's parent + (action, 2)
        const int64_t plen = status == ACX_BFS_FOUND ? batch::path_depth(meta, succ_node, a.rows) + 1 : 0;
        if (CACHE && cached && status == ACX_BFS_FOUND)
            cache::ended_cached(a, q, S, at, hit, succ_act, succ_node, hit_tot, n_nodes, steps, plen);
        else
            ended(a, q, S, status, succ_act, succ_node, n_nodes, steps, running, plen);
    } else if (cand_n == 0) {  // the beam died
        ended(a, q, S, ACX_BFS_EXHAUSTED, 0, 0, n_nodes, steps, running, 0);
    } else {
        S->n_nodes = n_nodes;
        S->steps = steps;
        S->cand_base = cand_base;
        S->cand_n = (int32_t)cand_n;
        S->running = running;
        a.counts[q] = (int32_t)cand_n;
    }
}

template <int NW, class... At>
__global__ __launch_bounds__(TPB) void beam_expand_kernel(Args a, At... at) {
    expand_body<NW, sizeof...(At) != 0>(a, cache::attach_of(at...));
}

template <int CAP, int THREADS>
__global__ __launch_bounds__(THREADS) void beam_select_kernel(Args a, const float* scores, int64_t M) {
    __shared__ uint64_t sk[CAP];
    __shared__ uint32_t s_nan;
    const int tid = threadIdx.x;
    const int64_t q = blockIdx.x;
    State* S = a.state + q;
    const int n = a.counts[q];  // 0 for a search that has ended
    const int64_t off = a.offsets[q];
    if (n <= 0 || n > CAP || off < 0 || off + n > M) return;
    int n2 = 1;
    while (n2 < n) n2 <<= 1;
    if (tid == 0) s_nan = 0;
    __syncthreads();
    for (int i = tid; i < n2; i += THREADS) {
        uint64_t k = ~0ull;  // padding sorts last
        if (i < n) {
            const uint32_t bits = __float_as_uint(scores[off + i]);
            if (score_is_nan(bits)) s_nan = 1;
            k = sort_key(bits, (uint32_t)i);
        }
        sk[i] = k;
    }
    __syncthreads();
    if (s_nan) {  // (uniform) sticky: the search has ended, nothing is selected
        if (tid == 0) ended(a, q, S, ACX_BEAM_NAN, 0, 0, S->n_nodes, S->steps, S->running, 0);
        return;
    }
    for (int k = 2; k <= n2; k <<= 1) {
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int t = tid; t < n2 / 2; t += THREADS) {
                const int i = ((t & ~(j - 1)) << 1) | (t & (j - 1)), p = i | j;  // the pair (i, i + j)
                const uint64_t x = sk[i], y = sk[p];
                if ((x > y) == ((i & k) == 0)) {
                    sk[i] = y;
                    sk[p] = x;
                }
            }
            __syncthreads();
        }
    }
    const int w = S->width < n ? S->width : n;
    uint32_t* beam = a.beam + q * a.max_width;
    const uint32_t cand_base = (uint32_t)S->cand_base;
    for (int i = tid; i < w && i < a.max_width; i += THREADS) beam[i] = cand_base + (uint32_t)sk[i];
    if (tid == 0) S->beam_n = w;
}

// what the handle (acx_batch.h) and the step frame (acx_scored.h) need of this engine; max_width is
// set before arrays() is called
struct Engine {
    using Args = beam::Args;
    // a found search's path (value_guided_search.py:87-97,497-498): the edges + (action, 2), no root entry
    // a search that ended on a cache hit below the root: the edges + the (action, total) of the child that hit
    static constexpr uint32_t WITH_PATH = 1u << ACX_BFS_FOUND | 1u << ACX_BFS_CACHED;
    static constexpr bool ROOT_ENTRY = false;
    static constexpr int GATHER_THREADS = TPB, MOST = 0;
    static constexpr bool LIVE = false;
    static int64_t rows_for(int64_t B) { return B; }
    static uint32_t buckets_for(int64_t B) { return round::buckets_for(B); }
    template <class F>
    static void arrays(Args& a, F f) {
        round::arrays(a, f);
        f(a.beam, 4 * (size_t)a.max_width, false);
        scored::arrays(a, f);
    }
};
static_assert(sizeof(State) == 56 && scored::RECORD<State> == 140, "the bytes formula of include/acx.h");

static bool shape(Args& a, int32_t L, int64_t B, int32_t W, int32_t cyclical) {
    if (W < 1 || W > ACX_BEAM_MAX_WIDTH) return false;
    a.max_width = W;
    return batch::shape<Engine>(a, L, B, cyclical);
}

}  // namespace beam
}  // namespace acx

namespace beam = acx::beam;
namespace batch = acx::batch;
namespace scored = acx::scored;

extern "C" {

int64_t acx_beam_bytes(int32_t L, int64_t max_nodes_each, int32_t max_width) {
    beam::Args a{};
    return beam::shape(a, L, max_nodes_each, max_width, 0) ? batch::bytes_of<beam::Engine>(a) : ACX_E_ARG;
}

void* acx_beam_create(int32_t L, int64_t n_searches, int64_t max_nodes_each, int32_t max_width, int32_t cyclical) {
    beam::Args a{};
    if (!beam::shape(a, L, max_nodes_each, max_width, cyclical)) return nullptr;
    return batch::create_from<beam::Engine>(a, n_searches);
}

void acx_beam_destroy(void* h) { batch::destroy<beam::Engine>(h); }

int acx_beam_begin(void* h, const int32_t* states, const int64_t* budgets, const int32_t* widths, int64_t n,
                   void* stream) {
    return scored::begin<beam::Engine>(h, states, budgets, widths != nullptr, n, stream,
                                       [=](auto nw, const beam::Args& a, auto... at) {
        beam::beam_begin_kernel<decltype(nw)::value>
            <<<dim3((unsigned)a.n), dim3(acx::bfs::TPB), 0, (hipStream_t)stream>>>(a, widths, at...);
    });
}

int acx_beam_set_cache(void* h, void* cache) { return acx::cache::set_cache<batch::Handle<beam::Engine>>(h, cache); }

int acx_beam_cache_hits(void* h, int64_t n, int64_t* entry, int32_t* rel, int32_t* k, void* stream) {
    return acx::cache::read_hits<batch::Handle<beam::Engine>>(h, n, entry, rel, k, stream);
}

int acx_beam_expand(void* h, int64_t* total, void* stream) {
    return scored::make<beam::Engine>(h, total, stream, [=](auto nw, const beam::Args& a, auto... at) {
        beam::beam_expand_kernel<decltype(nw)::value>
            <<<dim3((unsigned)a.n), dim3(acx::bfs::TPB), 0, (hipStream_t)stream>>>(a, at...);
    });
}

int acx_beam_gather(void* h, uint64_t* keys, int64_t M, void* stream) {
    return scored::gather<beam::Engine>(h, keys, M, stream);
}

int acx_beam_select(void* h, const float* scores, int64_t M, void* stream) {
    return scored::take<beam::Engine>(h, scores, M, stream, [=](const beam::Args& a, hipStream_t st) {
        const int most = 12 * a.max_width;  // candidates of a step
        if (most <= 1024) beam::beam_select_kernel<1024, 256><<<dim3((unsigned)a.n), dim3(256), 0, st>>>(a, scores, M);
        else if (most <= 4096) beam::beam_select_kernel<4096, 1024><<<dim3((unsigned)a.n), dim3(1024), 0, st>>>(a, scores, M);
        else beam::beam_select_kernel<16384, 1024><<<dim3((unsigned)a.n), dim3(1024), 0, st>>>(a, scores, M);
    });
}

int acx_beam_finish(void* h, int32_t* status, int64_t* nodes, int64_t* steps, int32_t* min_length, int64_t* path_len,
                    void* stream) {
    return scored::finish<beam::Engine>(h, status, nodes, steps, min_length, path_len, stream);
}

int acx_beam_paths(void* h, int64_t n, const int64_t* offsets, int32_t* actions, int32_t* totals, int64_t cap,
                   void* stream) {
    return batch::paths<beam::Engine>(h, n, offsets, actions, totals, cap, stream);
}

}  // extern "C"
