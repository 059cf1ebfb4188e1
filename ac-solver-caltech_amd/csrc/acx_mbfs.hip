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
//   scratch (768, kw) uint64  only for L > 64: the round's child keys.
// B = max_nodes_each.  Bytes per search (acx_mbfs_bytes):
//   8 kw B + 4 B + 64 ceil((B + 779) / 4) + 32 [+ 6144 kw when L > 64],   kw = acx_key_words(L).
//
// A round (acx_round.h) takes the next P <= 64 parents, nodes head .. head + P.  Its decide is
// wave 0's: survivors per parent, their prefix sum, the first parent after which len(tree_nodes) >=
// max_nodes, and the reference's verdict for the round (chunk_verdict, acx_bfs_verdict.h: raising
// child / success / budget cut, the earliest in sequential order; otherwise the next round, or
// queue exhaustion).  A round with a verdict appends nothing, so a search holds fewer than
// max_nodes nodes and the store needs B rows.  Every loop is bounded: rounds by max_nodes (each
// expands >= 1 of fewer than max_nodes nodes), probes by nb, the path walks by the node count.
//
// The frame around the round -- the root and its refusal statuses, the table view with its
// workgroup-scope reads (node codes in acx_bfs.hip are permanent, which is why its plain bucket
// loads are safe there; a round code here means another node a round later), the result record,
// the path reader and the reusable handle behind acx_mbfs_* -- is acx_batch.h.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "acx.h"

#include "acx_bfs_verdict.h"
#include "acx_round.h"

namespace acx {
namespace mbfs {

using namespace acx::round;

struct Args : round::Args {};

template <int NW>
__global__ __launch_bounds__(TPB) void mbfs_kernel(Args a) {
    __shared__ Lds r;
    __shared__ uint32_t s_dec[4];    // verdict kind, children looked at, last parent, new nodes

    const int tid = threadIdx.x, lane = tid & (WAVE - 1), wid = tid / WAVE;
    const int64_t q = blockIdx.x;
    const int L = a.L, kw = a.kw;
    const bool cyc = a.cyc != 0;
    uint64_t* store = a.store + q * a.rows * kw;
    uint32_t* meta = a.meta + q * a.rows;
    uint64_t* table = a.table + q * (int64_t)a.nb * BUCKET;
    uint64_t* ck = keys_of<NW>(a, q);

    if (tid == 0) r.s_over = 0;
    const batch::Root root = batch::root_setup<TPB, NW>(a, q, store, meta, table);
    if (root.refused) return;
    const int64_t max_nodes = root.max_nodes;
    __syncthreads();

    int64_t head = 0, n_nodes = 1, parents = 0, succ_node = 0;
    int32_t status = ACX_MBFS_OVERFLOW, succ_act = 0;
    uint32_t running = root.total0;

    for (int64_t round = 0; round <= max_nodes; ++round) {
        const int P = (int)(n_nodes - head < RP ? n_nodes - head : RP);
        const int nch = 12 * P;
        reset(r);
        __syncthreads();
        expand<NW>(r, ck, store, P, L, kw, cyc, [&](int p) { return head + p; });
        __syncthreads();
        insert<NW>(r, ck, store, table, a, n_nodes, nch, kw);
        __syncthreads();
        if (r.s_over) break;  // (uniform) cannot happen at load <= 1/2

        // decide
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
            r.pmask[lane] = m;
            r.pexcl[lane] = x - cnt;
            const uint32_t total = __shfl(x, WAVE - 1, WAVE);
            // the first parent after which len(tree_nodes) >= max_nodes
            const unsigned long long cutb = __ballot(lane < P && n_nodes + (int64_t)x >= max_nodes);
            const uint32_t cutp = cutb ? (uint32_t)__builtin_ctzll(cutb) : NONE;
            const uint32_t at_cut = __shfl(x, cutb ? (int)cutp : 0, WAVE);
            const Verdict v = chunk_verdict(r.s_succ, r.s_err, cutp, (uint32_t)P);
            if (lane == 0) {
                s_dec[0] = (uint32_t)v.kind;
                s_dec[1] = v.looked;
                s_dec[2] = v.last_p;
                s_dec[3] = v.kind == ACX_BFS_BUDGET ? at_cut : total;
                r.s_min = NONE;
            }
        }
        __syncthreads();
        const uint32_t kind = s_dec[0], s_end = s_dec[1], last_p = s_dec[2], newn = s_dec[3];

        if (kind == 0)
            commit<NW>(r, ck, store, meta, table, a, n_nodes, nch, kw, [&](int p) { return (uint32_t)(head + p); });
        min_upto(r, nch, s_end);
        __syncthreads();
        running = min(running, r.s_min);
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
        // [(-1, total0)] + the edges to the success child's parent + (action, 2)
        const int64_t plen = status == ACX_BFS_FOUND ? batch::path_depth(meta, succ_node, a.rows) + 2 : 0;
        batch::write_result(a, q, Res{status, succ_act, succ_node, 2, 0, n_nodes}, parents, running, plen);
    }
}

// what the handle (acx_batch.h) needs of this engine
struct Engine {
    using Args = mbfs::Args;
    static constexpr uint32_t WITH_PATH = 1u << ACX_BFS_FOUND;
    static constexpr bool ROOT_ENTRY = true;
    static int64_t rows_for(int64_t B) { return B; }
    static uint32_t buckets_for(int64_t B) { return round::buckets_for(B); }
    template <class F>
    static void arrays(Args& a, F f) { round::arrays(a, f); }
    template <int NW>
    static void launch(const Args& a, int64_t n, hipStream_t st) {
        mbfs_kernel<NW><<<dim3((unsigned)n), dim3(TPB), 0, st>>>(a);
    }
};

}  // namespace mbfs
}  // namespace acx

using acx::mbfs::Engine;
namespace batch = acx::batch;

extern "C" {

int64_t acx_mbfs_bytes(int32_t L, int64_t max_nodes_each) { return batch::bytes<Engine>(L, max_nodes_each); }

void* acx_mbfs_create(int32_t L, int64_t n_searches, int64_t max_nodes_each, int32_t cyclical) {
    return batch::create<Engine>(L, n_searches, max_nodes_each, cyclical);
}

void acx_mbfs_destroy(void* h) { batch::destroy<Engine>(h); }

int acx_mbfs_run(void* h, const int32_t* states, const int64_t* budgets, int64_t n, int32_t* status, int64_t* nodes,
                 int64_t* parents, int32_t* min_length, int64_t* path_len, void* stream) {
    return batch::run<Engine>(h, states, budgets, n, status, nodes, parents, min_length, path_len, stream);
}

int acx_mbfs_paths(void* h, int64_t n, const int64_t* offsets, int32_t* actions, int32_t* totals, int64_t cap,
                   void* stream) {
    return batch::paths<Engine>(h, n, offsets, actions, totals, cap, stream);
}

}  // extern "C"
