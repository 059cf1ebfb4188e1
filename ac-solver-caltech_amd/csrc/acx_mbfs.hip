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
// The frame around the round -- the root and its refusal statuses, the table view with its
// workgroup-scope reads (node codes in acx_bfs.hip are permanent, which is why its plain bucket
// loads are safe there; a round code here means another node a round later), the result record,
// the path reader and the reusable handle behind acx_mbfs_* -- is acx_batch.h, shared with
// acx_mgreedy.hip.  The insert call stays here: as a shared routine it cost mgreedy_kernel<8>
// 14 VGPRs (95 -> 109) in every shape tried.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "acx.h"
#include "acx_moves.h"

#include "acx_batch.h"
#include "acx_bfs_common.h"
#include "acx_bfs_verdict.h"
#include "acx_visited.h"

namespace acx {
namespace mbfs {

using namespace acx::bfs;
using batch::Buckets;
using batch::Res;
using visited::BUCKET;

constexpr int RP = 64;          // parents per round
constexpr int RC = 12 * RP;     // children per round

struct Args : batch::Args {
    uint64_t* scratch;
};

template <int NW>
__global__ __launch_bounds__(TPB) void mbfs_kernel(Args a) {
    constexpr bool LDS_KEYS = NW <= 4;
    __shared__ uint64_t kl[LDS_KEYS ? RC * (NW + 1) : 1];
    __shared__ uint32_t slot[RC];    // table index of the entry a child holds
    __shared__ uint16_t ctot[RC];    // child total, 0xffff: the move raised (or no such child)
    __shared__ uint8_t cand[RC];     // the child holds its state's entry after its own probe
    __shared__ uint8_t lost[RC];     // an earlier child of the round took that entry
    __shared__ uint32_t pmask[RP], pexcl[RP];
    __shared__ uint32_t s_succ, s_err, s_min, s_over;
    __shared__ uint32_t s_dec[4];    // verdict kind, children looked at, last parent, new nodes

    const int tid = threadIdx.x, lane = tid & (WAVE - 1), wid = tid / WAVE;
    const int64_t q = blockIdx.x;
    const int L = a.L, kw = a.kw;
    const bool cyc = a.cyc != 0;
    uint64_t* store = a.store + q * a.rows * kw;
    uint32_t* meta = a.meta + q * a.rows;
    uint64_t* table = a.table + q * (int64_t)a.nb * BUCKET;
    uint64_t* ck;
    if constexpr (LDS_KEYS) ck = kl;
    else ck = a.scratch + q * (int64_t)RC * kw;

    if (tid == 0) s_over = 0;
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
                if (pos >= a.rows) continue;  // (never: a round without a verdict ends below max_nodes)
                for (int k = 0; k < kw; ++k) store[pos * kw + k] = ck[c * kw + k];
                meta[pos] = ((uint32_t)(head + p) << 4) | (uint32_t)act;
                batch::recode_entry(table, slot[c], (uint64_t)pos);
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
        // [(-1, total0)] + the edges to the success child's parent + (action, 2)
        const int64_t plen = status == ACX_BFS_FOUND ? batch::path_depth(meta, succ_node, a.rows) + 2 : 0;
        batch::write_result(a, q, Res{status, succ_act, succ_node, 2, 0, n_nodes}, parents, running, plen);
    }
}

// what the handle (acx_batch.h) needs of this engine
struct Engine {
    using Args = mbfs::Args;
    static constexpr uint32_t WITH_PATH = 1u << ACX_BFS_FOUND;
    static int64_t rows_for(int64_t B) { return B; }
    static uint32_t buckets_for(int64_t B) { return (uint32_t)((2 * (B + 11 + RC) + BUCKET - 1) / BUCKET); }
    template <class F>
    static void arrays(Args& a, F f) {
        const size_t R = (size_t)a.rows, kw = (size_t)a.kw;
        f(a.store, 8 * kw * R, false);
        f(a.meta, 4 * R, false);
        f(a.table, 8 * (size_t)BUCKET * a.nb, true);
        f(a.res, sizeof(Res), true);
        f(a.scratch, a.L > 64 ? 8 * kw * RC : 0, false);  // the round's child keys where they do not stay in LDS
    }
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
