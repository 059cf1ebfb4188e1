// acx_round.h -- a round: at most 64 parents of one search expanded, deduplicated and appended by
// the search's workgroup of 256 threads, over the search's private store, meta and visited set
// (acx_batch.h).  acx_mbfs.hip runs rounds over its queue, acx_beam.hip over its beam ("a pass").
//
// A round takes P <= 64 parents and runs, with a barrier between:
//   reset   the round's LDS state (Lds, below);
//   expand  lane = parent, wave w makes actions 3w..3w+2 (child_of, acx_bfs_common.h); the 768
//           child keys go to LDS in sequential order s = 12 p + a (L <= 64: at most 30 KiB; above
//           that 54 KiB of LDS would halve the workgroups per CU, so they go to the search's
//           scratch in HBM); first success and first raising child by LDS atomicMin;
//   insert  thread per child s below the first success / raising child: visited::insert; a code
//           below n (the nodes before the round) names a stored node, a code n + s a child of this
//           round, so the full key is compared in the store or in the round's keys.  The first
//           occurrence holds the entry, the child it replaced is told (`lost`).  A probe that has
//           walked all nb buckets sets s_over;
//   decide  the engine's own: wave 0 turns cand & ~lost into the survivors per parent (pmask),
//           their exclusive prefix sum (pexcl) and its verdict, and sets s_min = NONE;
//   commit  the survivors in pmask are appended in (parent, action) order with their meta word,
//           and each one's table entry is rewritten from its round code to its node index;
//   min_upto  the minimum child total up to the ending event goes to s_min.
// The engine owns the loop around the round, the barriers, decide, and whether a round with a
// verdict commits.  The insert call is written here for the two engines whose parents come 64 at a
// time; mgreedy's (one wave, one parent) stays in acx_mgreedy.hip, where as a shared routine it
// cost mgreedy_kernel<8> 14 VGPRs.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "acx.h"
#include "acx_moves.h"

#include "acx_batch.h"
#include "acx_bfs_common.h"
#include "acx_visited.h"

namespace acx {
namespace round {

using namespace acx::bfs;
using batch::Buckets;
using batch::Res;
using visited::BUCKET;

constexpr int RP = 64;       // parents per round
constexpr int RC = 12 * RP;  // children per round

// the round's child keys stay in LDS up to four letter words (L <= 64)
template <int NW>
constexpr bool LDS_KEYS = NW <= 4;

struct Args : batch::Args {
    uint64_t* scratch;  // (768, kw) per search, only for L > 64: the round's child keys
};

// load <= 1/2 with a whole round's children in the table
inline uint32_t buckets_for(int64_t B) { return (uint32_t)((2 * (B + 11 + RC) + BUCKET - 1) / BUCKET); }

// the arrays every round engine has, for its Engine::arrays (acx_batch.h)
template <class A, class F>
void arrays(A& a, F f) {
    const size_t R = (size_t)a.rows, kw = (size_t)a.kw;
    f(a.store, 8 * kw * R, false);
    f(a.meta, 4 * R, false);
    f(a.table, 8 * (size_t)BUCKET * a.nb, true);
    f(a.res, sizeof(Res), true);
    f(a.scratch, a.L > 64 ? 8 * kw * RC : 0, false);  // the round's child keys where they do not stay in LDS
}

// the round's state: one __shared__ object per kernel.  (The round's keys, where they stay in LDS,
// are an array of their own, keys_of(): as a member of this object they cost mbfs_kernel<2> two
// VGPRs, 92 -> 94, one more than before the round was shared.)
struct Lds {
    uint32_t slot[RC];  // table index of the entry a child holds
    uint16_t ctot[RC];  // child total, 0xffff: the move raised (or no such child)
    uint8_t cand[RC];   // the child holds its state's entry after its own probe
    uint8_t lost[RC];   // an earlier child of the round took that entry
    uint32_t pmask[RP], pexcl[RP];
    uint32_t s_succ, s_err, s_min, s_over;
};

// where search q's round keys are
template <int NW>
__device__ __forceinline__ uint64_t* keys_of(const Args& a, int64_t q) {
    if constexpr (LDS_KEYS<NW>) {
        __shared__ uint64_t kl[RC * (NW + 1)];
        return kl;
    } else {
        return a.scratch + q * (int64_t)RC * a.kw;
    }
}

__device__ __forceinline__ void reset(Lds& r) {
    for (int c = threadIdx.x; c < RC; c += TPB) {
        r.cand[c] = 0;
        r.lost[c] = 0;
        r.ctot[c] = 0xffffu;
    }
    if (threadIdx.x == 0) r.s_succ = r.s_err = NONE;
}

// row_of(lane): the store row of the lane's parent
template <int NW, class RowOf>
__device__ __forceinline__ void expand(Lds& r, uint64_t* ck, const uint64_t* store, int P, int L, int kw, bool cyc,
                                       RowOf row_of) {
    const int lane = threadIdx.x & (WAVE - 1), wid = threadIdx.x / WAVE;
    uint32_t succ = NONE, err = NONE;
    if (lane < P) {
        PresRegs<NW> pr;
        load_key<NW>(store + row_of(lane) * kw, kw, L, pr);
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
                r.ctot[s] = (uint16_t)tot;
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
        if (succ != NONE) atomicMin(&r.s_succ, succ);
        if (err != NONE) atomicMin(&r.s_err, err);
    }
}

// the children below the success / raising child (it ends the search, later ones are not looked
// at) of a round that began with n_nodes nodes
template <int NW>
__device__ __forceinline__ void insert(Lds& r, const uint64_t* ck, const uint64_t* store, uint64_t* table,
                                       const Args& a, int64_t n_nodes, int nch, int kw) {
    const uint32_t end0 = min(r.s_succ, r.s_err);
    const uint64_t NB = (uint64_t)n_nodes;
    for (int c = threadIdx.x; c < nch; c += TPB) {
        if ((uint32_t)c >= end0) continue;
        const uint64_t code = NB + (uint64_t)c;
        const Key<NW + 1> key = kload<NW + 1>(ck + c * kw, kw);
        const visited::Outcome ins = visited::insert(
            Buckets{table, a.nb}, a.ep, code, khash<NW + 1>(key, kw),
            [&](uint64_t vc) {
                return vc < NB ? keq<NW + 1>(store + vc * kw, key, kw) : keq<NW + 1>(ck + (vc - NB) * kw, key, kw);
            },
            [&](uint32_t sl, uint64_t displaced) {  // a later child of the round that held it learns it lost
                r.slot[c] = sl;
                const uint64_t lc = displaced - NB;
                if (displaced != visited::NO_CODE && lc < (uint64_t)RC) r.lost[lc] = 1;
            });
        if (ins == visited::FULL) r.s_over = 1;
        r.cand[c] = ins == visited::HELD;
    }
}

// parent_of(p): the node index of the round's parent p, for the survivors' meta words
template <int NW, class ParentOf>
__device__ __forceinline__ void commit(Lds& r, const uint64_t* ck, uint64_t* store, uint32_t* meta, uint64_t* table,
                                       const Args& a, int64_t n_nodes, int nch, int kw, ParentOf parent_of) {
    for (int c = threadIdx.x; c < nch; c += TPB) {
        const int p = c / 12, act = c - 12 * p;
        const uint32_t m = r.pmask[p];
        if (!((m >> act) & 1u)) continue;
        const int64_t pos = n_nodes + r.pexcl[p] + __popc(m & ((1u << act) - 1u));
        if (pos >= a.rows) continue;  // (never: a search holds at most max_nodes <= rows nodes)
        for (int k = 0; k < kw; ++k) store[pos * kw + k] = ck[c * kw + k];
        meta[pos] = (parent_of(p) << 4) | (uint32_t)act;
        batch::recode_entry(table, r.slot[c], (uint64_t)pos);
    }
}

// the running minimum takes the totals of the children below s_end
__device__ __forceinline__ void min_upto(Lds& r, int nch, uint32_t s_end) {
    uint32_t m = NONE;
    for (int c = threadIdx.x; c < nch; c += TPB)
        if ((uint32_t)c < s_end) m = min(m, (uint32_t)r.ctot[c]);
    m = wave_min(m);
    if ((threadIdx.x & (WAVE - 1)) == 0 && m != NONE) atomicMin(&r.s_min, m);
}

}  // namespace round
}  // namespace acx
