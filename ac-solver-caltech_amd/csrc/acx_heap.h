// acx_heap.h -- the frontier of the heap engines (acx_mgreedy.hip, acx_vgreedy.hip): an implicit
// min-heap of fan-out 64 owned by one wave, in two arrays of a search's slice,
//   hk  (R) uint64   the entry's sort word,
//   hid (R) uint32   the node it names;
// entry i's children are 64 i + 1 .. 64 i + 64, so a level is one coalesced load (lane = child) and
// a wave minimum of hk by shuffles, and 5 levels hold more than 2^24 + 11 entries.
//
// The engine supplies the order of two entries, an object with
//   less(ka, va, kb, vb)    (ka, node va) goes before (kb, node vb);
//   winner(tied, lane, v)   the lane that holds the least entry among the lanes `tied` (at least
//                           one), which all hold the wave's smallest hk; v is the lane's own node.
//                           Every lane calls it and gets the same answer.
// The order must be total on the entries of one heap.  A lane without an entry holds (~0, NONE): no
// entry's hk is all ones.  take and push are called by the whole wave, between the caller's barriers.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "acx_bfs_common.h"

namespace acx {
namespace heap {

using namespace acx::bfs;

constexpr int FAN = 64;    // heap fan-out = lanes of the wave
constexpr int LEVELS = 5;  // 1 + 64 + 64^2 + 64^3 + 64^4 > 2^24 + 11 entries
static_assert(FAN == WAVE, "one lane per child of an entry");

__device__ __forceinline__ uint64_t shfl_xor64(uint64_t v, int o) {
    const uint32_t lo = (uint32_t)__shfl_xor((int)(uint32_t)v, o, WAVE);
    const uint32_t hi = (uint32_t)__shfl_xor((int)(uint32_t)(v >> 32), o, WAVE);
    return (uint64_t)lo | ((uint64_t)hi << 32);
}

__device__ __forceinline__ uint64_t wave_min64(uint64_t v) {
#pragma unroll
    for (int o = 1; o < WAVE; o <<= 1) {
        const uint64_t w = shfl_xor64(v, o);
        v = w < v ? w : v;
    }
    return v;
}

// The minimum of a heap that had hn + 1 entries leaves it (the caller has read hid[0]): the last
// entry sifts down from the root, at most LEVELS steps.
template <class Order>
__device__ __forceinline__ void take(uint64_t* hk, uint32_t* hid, int64_t hn, int lane, const Order& order) {
    if (hn <= 0) return;
    const uint64_t xk = hk[hn];
    const uint32_t xv = hid[hn];
    int64_t i = 0;
    for (int lvl = 0; lvl < LEVELS; ++lvl) {
        const int64_t c0 = (int64_t)FAN * i + 1;
        if (c0 >= hn) break;
        const int64_t c = c0 + lane;
        const bool has = c < hn;
        const uint64_t k = has ? hk[c] : ~0ull;
        uint32_t v = has ? hid[c] : NONE;
        // the smallest hk by shuffles alone; the order decides among the lanes that tie on it
        // (lane 0 holds an entry: c0 < hn)
        const uint64_t kmin = wave_min64(k);
        const uint32_t cl = order.winner(__ballot(has && k == kmin), lane, v);
        v = (uint32_t)__shfl((int)v, (int)cl, WAVE);
        if (!order.less(kmin, v, xk, xv)) break;
        if (lane == 0) {
            hk[i] = kmin;
            hid[i] = v;
        }
        i = c0 + cl;
    }
    if (lane == 0) {
        hk[i] = xk;
        hid[i] = xv;
    }
}

// The cnt <= 12 new leaves of a heap of hn entries enter it.  They are written already: the lanes of
// the mask m (`alive`: this lane is one) hold them in lane order, the lane of rank r in m the leaf
// in slot hpos = hn + r with sort word myk and node vbase + r.  They sit under at most two heap
// parents (12 < 64).  Per parent: while the smallest of its new leaves beats the entry in the
// parent's slot, lane 0 sifts that leaf up from its slot (the parent's entry moves into the leaf;
// what settles in the parent's slot is smaller than what was there, so the leaves already dealt
// with stay in order); the others are looked at again: mostly one wave minimum per parent.
template <class Order>
__device__ __forceinline__ void push(uint64_t* hk, uint32_t* hid, int64_t hn, uint32_t m, uint32_t cnt, bool alive,
                                     int64_t hpos, uint64_t myk, int64_t vbase, int lane, const Order& order) {
    if (hn + cnt <= 1) return;
    const int64_t pa = ((hn > 1 ? hn : 1) - 1) / FAN, pb = (hn + (int64_t)cnt - 2) / FAN;
    for (int64_t p = pa; p <= pb; ++p) {  // (uniform, at most 2)
        bool cand = alive && hpos >= 1 && (hpos - 1) / FAN == p;
        for (int it = 0; it < 12; ++it) {  // (uniform) each round retires one new leaf
            const uint64_t xk = wave_min64(cand ? myk : ~0ull);
            const unsigned long long tied = __ballot(cand && myk == xk);
            if (!tied) break;  // no leaf left under this parent
            const uint32_t w = order.winner(tied, lane, (uint32_t)(vbase + (hpos - hn)));
            const uint32_t wr = __popc(m & ((1u << w) - 1u));
            const uint32_t xv = (uint32_t)(vbase + wr);
            if (!order.less(xk, xv, hk[p], hid[p])) break;
            if (lane == 0) {
                int64_t i = hn + wr;
                for (int lvl = 0; lvl < LEVELS && i > 0; ++lvl) {
                    const int64_t par = (i - 1) / FAN;
                    const uint64_t pk = hk[par];
                    const uint32_t pv = hid[par];
                    if (!order.less(xk, xv, pk, pv)) break;
                    hk[i] = pk;
                    hid[i] = pv;
                    i = par;
                }
                hk[i] = xk;
                hid[i] = xv;
            }
            cand = cand && (uint32_t)lane != w;
            __syncthreads();
        }
    }
}

}  // namespace heap
}  // namespace acx
