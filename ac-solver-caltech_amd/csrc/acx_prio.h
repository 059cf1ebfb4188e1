// acx_prio.h -- the greedy frontier's order on packed keys (acx_key.h), for the host compiler and
// for hipcc (host and device): Python's order on (total, path length, tuple(state)) of
// ac_solver/search/greedy.py:55-64,104-113, with letters compared as the integers
// -2 < -1 < 0 (padding) < 1 < 2, r0 before r1.  It is the unsigned word order of prio_key
// (acx_frontier.h), taken directly on the packed key plus (total, depth) -- no expanded priority
// key is built, so the batched greedy kernel (acx_mgreedy.hip) and a CPU test
// (tests/prio_check.cpp) run the same code.
#pragma once
#include <stdint.h>

#include "acx_key.h"

namespace acx {

// a letter's rank by its 2-bit code (x = 0, x^-1 = 1, y = 2, y^-1 = 3): y^-1 0, x^-1 1, x 3, y 4;
// padding ranks 2, between the inverses and the generators
constexpr uint32_t PRIO_PAD = 2;
ACX_HD inline uint32_t prio_rank(uint32_t code) { return (0x0413u >> (4 * code)) & 7u; }

// rank of position i of relator h, which holds n letters
ACX_HD inline uint32_t prio_rank_at(const uint64_t* k, int L, int h, int i, int n) {
    return i < n ? prio_rank(key_code_at(k, L, h, i)) : PRIO_PAD;
}

// The order's leading 64 bits: total (9 bits) | path length (31) | the ranks of the first
// min(8, 2L) positions of r0 r1, 3 bits each, MSB first -- prio_key's first word.  Monotone in the
// full order, so two entries whose k0 differ are ordered by k0 alone.
ACX_HD inline uint64_t prio_k0(const uint64_t* k, int L, int tot, int dep) {
    uint64_t v = ((uint64_t)(tot & 0x1ff) << 55) | ((uint64_t)(dep & 0x7fffffff) << 24);
    const int n0 = key_len(k, L, 0), n1 = key_len(k, L, 1);
    for (int p = 0; p < 8 && p < 2 * L; ++p) {
        const int h = p >= L, i = p - h * L;
        v |= (uint64_t)prio_rank_at(k, L, h, i, h ? n1 : n0) << (21 - 3 * p);
    }
    return v;
}

// -1 / 0 / +1: the order of the two keys' state tuples.  Per relator: below the shorter length the
// first differing code decides (one XOR and count-trailing-zeros per 64-bit word); if none does
// and the lengths differ, the shorter relator's first padding meets a letter of the longer one.
ACX_HD inline int prio_cmp_states(const uint64_t* a, const uint64_t* b, int L) {
    for (int h = 0; h < 2; ++h) {
        const int na = key_len(a, L, h), nb = key_len(b, L, h);
        const int m = na < nb ? na : nb;
        const int lo = 2 * h * L, hi = lo + 2 * m;  // the code bits of letters [0, m)
        for (int w = lo >> 6; (w << 6) < hi; ++w) {
            const int b0 = w << 6;
            uint64_t x = a[w] ^ b[w];
            if (lo > b0) x &= ~0ull << (lo - b0);
            if (hi < b0 + 64) x &= (1ull << (hi - b0)) - 1;
            if (x) {
                const int bit = __builtin_ctzll(x) & ~1;
                const uint32_t ra = prio_rank((uint32_t)(a[w] >> bit) & 3u);
                const uint32_t rb = prio_rank((uint32_t)(b[w] >> bit) & 3u);
                return ra < rb ? -1 : 1;
            }
        }
        if (na < nb) return PRIO_PAD < prio_rank(key_code_at(b, L, h, m)) ? -1 : 1;
        if (nb < na) return prio_rank(key_code_at(a, L, h, m)) < PRIO_PAD ? -1 : 1;
    }
    return 0;
}

// (total, depth, state) of a before that of b
ACX_HD inline bool prio_less(const uint64_t* a, int tot_a, int dep_a, const uint64_t* b, int tot_b, int dep_b, int L) {
    if (tot_a != tot_b) return tot_a < tot_b;
    if (dep_a != dep_b) return dep_a < dep_b;
    return prio_cmp_states(a, b, L) < 0;
}

}  // namespace acx
