// acx_beam_key.h -- the order of a beam step's scores as an unsigned integer: beam_select_kernel
// (acx_beam.hip) sorts (score_key << 32 | candidate index), which is the reference's stable
// `scored.sort(key=lambda x: x[0])` (value_guided_search.py:539-541) as long as no score is NaN.
// Host / device like acx_bfs_verdict.h: tests/beam_key_check.cpp compiles it with the host compiler.
#pragma once
#include <stdint.h>
#include <string.h>

#include "acx_key.h"

namespace acx {
namespace beam {

// Python cannot order a NaN (its sort's result then depends on where the NaN stands), so a NaN
// score is refused and never keyed
ACX_HD inline bool score_is_nan(uint32_t bits) { return (bits & 0x7fffffffu) > 0x7f800000u; }

// a < b as floats  <=>  score_key(a) < score_key(b), and a == b as floats (-0.0 == +0.0)  <=>
// equal keys, over the finite values, the denormals and +-inf: a negative float's bits order
// backwards, so they are complemented; a non-negative one moves above them all by its sign bit
ACX_HD inline uint32_t score_key(uint32_t bits) {
    if ((bits << 1) == 0) bits = 0;  // -0.0 is +0.0
    return (bits & 0x80000000u) ? ~bits : bits | 0x80000000u;
}

inline uint32_t score_bits(float f) {
    uint32_t u;
    memcpy(&u, &f, 4);
    return u;
}

// what is sorted: unique per candidate, so any correct sort of it is the stable sort by score
ACX_HD inline uint64_t sort_key(uint32_t bits, uint32_t index) { return ((uint64_t)score_key(bits) << 32) | index; }

}  // namespace beam
}  // namespace acx
