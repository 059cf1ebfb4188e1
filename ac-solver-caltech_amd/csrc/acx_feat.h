// acx_feat.h -- the 14 features of a presentation from its letter counts, for the units that
// compute them on the device: acx_features.hip (acx_features, one lane per row) and acx_vgreedy.hip
// (the fused pop, from a candidate's store row).  The arithmetic, and what is bit-exact in it, is
// described at the top of acx_features.hip.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "acx.h"
#include "acx_moves.h"

namespace acx {
namespace feat {

constexpr int NF = 14;

struct Counts {
    int n[2];       // relator lengths (count_nonzero of each half)
    int c[2][4];    // per relator: count of x, x^-1, y, y^-1 among the first n letters
};

__device__ __forceinline__ void write_features(const Counts& k, float* out, const float* mean, const float* stdv) {
    const int n0 = k.n[0], n1 = k.n[1], tot = n0 + n1;
    const int ex = (k.c[0][0] - k.c[0][1]) + (k.c[1][0] - k.c[1][1]);
    const double ratio = tot > 0 ? (double)n0 / (double)tot : 0.5;
    const int mn = n0 < n1 ? n0 : n1, mx = n0 < n1 ? n1 : n0;
    const double mmr = mn > 0 ? (double)mx / (double)mn : (double)mx;
    float f[NF] = {(float)tot,       (float)n0,        (float)n1,        (float)k.c[0][0], (float)k.c[0][1],
                   (float)k.c[0][2], (float)k.c[0][3], (float)k.c[1][0], (float)k.c[1][1], (float)k.c[1][2],
                   (float)k.c[1][3], (float)ex,        (float)ratio,     (float)mmr};
#pragma unroll
    for (int i = 0; i < NF; ++i) {
        float v = f[i];
        if (mean) v = (v - mean[i]) / stdv[i];
        out[i] = v;
    }
}

// count of 2-bit fields equal to `code` among the first n letters of w
template <int NW>
__device__ __forceinline__ int count_code(const Word<NW>& w, int n, uint32_t code) {
    const Word<NW> m = wmask<NW>(2 * n);
    const uint32_t rep = code * P55;
    int c = 0;
#pragma unroll
    for (int k = 0; k < NW; ++k) {
        const uint32_t x = w.w[k] ^ rep;
        c += __popc(~(x | (x >> 1)) & P55 & m.w[k]);
    }
    return c;
}

}  // namespace feat
}  // namespace acx
