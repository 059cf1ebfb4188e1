// acx_mlp_host.cpp -- acx_mlp_scores_host: the FeatureMLP scorer of acx_mlp.h on host memory, in the
// contract's arithmetic: per output acc = bias, then acc = fmaf(W[k][j], x[k], acc) for ascending k
// (std::fmaf: one rounding), v < 0 ? 0 : v after a hidden layer, y the last layer's output.  The
// loops run k outside and j inside -- the parameters are k-major -- which leaves every output's chain
// in ascending k.  No GPU is needed.
#include <cmath>
#include <cstdint>

#include "acx.h"

#include "acx_mlp.h"

using namespace acx::mlp;

extern "C" int acx_mlp_scores_host(const float* x, const float* params, const int32_t* dims, int32_t n_layers,
                                   float* out, int64_t M) {
    if (M < 0 || !params || !valid(dims, n_layers)) return ACX_E_ARG;
    if (M == 0) return ACX_OK;
    if (!x || !out) return ACX_E_ARG;
    float a[MAX_W], b[MAX_W];
    for (int64_t r = 0; r < M; ++r) {
        float *cur = a, *nxt = b;
        for (int k = 0; k < IN; ++k) cur[k] = x[r * IN + k];
        const float* W = params;
        for (int l = 0; l < n_layers; ++l) {
            const int K = dims[l], H = dims[l + 1];
            const float* bias = W + (int64_t)K * H;
            for (int j = 0; j < H; ++j) nxt[j] = bias[j];
            for (int k = 0; k < K; ++k) {
                const float xk = cur[k];
                for (int j = 0; j < H; ++j) nxt[j] = std::fmaf(W[k * H + j], xk, nxt[j]);
            }
            if (l + 1 < n_layers)
                for (int j = 0; j < H; ++j) nxt[j] = nxt[j] < 0.0f ? 0.0f : nxt[j];
            W = bias + H;
            float* t = cur;
            cur = nxt;
            nxt = t;
        }
        out[r] = cur[0];
    }
    return ACX_OK;
}
