// acx_mlp.hip -- acx_mlp_scores: the FeatureMLP scorer of acx_mlp.h over rows of features already on
// the device, one wave per 4 rows.  The arithmetic is the contract of acx_mlp.h, the same as the
// host's acx_mlp_scores_host (acx_mlp_host.cpp) bit for bit (tests/test_gpu_mlp_scores.py).
//
// mlp_scores_kernel: a workgroup is one wave; it loads 4 rows' features into LDS as act[k][4],
// runs the layers (acx_mlp.h, forward) and lanes 0 .. 3 write the rows' y.  The grid is one wave per
// 4 rows up to 2^16 waves, which then stride.  Every wave reads all the weights (L2).
//
// Registers and LDS (tools/kernel_resources.py; profiles/fused_mlp/kernel_resources.md):
//   mlp_scores_kernel   110 VGPRs, 4,096 B of LDS, no scratch.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "acx.h"

#include "acx_mlp.h"

namespace acx {
namespace mlp {

constexpr int64_t MAX_WAVES = 1 << 16;

__global__ __launch_bounds__(64) void mlp_scores_kernel(const float* x, Net net, float* out, int64_t M) {
    __shared__ __attribute__((aligned(16))) float act[MAX_W][G];
    const int lane = threadIdx.x;
    for (int64_t r0 = (int64_t)blockIdx.x * G; r0 < M; r0 += (int64_t)gridDim.x * G) {
        __syncthreads();  // the last rows' chains have read act
        if (lane < IN * G) {  // lane = k * G + c: row c's feature k (a row past M: 0)
            const int k = lane / G, c = lane % G;
            act[k][c] = r0 + c < M ? x[(r0 + c) * IN + k] : 0.0f;
        }
        __syncthreads();
        const float y = forward(net, act, lane);
        if (lane < G && r0 + lane < M) out[r0 + lane] = y;
    }
}

}  // namespace mlp
}  // namespace acx

using namespace acx::mlp;

extern "C" int acx_mlp_scores(const float* x, const float* params, const int32_t* dims, int32_t n_layers, float* out,
                              int64_t M, void* stream) {
    if (M < 0 || !aligned(params) || !valid(dims, n_layers)) return ACX_E_ARG;
    if (M == 0) return ACX_OK;  // (an empty tensor's data pointer may be NULL)
    if (!x || !out) return ACX_E_ARG;
    const int64_t waves = (M + G - 1) / G;
    mlp_scores_kernel<<<dim3((unsigned)(waves < MAX_WAVES ? waves : MAX_WAVES)), dim3(64), 0, (hipStream_t)stream>>>(
        x, net_of(params, dims, n_layers), out, M);
    return hipGetLastError() == hipSuccess ? ACX_OK : ACX_E_LAUNCH;
}
