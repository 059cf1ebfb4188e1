// acx_mlp.h -- the FeatureMLP scorer (value_search/value_network.py, FeatureMLP: 14 features,
// hidden layers with ReLU, one output) as one exact float32 arithmetic, shared by the device units
// (acx_mlp.hip: acx_mlp_scores; acx_vgreedy.hip: the fused pop) and the host one (acx_mlp_host.cpp).
//
// A network is n layers, 2 <= n <= 5, of widths dims[0 .. n]: dims[0] = 14, every hidden width a
// multiple of 64 up to 256, dims[n] = 1.  Its parameters are one float32 buffer: per layer W
// transposed (k-major, K x H), then the bias (H): the weights of all outputs for one k are contiguous.
//
// The contract, for every output j of every layer:
//   acc = bias[j];  for k = 0 .. K-1 ascending: acc = fmaf(W[k][j], x[k], acc)
// with the explicit fused multiply-add, no reassociation inside a chain, and after a hidden layer
// v < 0 ? 0 : v (a NaN and -0.0 pass).  The score is the last layer's output y itself: the
// reference takes expm1(y), which is increasing, so y orders as the reference's exact scores do; in
// float32 expm1 merges neighbours into ties and is +inf above about 88.7, y does neither.
//
// Device: one wave evaluates G = 4 rows at a time.  Lane j owns the NO = H / 64 consecutive outputs
// NO j .. NO j + NO - 1 of a hidden layer, G accumulators each: its weights for one k are one load of
// up to 16 bytes, the wave's a contiguous 4 H bytes; the rows' activations sit in LDS as act[k][G]
// (one 16-byte broadcast read per k), written in place once a layer's chains are complete.  The last
// layer's chain of row c is lane c's.  Parallelism is across outputs and rows only.  params must be
// 16-byte aligned.
#pragma once
#include <stdint.h>

namespace acx {
namespace mlp {

constexpr int IN = 14;        // input width
constexpr int MAX_HIDDEN = 4;  // hidden layers
constexpr int MAX_W = 256;     // widest hidden layer
constexpr int STEP = 64;       // a hidden width is a multiple of this
constexpr int G = 4;           // rows a wave evaluates together

struct Net {
    const float* params;
    int n;            // layers
    uint32_t hidden;  // width / STEP of hidden layer l = 1 .. n - 1 in bits 4 (l - 1) .. 4 l - 1: no indexed array
};

// dims[0 .. n_layers] within the limits above
inline bool aligned(const float* params) { return params && ((uintptr_t)params & 15u) == 0; }

inline bool valid(const int32_t* dims, int32_t n_layers) {
    if (!dims || n_layers < 2 || n_layers > MAX_HIDDEN + 1) return false;
    if (dims[0] != IN || dims[n_layers] != 1) return false;
    for (int l = 1; l < n_layers; ++l)
        if (dims[l] < STEP || dims[l] > MAX_W || dims[l] % STEP) return false;
    return true;
}

inline Net net_of(const float* params, const int32_t* dims, int32_t n_layers) {
    Net net{params, n_layers, 0};
    for (int l = 1; l < n_layers; ++l) net.hidden |= (uint32_t)(dims[l] / STEP) << (4 * (l - 1));
    return net;
}

#ifdef __HIPCC__
// lane's NO consecutive weights of one k as one load (16-byte aligned: a layer starts a multiple of
// 256 bytes into params)
template <int NO>
__device__ __forceinline__ void load_w(const float* __restrict__ p, float (&w)[NO]) {
    if constexpr (NO == 4) {
        const float4 v = *reinterpret_cast<const float4*>(p);
        w[0] = v.x, w[1] = v.y, w[2] = v.z, w[3] = v.w;
    } else if constexpr (NO == 2) {
        const float2 v = *reinterpret_cast<const float2*>(p);
        w[0] = v.x, w[1] = v.y;
    } else {
#pragma unroll
        for (int o = 0; o < NO; ++o) w[o] = p[o];
    }
}

// a hidden layer of H = 64 NO outputs over act[0 .. K): in place
template <int NO>
__device__ __forceinline__ void hidden(const float* __restrict__ W, int K, float (*act)[G], int lane) {
    constexpr int H = STEP * NO;
    const float* bias = W + K * H;
    float acc[NO][G];
    {
        float b[NO];
        load_w<NO>(bias + NO * lane, b);
#pragma unroll
        for (int o = 0; o < NO; ++o)
#pragma unroll
            for (int c = 0; c < G; ++c) acc[o][c] = b[o];
    }
#pragma unroll 8
    for (int k = 0; k < K; ++k) {
        float x[G], w[NO];
        load_w<NO>(W + k * H + NO * lane, w);
#pragma unroll
        for (int c = 0; c < G; ++c) x[c] = act[k][c];
#pragma unroll
        for (int o = 0; o < NO; ++o)
#pragma unroll
            for (int c = 0; c < G; ++c) acc[o][c] = __fmaf_rn(w[o], x[c], acc[o][c]);
    }
    __syncthreads();  // every chain has read its inputs
#pragma unroll
    for (int o = 0; o < NO; ++o)
#pragma unroll
        for (int c = 0; c < G; ++c) {
            const float v = acc[o][c];
            act[NO * lane + o][c] = v < 0.0f ? 0.0f : v;
        }
    __syncthreads();
}

// the network over the G rows in act[0 .. IN) (act: MAX_W rows of LDS), by one wave: lane c < G
// returns row c's y.  The caller's next barrier frees act.
__device__ __forceinline__ float forward(const Net& net, float (*act)[G], int lane) {
    const float* W = net.params;
    int K = IN;
#pragma unroll 1
    for (int l = 1; l < net.n; ++l) {
        const int H = STEP * (int)((net.hidden >> (4 * (l - 1))) & 15u);
        switch (H / STEP) {  // (uniform)
            case 1: hidden<1>(W, K, act, lane); break;
            case 2: hidden<2>(W, K, act, lane); break;
            case 3: hidden<3>(W, K, act, lane); break;
            default: hidden<4>(W, K, act, lane); break;
        }
        W += (K + 1) * H;
        K = H;
    }
    float y = 0.0f;
    if (lane < G) {
        y = W[K];
        for (int k = 0; k < K; ++k) y = __fmaf_rn(W[k], act[k][lane], y);
    }
    return y;
}
#endif  // __HIPCC__

}  // namespace mlp
}  // namespace acx
