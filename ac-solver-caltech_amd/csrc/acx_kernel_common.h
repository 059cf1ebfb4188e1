// acx_kernel_common.h -- what the env-side kernels share besides the tile: the per-wave prologue
// (which tile of 64 rows a wave owns), a lane's registers written straight to a global row, and
// the resets' whole-tile threshold.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "acx_moves.h"
#include "acx_planes.h"

namespace acx {

// Per-lane registers -> row in HBM directly (uncoalesced; only for final_obs on the rare
// same-step-autoreset path of the step kernel).
template <int NW>
__device__ __forceinline__ void regs_to_global(int32_t* dst, const PresRegs<NW>& p, int L) {
    for (int h = 0; h < 2; ++h) {
        const Word<NW> w = h ? p.w1 : p.w0;
        const int n = h ? p.n1 : p.n0;
#pragma unroll 1
        for (int k = 0; k < L; ++k) {
            const uint32_t code = wletter<NW>(w, k);
            const int32_t v = (int32_t)(int8_t)((0xFE02FF01u >> (code << 3)) & 0xffu);
            dst[h * L + k] = k < n ? v : 0;
        }
    }
}

template <int PW>
__device__ __forceinline__ void regs_to_global(int32_t* dst, const PlaneRegs<PW>& p, int L) {
    for (int h = 0; h < 2; ++h) {
        const Planes<PW> w = h ? p.w1 : p.w0;
        const int n = h ? p.n1 : p.n0;
#pragma unroll 1
        for (int k = 0; k < L; ++k) {
            const uint32_t code = pl::pletter<PW>(w, k);
            const int32_t v = (int32_t)(int8_t)((0xFE02FF01u >> (code << 3)) & 0xffu);
            dst[h * L + k] = k < n ? v : 0;
        }
    }
}

// A wave reloads its whole tile of starting states (one coalesced pass) when more than this
// many of its lanes reset on the same step (a synchronised truncation); for fewer resetting
// lanes the wave loads just their rows (tile.load_rows), so scattered resets cost their rows.
constexpr int RESET_TILE_MIN = 24;

// common per-wave prologue: tile index, rows in the tile, LDS slice
struct WaveCtx {
    int lane, wid;
    int64_t r0;
    int R;
    bool active;
};
__device__ __forceinline__ bool wave_ctx(int64_t rows, WaveCtx& w) {
    w.lane = threadIdx.x & (WAVE - 1);
    // wave-uniform (SGPR): the tile base, its row count and the addresses derived from them
    w.wid = __builtin_amdgcn_readfirstlane((int)(threadIdx.x / WAVE));
    w.r0 = ((int64_t)blockIdx.x * WPB + w.wid) * WAVE;
    if (w.r0 >= rows) return false;
    w.R = (int)((rows - w.r0) < WAVE ? (rows - w.r0) : WAVE);
    w.active = w.lane < w.R;
    return true;
}

}  // namespace acx
