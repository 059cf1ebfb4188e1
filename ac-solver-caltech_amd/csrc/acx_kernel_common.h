// acx_kernel_common.h -- what the env-side kernels share besides the tile: the per-wave prologue
// (which tile of 64 rows a wave owns), the rollout's deal of blocks by XCC, a lane's registers
// written straight to a global row, and the resets' whole-tile threshold.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "acx_moves.h"
#include "acx_planes.h"
#include "acx_step_args.h"

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
// `blk`: the block of BLOCK rows this workgroup runs (wave-uniform)
__device__ __forceinline__ bool wave_ctx_at(int64_t rows, int64_t blk, WaveCtx& w) {
    w.lane = threadIdx.x & (WAVE - 1);
    // wave-uniform (SGPR): the tile base, its row count and the addresses derived from them
    w.wid = __builtin_amdgcn_readfirstlane((int)(threadIdx.x / WAVE));
    w.r0 = (blk * WPB + w.wid) * WAVE;
    if (w.r0 >= rows) return false;
    w.R = (int)((rows - w.r0) < WAVE ? (rows - w.r0) : WAVE);
    w.active = w.lane < w.R;
    return true;
}
__device__ __forceinline__ bool wave_ctx(int64_t rows, WaveCtx& w) { return wave_ctx_at(rows, (int64_t)blockIdx.x, w); }

// The XCC deal (acx_step_args.h XccDeal, DESIGN.md "Rollout"): which block of rows a workgroup runs,
// decided by the XCC it landed on instead of by blockIdx.  The blocks of the batch are 8 contiguous
// ranges [bound[x], bound[x + 1]), one per XCC; a workgroup takes the next block of its own XCC's
// range from that range's head counter, and when the range is exhausted it takes from the other
// seven in turn, starting at x + 1 so that thieves spread out.  -1: every range is exhausted.
// Nothing waits on another workgroup, and nothing depends on which ids the hardware reports: a
// counter hands out each of its range's blocks once, a workgroup takes at most one block and leaves
// without one only after it has seen all eight ranges exhausted, so a grid of at least as many
// workgroups as blocks runs every block exactly once.
__device__ __forceinline__ uint32_t xcc_id() {
    // HW_REG_XCC_ID (id 20), bits [3:0]
    return __builtin_amdgcn_s_getreg(20 | (0 << 6) | (3 << 11)) & 0xf;
}
// called by every thread of the workgroup, before `smem`'s first other use; wave-uniform result
__device__ __forceinline__ int64_t xcc_deal_block(const XccDeal& d, char* smem) {
    int* slot = reinterpret_cast<int*>(smem);
    if (threadIdx.x == 0) {
        const uint32_t x = xcc_id();
        int blk = -1;
        for (uint32_t i = 0; i < XCC_RANGES; ++i) {
            const uint32_t y = (x + i) % XCC_RANGES;
            const uint32_t quota = d.bound[y + 1] - d.bound[y];
            if (quota == 0) continue;
            const uint32_t k = atomicAdd(d.heads + y * XCC_HEAD_STRIDE, 1u);
            if (k < quota) {
                blk = (int)(d.bound[y] + k);
                break;
            }
        }
        *slot = blk;
    }
    __syncthreads();
    const int blk = __builtin_amdgcn_readfirstlane(*slot);
    __syncthreads();  // read by every wave before wave 0's tile overwrites it
    return (int64_t)blk;
}

}  // namespace acx
