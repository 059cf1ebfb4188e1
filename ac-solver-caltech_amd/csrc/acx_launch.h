// acx_launch.h -- the host side of the env-side kernels: the instantiation matching L (dispatch), one
// launcher per kernel family, and the table of which object (-DACX_PART=n) instantiates which.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "acx.h"
#include "acx_expand_kernels.h"
#include "acx_moves.h"
#include "acx_rollout_kernel.h"
#include "acx_step_args.h"
#include "acx_step_kernel.h"
#include "acx_step_pair.h"
#include "acx_tile.h"

namespace acx {

// ---------------------------------------------------------------------------------
// host-side dispatch
// ---------------------------------------------------------------------------------
static inline int nw_for(int L) {
    return L <= 16 ? 1 : L <= 32 ? 2 : L <= 48 ? 3 : L <= 64 ? 4 : 8;
}

template <int NW, int LC, int VEC>
static inline size_t smem_bytes(int L) {
    return (size_t)WPB * TileFor<NW, LC, VEC>::wave_bytes(L);
}

static inline bool aligned16(const void* p) { return ((uintptr_t)p & 15u) == 0; }

// call `f.template go<NW, LC, VEC>()` for the instantiation matching L
template <class F>
static int dispatch(int L, F&& f) {
    const bool v4 = (2 * L) % 4 == 0;
#if defined(ACX_ISA_L128_ONLY)  // faster builds for ISA inspection only
    (void)v4;
    return L == 128 ? f.template go<8, 128, 4>() : ACX_E_ARG;
#elif defined(ACX_ISA_L36_ONLY)  // faster builds for ISA inspection only
    (void)v4;
    return L == 36 ? f.template go<3, 36, 4>() : ACX_E_ARG;
#else
    if (L == 36) return f.template go<3, 36, 4>();
    if (L == 128) return f.template go<8, 128, 4>();
    switch (nw_for(L)) {
        case 1: return v4 ? f.template go<1, 0, 4>() : f.template go<1, 0, 2>();
        case 2: return v4 ? f.template go<2, 0, 4>() : f.template go<2, 0, 2>();
        case 3: return v4 ? f.template go<3, 0, 4>() : f.template go<3, 0, 2>();
        case 4: return v4 ? f.template go<4, 0, 4>() : f.template go<4, 0, 2>();
        default: return v4 ? f.template go<8, 0, 4>() : f.template go<8, 0, 2>();
    }
#endif
}

static inline int finish_launch() {
    return hipGetLastError() == hipSuccess ? ACX_OK : ACX_E_LAUNCH;
}

static inline unsigned grid_for(int64_t rows) {
    return (unsigned)((rows + (int64_t)BLOCK - 1) / BLOCK);
}

// One launcher per kernel family and instantiation.  They are plain (non-static) function
// templates so that the slow-to-compile L = 128 instantiations can be explicitly instantiated in
// separate objects built from the same acx_kernels.hip (-DACX_PART=n, compiled in parallel by build.py)
// while the main object declares them `extern template` below.
template <int NW, int LC, int VEC, bool LEARN>
int launch_step(StepArgs a, hipStream_t s) {
    const size_t shm = smem_bytes<NW, LC, VEC>(a.L);
    if (!LEARN && a.live) {
        step_lengths_kernel<NW, LC, VEC><<<dim3(grid_for(a.B)), dim3(BLOCK), shm, s>>>(a);
        return finish_launch();
    }
    if constexpr (!LEARN && small_step_ok<NW, LC, VEC>()) {
        if (a.B <= SMALL_STEP_MAX_B) {
            constexpr int per_block = WPB * PairLayout<LC>::ENVS;
            step_pair_kernel<NW, LC, VEC><<<dim3((unsigned)((a.B + per_block - 1) / per_block)), dim3(BLOCK),
                                            WPB * PairLayout<LC>::wave_bytes, s>>>(a);
            return finish_launch();
        }
    }
    step_kernel<NW, LC, VEC, LEARN><<<dim3(grid_for(a.B)), dim3(BLOCK), shm, s>>>(a);
    return finish_launch();
}
// How a rollout launch deals its blocks (acx_rollout_deal).  mode ACX_DEAL_*; pct: an odd XCC's
// range as a percentage of an even one's; over_pct: the grid as a percentage of the blocks (the
// surplus is what a fast XCD steals with); ws: the caller's ACX_ROLLOUT_DEAL_WORDS head counters.
// info (acx_rollout_deal_info): filled instead of launching.
struct DealRequest {
    int mode = ACX_DEAL_PLAIN, pct = ACX_DEAL_PCT, over_pct = ACX_DEAL_OVER_PCT;
    uint32_t* ws = nullptr;
    int64_t* info = nullptr;
};
// Launches of at most this many steps (the ones that read int32 ids) keep the plain deal under
// ACX_DEAL_AUTO: at K = 20 the deal's medians were 1.312-1.326 ms against the plain launch's 1.302
// (profiles/r07/r07a_ab_deal_sweep.json, DESIGN.md "Rollout")
constexpr int DEAL_AUTO_MIN_T = 32;

// range limits for `tiles` blocks: the even XCCs weigh 100, the odd ones pct
static inline void deal_bounds(int64_t tiles, int pct, uint32_t* bound) {
    const int64_t total = 4 * (100 + (int64_t)pct);
    for (int x = 0; x <= (int)XCC_RANGES; ++x) {
        const int64_t before = (int64_t)((x + 1) / 2) * 100 + (int64_t)(x / 2) * pct;  // weights of XCCs < x
        bound[x] = (uint32_t)(tiles * before / total);
    }
}

template <int NW, int LC, int VEC, int OBS>
int launch_rollout(RolloutArgs a, hipStream_t s, DealRequest d) {
    const size_t shm = smem_bytes<NW, LC, VEC>(a.L);
    unsigned grid = grid_for(a.B);
    a.deal = XccDeal{};
    if (d.mode != ACX_DEAL_PLAIN || d.info) {
        const int64_t tiles = grid;
        const int64_t dealt_grid = 8 * ((tiles * d.over_pct + 799) / 800);
        bool on = d.mode == ACX_DEAL_XCC;
        int64_t resident = 0;
        if (d.mode == ACX_DEAL_AUTO || d.info) {
            // one resident round: blocks per CU (the occupancy query) x CUs of the current device
            int dev = 0, cus = 0, per_cu = 0;
            if (hipGetDevice(&dev) != hipSuccess ||
                hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess ||
                hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, rollout_kernel<NW, LC, VEC, OBS>, BLOCK, shm) !=
                    hipSuccess)
                return ACX_E_LAUNCH;
            resident = (int64_t)per_cu * cus;
            if (d.mode == ACX_DEAL_AUTO) on = tiles > resident && a.T > DEAL_AUTO_MIN_T;
        }
        if (dealt_grid > INT32_MAX) {
            if (d.mode == ACX_DEAL_XCC) return ACX_E_ARG;
            on = false;
        }
        if (on) {
            deal_bounds(tiles, d.pct, a.deal.bound);
            a.deal.heads = d.ws;
            grid = (unsigned)dealt_grid;
        }
        if (d.info) {
            d.info[0] = on;
            d.info[1] = tiles;
            d.info[2] = grid;
            d.info[3] = resident;
            if (!on) deal_bounds(tiles, d.pct, a.deal.bound);
            for (int x = 0; x < (int)XCC_RANGES; ++x) d.info[4 + x] = a.deal.bound[x + 1] - a.deal.bound[x];
            return ACX_OK;
        }
        if (on) {
            if (!d.ws) return ACX_E_ARG;
            if (hipMemsetAsync(d.ws, 0, ACX_ROLLOUT_DEAL_WORDS * sizeof(uint32_t), s) != hipSuccess) return ACX_E_LAUNCH;
        }
    }
    rollout_kernel<NW, LC, VEC, OBS><<<dim3(grid), dim3(BLOCK), shm, s>>>(a);
    return finish_launch();
}
template <int NW, int LC, int VEC>
int launch_expand(ExpandArgs a, hipStream_t s) {
    if constexpr (LC > 0 && LC % 4 == 0) {
        const size_t rshm = ExpandRowsSmem<NW, LC, VEC>::bytes(a.L);
        if (a.children && rshm <= 64 * 1024) {
            expand12_rows_kernel<NW, LC, VEC><<<dim3((unsigned)((a.N + WAVE - 1) / WAVE)), dim3(BLOCK), rshm, s>>>(a);
            return finish_launch();
        }
    }
    const size_t cshm = ExpandChildrenSmem<NW, LC, VEC>::bytes(a.L);
    if (a.children && cshm <= 64 * 1024) {
        expand12_children_kernel<NW, LC, VEC><<<dim3((unsigned)((a.N + WAVE - 1) / WAVE)), dim3(BLOCK), cshm, s>>>(a);
        return finish_launch();
    }
    const size_t kshm = ExpandKeysSmem<NW, LC, VEC>::bytes(a.L);
    if (!a.children && a.child_key && kshm <= 40 * 1024) {  // the search path
        expand12_keys_kernel<NW, LC, VEC><<<dim3((unsigned)((a.N + WAVE - 1) / WAVE)), dim3(BLOCK), kshm, s>>>(a);
        return finish_launch();
    }
    const size_t shm = (size_t)WPB * ExpandLaunchSmem<NW, LC, VEC>::wave_bytes(a.L);
    expand12_kernel<NW, LC, VEC><<<dim3(grid_for(a.N)), dim3(BLOCK), shm, s>>>(a);
    return finish_launch();
}
template <int NW, int LC, int VEC>
int launch_canon(CanonArgs a, hipStream_t s) {
    const size_t shm = smem_bytes<NW, LC, VEC>(a.L);
    canon_kernel<NW, LC, VEC><<<dim3(grid_for(a.B)), dim3(BLOCK), shm, s>>>(a);
    return finish_launch();
}
template <int NW, int LC, int VEC>
int launch_unpack(UnpackArgs a, hipStream_t s) {
    const size_t shm = smem_bytes<NW, LC, VEC>(a.L);
    unpack_keys_kernel<NW, LC, VEC><<<dim3(grid_for(a.M)), dim3(BLOCK), shm, s>>>(a);
    return finish_launch();
}

// Each kernel instantiation set compiles in an object of its own, built from acx_kernels.hip with
// -DACX_PART=n (build.py compiles them in parallel with the main object, which holds L = 36):
// the runtime-L generic sets (fully unrolled per-letter loops up to 16*NW letters) took ~7 of the
// ~7.5 minutes of one object.  The main object declares them `extern template`.
#define ACX_INST_STEP(EXT, NW, LC, VEC)                                   \
    EXT template int launch_step<NW, LC, VEC, false>(StepArgs, hipStream_t); \
    EXT template int launch_step<NW, LC, VEC, true>(StepArgs, hipStream_t);
#define ACX_INST_ROLL(EXT, NW, LC, VEC, OBS) EXT template int launch_rollout<NW, LC, VEC, OBS>(RolloutArgs, hipStream_t, DealRequest);
#define ACX_INST_SEARCH(EXT, NW, LC, VEC)                                 \
    EXT template int launch_expand<NW, LC, VEC>(ExpandArgs, hipStream_t);  \
    EXT template int launch_canon<NW, LC, VEC>(CanonArgs, hipStream_t);    \
    EXT template int launch_unpack<NW, LC, VEC>(UnpackArgs, hipStream_t);
#define ACX_INST_ALL(EXT, NW, LC, VEC) \
    ACX_INST_STEP(EXT, NW, LC, VEC)    \
    ACX_INST_ROLL(EXT, NW, LC, VEC, 0) \
    ACX_INST_ROLL(EXT, NW, LC, VEC, 1) \
    ACX_INST_ROLL(EXT, NW, LC, VEC, 2) \
    ACX_INST_SEARCH(EXT, NW, LC, VEC)
// part n: 1-3 the L = 128 rollout (int32 obs / int8 obs / none), 4 the L = 128 step, 5 the L = 128
// expand / canonicalize / unpack, 6-10 the generic (runtime-L) sets; build.py's KERNEL_PARTS = 10
#if !defined(ACX_PART)
#if !defined(ACX_ISA_L36_ONLY) && !defined(ACX_ISA_L128_ONLY)
ACX_INST_ROLL(extern, 8, 128, 4, 1)
ACX_INST_ROLL(extern, 8, 128, 4, 2)
ACX_INST_ROLL(extern, 8, 128, 4, 0)
ACX_INST_STEP(extern, 8, 128, 4)
ACX_INST_SEARCH(extern, 8, 128, 4)
ACX_INST_ALL(extern, 8, 0, 4)
ACX_INST_ALL(extern, 8, 0, 2)
ACX_INST_ALL(extern, 4, 0, 4)
ACX_INST_ALL(extern, 4, 0, 2)
ACX_INST_ALL(extern, 3, 0, 4)
ACX_INST_ALL(extern, 3, 0, 2)
ACX_INST_ALL(extern, 2, 0, 4)
ACX_INST_ALL(extern, 2, 0, 2)
ACX_INST_ALL(extern, 1, 0, 4)
ACX_INST_ALL(extern, 1, 0, 2)
#endif
#elif ACX_PART == 1
ACX_INST_ROLL(, 8, 128, 4, 1)
#elif ACX_PART == 2
ACX_INST_ROLL(, 8, 128, 4, 2)
#elif ACX_PART == 3
ACX_INST_ROLL(, 8, 128, 4, 0)
#elif ACX_PART == 4
ACX_INST_STEP(, 8, 128, 4)
#elif ACX_PART == 5
ACX_INST_SEARCH(, 8, 128, 4)
#elif ACX_PART == 6
ACX_INST_ALL(, 8, 0, 4)
#elif ACX_PART == 7
ACX_INST_ALL(, 8, 0, 2)
#elif ACX_PART == 8
ACX_INST_ALL(, 4, 0, 4)
ACX_INST_ALL(, 4, 0, 2)
#elif ACX_PART == 9
ACX_INST_ALL(, 3, 0, 4)
ACX_INST_ALL(, 3, 0, 2)
#elif ACX_PART == 10
ACX_INST_ALL(, 2, 0, 4)
ACX_INST_ALL(, 2, 0, 2)
ACX_INST_ALL(, 1, 0, 4)
ACX_INST_ALL(, 1, 0, 2)
#endif

struct StepLaunch {
    StepArgs a;
    hipStream_t s;
    bool learn;
    template <int NW, int LC, int VEC>
    int go() {
        a.in_place = a.state_in == a.state_out;
        return learn ? launch_step<NW, LC, VEC, true>(a, s) : launch_step<NW, LC, VEC, false>(a, s);
    }
};
struct RolloutLaunch {
    RolloutArgs a;
    hipStream_t s;
    DealRequest d;
    template <int NW, int LC, int VEC>
    int go() {
        if (a.obs_traj8) return launch_rollout<NW, LC, VEC, 2>(a, s, d);
        if (a.obs_traj) return launch_rollout<NW, LC, VEC, 1>(a, s, d);
        return launch_rollout<NW, LC, VEC, 0>(a, s, d);
    }
};
struct ExpandLaunch {
    ExpandArgs a;
    hipStream_t s;
    template <int NW, int LC, int VEC>
    int go() { return launch_expand<NW, LC, VEC>(a, s); }
};
struct CanonLaunch {
    CanonArgs a;
    hipStream_t s;
    template <int NW, int LC, int VEC>
    int go() { return launch_canon<NW, LC, VEC>(a, s); }
};
struct UnpackLaunch {
    UnpackArgs a;
    hipStream_t s;
    template <int NW, int LC, int VEC>
    int go() { return launch_unpack<NW, LC, VEC>(a, s); }
};

}  // namespace acx
