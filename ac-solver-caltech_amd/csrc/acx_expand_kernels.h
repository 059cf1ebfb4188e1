// acx_expand_kernels.h -- the search-side kernels: the 12 children of every parent (four expand12
// kernels, launch_expand in acx_launch.h picks one), canonicalize and unpack_keys.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "acx.h"
#include "acx_kernel_common.h"
#include "acx_moves.h"
#include "acx_step_args.h"
#include "acx_tile.h"

namespace acx {

// ---------------------------------------------------------------------------------
// What the four expand12 kernels share.  Only three small helpers are here: the compiled kernels are
// held to the instructions of their hand-inlined versions, and a helper for any of the other shared
// steps -- the move on a child (bad -> ACX_ERR_DOMAIN, clean -> ac_move_clean, else ac_move), the
// 0xFF length sentinel of an errored child's key, staging a packed parent and reading it back, a
// prologue with the early return inside -- changed register allocation and schedule in some
// instantiation.  Those steps stay inline in each kernel, marked "(inline: ...)"; a change to one
// of them is made at every such mark.
// ---------------------------------------------------------------------------------

// 64-bit words of a packed key (acx_key_words): 2 x 2L code bits, then the two length bytes
__host__ __device__ constexpr int key_words(int L) { return (4 * L + 16 + 63) / 64; }

// The prologue of a block that owns one tile of 64 parents (wave_ctx's counterpart for the three
// block-per-tile kernels, whose waves share the tile and split the 12 actions).  The kernel returns
// on r0 >= N (block-uniform) itself, then takes its row count from tile_rows.
struct BlockCtx {
    int lane, wid;
    int64_t r0;
};
__device__ __forceinline__ BlockCtx block_ctx() {
    BlockCtx b;
    b.lane = threadIdx.x & (WAVE - 1);
    b.wid = __builtin_amdgcn_readfirstlane((int)(threadIdx.x / WAVE));
    b.r0 = (int64_t)blockIdx.x * WAVE;
    return b;
}
__device__ __forceinline__ int tile_rows(int64_t rows, int64_t r0) {
    return (int)((rows - r0) < WAVE ? (rows - r0) : WAVE);
}

// A packed parent staged in LDS by wave 0 for the block's other waves (expand12_keys_kernel,
// expand12_rows_kernel): packed_words<NW>() dwords -- both relators' codes, the two lengths (a
// byte each), then bad | clean << 1
template <int NW>
__host__ __device__ constexpr int packed_words() { return 2 * NW + 2; }

// n staged words or bytes -> their contiguous run in HBM, by all threads of the block
template <class T>
__device__ __forceinline__ void copy_run(T* dst, const T* src, int n) {
    for (int i = threadIdx.x; i < n; i += BLOCK) dst[i] = src[i];
}

constexpr int KEY_GROUP = 3;  // actions per staged key group in expand12 (12 % KEY_GROUP == 0)

// expand12's per-wave LDS: the tile, or the staged keys of one group, whichever is larger
template <int NW, int LC, int VEC>
struct ExpandLaunchSmem {
    static __host__ __device__ size_t wave_bytes(int L) {
        const size_t t = TileFor<NW, LC, VEC>::wave_bytes(L);
        const size_t k = (size_t)WAVE * KEY_GROUP * (size_t)key_words(L) * 8;
        return ((t > k ? t : k) + 15) & ~(size_t)15;
    }
};

template <int NW, int LC, int VEC>
__global__ __launch_bounds__(BLOCK, Occupancy<LC>::waves_per_simd) void expand12_kernel(ExpandArgs a) {
    using Tile = TileFor<NW, LC, VEC>;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    WaveCtx w;
    if (!wave_ctx(a.N, w)) return;
    Tile tile(smem + w.wid * ExpandLaunchSmem<NW, LC, VEC>::wave_bytes(a.L), a.L);
    const int L = tile.Lr(), twoL = 2 * L;
    const int64_t par = w.r0 + w.lane;

    tile.load(a.parents + w.r0 * twoL, w.R, w.lane);
    PresRegs<NW> p;
    bool bad = false, clean = false;
    const bool cyc = a.cyclical != 0;
    if (w.active) {
        bad = tile.pack(w.lane, p);
        clean = !bad && is_clean<NW>(p.w0, p.n0, p.w1, p.n1, cyc);
    }
    tile.flag_rows(w.lane, bad ? FB_IN : 0u);  // children of out-of-domain parents copy the parent row
    int nerr = 0;
    // keys only (the search path): stage each group of KEY_GROUP actions' keys in LDS
    // (the parents' rows are no longer needed once packed) and write them out as
    // contiguous KEY_GROUP*kw64*8-byte segments instead of per-lane 8-byte pieces
    const bool stage_keys = a.child_key != nullptr && a.children == nullptr;
    uint64_t* kst = reinterpret_cast<uint64_t*>(smem + w.wid * ExpandLaunchSmem<NW, LC, VEC>::wave_bytes(a.L));
    for (int act = 0; act < 12; ++act) {
        if (w.active) {
            PresRegs<NW> q = p;  // (inline: the move on a child)
            int e;
            if (bad) e = ACX_ERR_DOMAIN;
            else if (clean) e = ac_move_clean<NW>(q.w0, q.n0, q.w1, q.n1, act, L, cyc);
            else e = ac_move<NW>(q.w0, q.n0, q.w1, q.n1, act, L, cyc);
            const int64_t ci = par * 12 + act;
            nerr += e != ACX_ERR_NONE;
            if (a.err) a.err[ci] = (uint8_t)e;
            if (a.child_len) {
                a.child_len[2 * ci] = q.n0;
                a.child_len[2 * ci + 1] = q.n1;
            }
            if (a.child_key) {
                // (inline: the sentinel) an errored child's key has both length bytes 0xFF (acx.h)
                PresRegs<NW> kq = q;
                if (e != ACX_ERR_NONE) {
                    kq.n0 = 0xff;
                    kq.n1 = 0xff;
                }
                if (stage_keys) store_key<NW>(kst + (w.lane * KEY_GROUP + act % KEY_GROUP) * a.kw64, a.kw64, L, kq);
                else store_key<NW>(a.child_key + ci * a.kw64, a.kw64, L, kq);
            }
            if (a.children && !bad) tile.unpack(w.lane, q);
        }
        if (a.children) {
            wave_sync();
            tile.template store<true, NT_STATE>(a.children + (w.r0 * 12 + act) * twoL, (int64_t)12 * twoL, w.R,
                                      a.parents + w.r0 * twoL, twoL, w.lane);
            wave_sync();
        }
        if (stage_keys && act % KEY_GROUP == KEY_GROUP - 1) {
            wave_sync();
            const int kw = LC > 0 ? key_words(LC) : a.kw64;
            const int seg = KEY_GROUP * kw;  // u64 words per parent in this group
            const int n = w.R * seg;
            uint64_t* gbase = a.child_key + (w.r0 * 12 + (act - (KEY_GROUP - 1))) * kw;
            for (int i = w.lane; i < n; i += WAVE) {
                const int pp = i / seg;
                gbase[(int64_t)pp * 12 * kw + (i - pp * seg)] = kst[i];
            }
            wave_sync();
        }
    }
    if (nerr && a.err_count) atomicAdd(a.err_count, nerr);
}

// expand12 without int32 children (the search path: packed child keys, optional lengths/err):
// one block of 4 waves per tile of 64 parents; wave 0 stages and packs the tile, every wave then
// makes the children of 3 actions (wave w: 3w..3w+2) -- 4x the lanes of a lane-per-parent loop
// over 12 moves, whose dependent VALU chain left most issue slots empty -- and the block's
// 12 * 64 keys are staged in LDS (parent-major, as in HBM) and written as one contiguous run.
constexpr int KEYS_APW = 12 / WPB;  // actions per wave (3)

template <int NW, int LC, int VEC>
struct ExpandKeysSmem {
    static __host__ __device__ size_t region_a(int L) {
        const size_t t = TileFor<NW, LC, VEC>::wave_bytes(L);
        const size_t k = (size_t)WAVE * 12 * (size_t)key_words(L) * 8;
        return ((t > k ? t : k) + 15) & ~(size_t)15;
    }
    static __host__ __device__ size_t bytes(int L) { return region_a(L) + (size_t)WAVE * packed_words<NW>() * 4; }
};

template <int NW, int LC, int VEC>
__global__ __launch_bounds__(BLOCK) void expand12_keys_kernel(ExpandArgs a) {
    using Tile = TileFor<NW, LC, VEC>;
    using Smem = ExpandKeysSmem<NW, LC, VEC>;
    constexpr int PW = packed_words<NW>();
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const BlockCtx b = block_ctx();
    if (b.r0 >= a.N) return;  // block-uniform
    const int lane = b.lane, wid = b.wid, R = tile_rows(a.N, b.r0);
    const int64_t r0 = b.r0;
    const int L = LC > 0 ? LC : a.L;
    const int kw = LC > 0 ? key_words(LC) : a.kw64;
    char* region = smem;
    uint32_t* packed = reinterpret_cast<uint32_t*>(smem + Smem::region_a(a.L));
    const bool cyc = a.cyclical != 0;
    Tile tile(region, a.L);
    if constexpr (LC > 0 && LC % 4 == 0) tile.load_block(a.parents + r0 * 2 * L, R);
    else if (wid == 0) tile.load(a.parents + r0 * 2 * L, R, lane);
    if (wid == 0) {
        if (lane < R) {
            PresRegs<NW> p;
            const bool bad = tile.pack(lane, p);
            const bool clean = !bad && is_clean<NW>(p.w0, p.n0, p.w1, p.n1, cyc);
            uint32_t* d = packed + lane * PW;  // (inline: staging a packed parent)
#pragma unroll
            for (int k = 0; k < NW; ++k) {
                d[k] = p.w0.w[k];
                d[NW + k] = p.w1.w[k];
            }
            d[2 * NW] = (uint32_t)p.n0 | ((uint32_t)p.n1 << 8);
            d[2 * NW + 1] = (uint32_t)bad | ((uint32_t)clean << 1);
        }
    }
    __syncthreads();
    uint64_t* kst = reinterpret_cast<uint64_t*>(region);
    int nerr = 0;
    if (lane < R) {
        PresRegs<NW> p;
        const uint32_t* d = packed + lane * PW;  // (inline: reading a staged parent back)
#pragma unroll
        for (int k = 0; k < NW; ++k) {
            p.w0.w[k] = d[k];
            p.w1.w[k] = d[NW + k];
        }
        p.n0 = (int)(d[2 * NW] & 0xffu);
        p.n1 = (int)((d[2 * NW] >> 8) & 0xffu);
        const bool bad = (d[2 * NW + 1] & 1u) != 0, clean = (d[2 * NW + 1] & 2u) != 0;
        const int64_t par = r0 + lane;
#pragma unroll 1
        for (int j = 0; j < KEYS_APW; ++j) {
            const int act = wid * KEYS_APW + j;
            PresRegs<NW> q = p;  // (inline: the move on a child)
            int e;
            if (bad) e = ACX_ERR_DOMAIN;
            else if (clean) e = ac_move_clean<NW>(q.w0, q.n0, q.w1, q.n1, act, L, cyc);
            else e = ac_move<NW>(q.w0, q.n0, q.w1, q.n1, act, L, cyc);
            const int64_t ci = par * 12 + act;
            nerr += e != ACX_ERR_NONE;
            if (a.err) a.err[ci] = (uint8_t)e;
            if (a.child_len) {
                a.child_len[2 * ci] = q.n0;
                a.child_len[2 * ci + 1] = q.n1;
            }
            if (e != ACX_ERR_NONE) {  // (inline: the sentinel) both length bytes 0xFF (acx.h)
                q.n0 = 0xff;
                q.n1 = 0xff;
            }
            uint64_t key[NW + 1];
            make_key<NW>(L, q, key);
#pragma unroll
            for (int k = 0; k < NW + 1; ++k)
                if (k < kw) kst[(lane * 12 + act) * kw + k] = key[k];
        }
    }
    __syncthreads();
    uint64_t* dst = a.child_key + r0 * 12 * kw;
    if constexpr (NT_KEYS) {
        // 16-B non-temporal stores (dst is 16-B aligned: r0 is a multiple of 64), odd tail word apart
        const int nw = R * 12 * kw;
        for (int i = threadIdx.x; 2 * i + 1 < nw; i += BLOCK) {
            typedef unsigned long long v2u_t __attribute__((ext_vector_type(2)));
            const v2u_t x = {kst[2 * i], kst[2 * i + 1]};
            __builtin_nontemporal_store(x, reinterpret_cast<v2u_t*>(dst) + i);
        }
        if ((nw & 1) && threadIdx.x == 0) dst[nw - 1] = kst[nw - 1];
    } else {
        for (int i = threadIdx.x; i < R * 12 * kw; i += BLOCK) dst[i] = kst[i];
    }
    if (nerr && a.err_count) atomicAdd(a.err_count, nerr);
}

// expand12 with int32 children (acx_expand12 children != NULL): one block of 4 waves per tile
// of 64 parents, as expand12_keys_kernel -- every wave stages and packs the parents, wave w
// makes the children of actions 3w..3w+2, one action at a time: unpack into its own LDS tile,
// then a tile store with row pitch 12 * 2L (child (p, a) is row 12p + a).  The block's 64 x 12
// child rows are one contiguous 221 KB region at L = 36, written as 3-row runs per parent and
// wave (the lane-per-parent loop it replaces made 12 serial moves per lane and wrote each child
// row as its own 288-byte run).  Lengths and error codes go through LDS and out as one
// contiguous run per block.  Out-of-domain parents' children are copies of the parent row (the
// fallback rows of the tile store), as in expand12_kernel.
template <int NW, int LC, int VEC>
struct ExpandChildrenSmem {
    static __host__ __device__ size_t tile_bytes(int L) {
        return (TileFor<NW, LC, VEC>::wave_bytes(L) + 15) & ~(size_t)15;
    }
    static __host__ __device__ size_t lens_off(int L) { return WPB * tile_bytes(L); }
    static __host__ __device__ size_t err_off(int L) { return lens_off(L) + (size_t)WAVE * 12 * 2 * 4; }
    static __host__ __device__ size_t bytes(int L) { return err_off(L) + (size_t)WAVE * 12; }
};

template <int NW, int LC, int VEC>
__global__ __launch_bounds__(BLOCK) void expand12_children_kernel(ExpandArgs a) {
    using Tile = TileFor<NW, LC, VEC>;
    using Smem = ExpandChildrenSmem<NW, LC, VEC>;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const BlockCtx b = block_ctx();
    if (b.r0 >= a.N) return;  // block-uniform
    const int lane = b.lane, wid = b.wid, R = tile_rows(a.N, b.r0);
    const int64_t r0 = b.r0;
    const bool active = lane < R;
    Tile tile(smem + wid * Smem::tile_bytes(a.L), a.L);
    const int L = tile.Lr(), twoL = 2 * L;
    int32_t* lens_st = reinterpret_cast<int32_t*>(smem + Smem::lens_off(a.L));
    uint8_t* err_st = reinterpret_cast<uint8_t*>(smem + Smem::err_off(a.L));
    const bool cyc = a.cyclical != 0;
    // every wave stages and packs the parent tile itself (the block's other three reads of the
    // 18 KB tile are L2 hits): no block-wide wait on one wave's load before the moves start;
    // the tile's flags mark the out-of-domain rows, whose children copy the parent row
    tile.load(a.parents + r0 * twoL, R, lane);
    PresRegs<NW> p;
    bool bad = false, clean = false;
    if (active) {
        bad = tile.pack(lane, p);
        clean = !bad && is_clean<NW>(p.w0, p.n0, p.w1, p.n1, cyc);
    }
    tile.flag_rows(lane, bad ? FB_IN : 0u);  // incl. a zero inside a relator (not flagged by the load)

    int nerr = 0;
    const int64_t par = r0 + lane;
#pragma unroll 1
    for (int j = 0; j < KEYS_APW; ++j) {
        const int act = wid * KEYS_APW + j;
        if (active) {
            PresRegs<NW> q = p;  // (inline: the move on a child)
            int e;
            if (bad) e = ACX_ERR_DOMAIN;
            else if (clean) e = ac_move_clean<NW>(q.w0, q.n0, q.w1, q.n1, act, L, cyc);
            else e = ac_move<NW>(q.w0, q.n0, q.w1, q.n1, act, L, cyc);
            nerr += e != ACX_ERR_NONE;
            err_st[lane * 12 + act] = (uint8_t)e;
            lens_st[(lane * 12 + act) * 2] = q.n0;
            lens_st[(lane * 12 + act) * 2 + 1] = q.n1;
            if (a.child_key) {  // keys as well (not the search path): per lane, unstaged
                PresRegs<NW> kq = q;
                if (e != ACX_ERR_NONE) {  // (inline: the sentinel)
                    kq.n0 = 0xff;
                    kq.n1 = 0xff;
                }
                store_key<NW>(a.child_key + (par * 12 + act) * a.kw64, a.kw64, L, kq);
            }
            if (!bad) tile.unpack(lane, q);
        }
        wave_sync();
        tile.template store<true, NT_STATE>(a.children + (r0 * 12 + act) * twoL, (int64_t)12 * twoL, R,
                                  a.parents + r0 * twoL, twoL, lane);
        wave_sync();
    }
    __syncthreads();
    if (a.child_len) copy_run(a.child_len + r0 * 24, lens_st, R * 24);
    if (a.err) copy_run(a.err + r0 * 12, err_st, R * 12);
    if (nerr && a.err_count) atomicAdd(a.err_count, nerr);
}

// expand12 with int32 children for compile-time L % 4 == 0 (L = 36 and 128): the block makes its
// 64 x 12 children exactly as expand12_keys_kernel (wave 0 packs the parents, wave w the actions
// 3w..3w+2), stages each child in LDS as packed words (both relators' 2-bit codes and the two
// lengths: 2 NW + 1 dwords), then all 256 threads expand the staged children into the block's
// contiguous 64 x 12 x 2L int32 region with 16-byte stores, consecutive threads on consecutive
// chunks -- the whole 221 KB (L = 36) as one linear stream per block.  Out-of-domain parents'
// children are copies of the parent row; lengths come from the staged words, error codes from LDS.
template <int NW, int LC, int VEC>
struct ExpandRowsSmem {
    static constexpr int SW = 2 * NW + 1;  // staged dwords per child
    static __host__ __device__ size_t region_a(int L) {
        const size_t t = TileFor<NW, LC, VEC>::wave_bytes(L);
        const size_t k = (size_t)WAVE * 12 * SW * 4;
        return ((t > k ? t : k) + 15) & ~(size_t)15;
    }
    static __host__ __device__ size_t err_off(int L) { return region_a(L) + (size_t)WAVE * packed_words<NW>() * 4; }
    static __host__ __device__ size_t bytes(int L) { return err_off(L) + (size_t)WAVE * 12; }
};

template <int NW, int LC, int VEC>
__global__ __launch_bounds__(BLOCK) void expand12_rows_kernel(ExpandArgs a) {
    static_assert(LC > 0 && LC % 4 == 0, "compile-time L, whole 16-byte chunks per relator");
    using Tile = TileFor<NW, LC, VEC>;
    using Smem = ExpandRowsSmem<NW, LC, VEC>;
    constexpr int PW = packed_words<NW>();
    constexpr int SW = Smem::SW;
    constexpr int L = LC, CPR = LC / 2, HC = LC / 4;  // 16-byte chunks per row / per relator
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const BlockCtx b = block_ctx();
    if (b.r0 >= a.N) return;  // block-uniform
    const int lane = b.lane, wid = b.wid, R = tile_rows(a.N, b.r0);
    const int64_t r0 = b.r0;
    uint32_t* packed = reinterpret_cast<uint32_t*>(smem + Smem::region_a(a.L));
    uint8_t* err_st = reinterpret_cast<uint8_t*>(smem + Smem::err_off(a.L));
    const bool cyc = a.cyclical != 0;
    Tile tile(smem, a.L);
    tile.load_block(a.parents + r0 * 2 * L, R);
    if (wid == 0) {
        if (lane < R) {
            PresRegs<NW> p;
            const bool bad = tile.pack(lane, p);
            const bool clean = !bad && is_clean<NW>(p.w0, p.n0, p.w1, p.n1, cyc);
            uint32_t* d = packed + lane * PW;  // (inline: staging a packed parent)
#pragma unroll
            for (int k = 0; k < NW; ++k) {
                d[k] = p.w0.w[k];
                d[NW + k] = p.w1.w[k];
            }
            d[2 * NW] = (uint32_t)p.n0 | ((uint32_t)p.n1 << 8);
            d[2 * NW + 1] = (uint32_t)bad | ((uint32_t)clean << 1);
        }
    }
    __syncthreads();  // the tile is dead from here: region a holds the staged children
    uint32_t* stw = reinterpret_cast<uint32_t*>(smem);
    int nerr = 0;
    if (lane < R) {
        PresRegs<NW> p;
        const uint32_t* d = packed + lane * PW;  // (inline: reading a staged parent back)
#pragma unroll
        for (int k = 0; k < NW; ++k) {
            p.w0.w[k] = d[k];
            p.w1.w[k] = d[NW + k];
        }
        p.n0 = (int)(d[2 * NW] & 0xffu);
        p.n1 = (int)((d[2 * NW] >> 8) & 0xffu);
        const bool bad = (d[2 * NW + 1] & 1u) != 0, clean = (d[2 * NW + 1] & 2u) != 0;
        const int64_t par = r0 + lane;
#pragma unroll 1
        for (int j = 0; j < KEYS_APW; ++j) {
            const int act = wid * KEYS_APW + j;
            PresRegs<NW> q = p;  // (inline: the move on a child)
            int e;
            if (bad) e = ACX_ERR_DOMAIN;
            else if (clean) e = ac_move_clean<NW>(q.w0, q.n0, q.w1, q.n1, act, L, cyc);
            else e = ac_move<NW>(q.w0, q.n0, q.w1, q.n1, act, L, cyc);
            nerr += e != ACX_ERR_NONE;
            err_st[lane * 12 + act] = (uint8_t)e;
            if (a.child_key) {  // keys as well (not the search path): per lane, unstaged
                PresRegs<NW> kq = q;
                if (e != ACX_ERR_NONE) {  // (inline: the sentinel)
                    kq.n0 = 0xff;
                    kq.n1 = 0xff;
                }
                store_key<NW>(a.child_key + (par * 12 + act) * a.kw64, a.kw64, L, kq);
            }
            uint32_t* c = stw + (lane * 12 + act) * SW;  // odd stride: conflict-free
#pragma unroll
            for (int k = 0; k < NW; ++k) {
                c[k] = q.w0.w[k];
                c[NW + k] = q.w1.w[k];
            }
            c[2 * NW] = (uint32_t)q.n0 | ((uint32_t)q.n1 << 8);
        }
    }
    __syncthreads();
    int4* dst = reinterpret_cast<int4*>(a.children + r0 * 12 * 2 * L);
    const int nch = R * 12 * CPR;
    for (int i = threadIdx.x; i < nch; i += BLOCK) {
        const int ci = i / CPR, k = i - ci * CPR;  // child (parent-major), 16-byte chunk of its row
        const int pp = ci / 12;
        int4 v;
        if (packed[pp * PW + 2 * NW + 1] & 1u) {  // out-of-domain parent: its row, as is
            v = reinterpret_cast<const int4*>(a.parents + (r0 + pp) * 2 * L)[k];
        } else {
            const uint32_t* c = stw + ci * SW;
            const int h = k >= HC ? 1 : 0, m = k - h * HC;
            const uint32_t c8 = (c[h * NW + (m >> 2)] >> (8 * (m & 3))) & 0xffu;
            const int n = (int)((c[2 * NW] >> (8 * h)) & 0xffu);
            v = widen4(codes_to_i8x4(c8, clamp_bits(8 * n - 32 * m)));
        }
        dst[i] = v;
    }
    if (a.child_len) {
        int32_t* ld = a.child_len + r0 * 24;
        for (int i = threadIdx.x; i < R * 24; i += BLOCK) ld[i] = (int32_t)((stw[(i >> 1) * SW + 2 * NW] >> (8 * (i & 1))) & 0xffu);
    }
    if (a.err) copy_run(a.err + r0 * 12, err_st, R * 12);
    if (nerr && a.err_count) atomicAdd(a.err_count, nerr);
}

// simplify_presentation (utils.py:246-283): assert valid, then reduce both relators
template <int NW, int LC, int VEC>
__global__ __launch_bounds__(BLOCK) void canon_kernel(CanonArgs a) {
    using Tile = TileFor<NW, LC, VEC>;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    WaveCtx w;
    if (!wave_ctx(a.B, w)) return;
    Tile tile(smem + w.wid * Tile::wave_bytes(a.L), a.L);
    const int L = tile.Lr(), twoL = 2 * L;
    const int64_t env = w.r0 + w.lane;
    tile.load(a.state_in + w.r0 * twoL, w.R, w.lane);
    bool bad = false;
    if (w.active) {
        PresRegs<NW> p;
        bad = tile.pack(w.lane, p);
        const int e = bad ? ACX_ERR_DOMAIN : ((p.n0 == 0 || p.n1 == 0) ? ACX_ERR_INVALID : ACX_ERR_NONE);
        if (e == ACX_ERR_NONE) {
            simplify<NW>(p.w0, p.n0, a.cyclical != 0);
            simplify<NW>(p.w1, p.n1, a.cyclical != 0);
            tile.unpack(w.lane, p);
        }
        if (a.lengths_out) {
            a.lengths_out[2 * env] = p.n0;
            a.lengths_out[2 * env + 1] = p.n1;
        }
        if (a.err) a.err[env] = (uint8_t)e;
        if (e != ACX_ERR_NONE && a.err_count) atomicAdd(a.err_count, 1);
    }
    tile.flag_rows(w.lane, bad ? FB_IN : 0u);  // incl. a zero inside a relator (not flagged by the load)
    wave_sync();
    tile.template store<true, NT_STATE>(a.state_out + w.r0 * twoL, twoL, w.R, a.state_in + w.r0 * twoL, twoL,
                                                 w.lane);
}

template <int NW, int LC, int VEC>
__global__ __launch_bounds__(BLOCK) void unpack_keys_kernel(UnpackArgs a) {
    using Tile = TileFor<NW, LC, VEC>;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    WaveCtx w;
    if (!wave_ctx(a.M, w)) return;
    Tile tile(smem + w.wid * Tile::wave_bytes(a.L), a.L);
    const int L = tile.Lr(), twoL = 2 * L;
    const int64_t k = w.r0 + w.lane;
    if (w.active) {
        PresRegs<NW> p;
        load_key<NW>(a.keys + k * a.kw64, a.kw64, L, p);
        tile.unpack(w.lane, p);
        if (a.lengths_out) {
            a.lengths_out[2 * k] = p.n0;
            a.lengths_out[2 * k + 1] = p.n1;
        }
    }
    wave_sync();
    tile.template store<false>(a.states + w.r0 * twoL, twoL, w.R, nullptr, 0, w.lane);
}

}  // namespace acx
