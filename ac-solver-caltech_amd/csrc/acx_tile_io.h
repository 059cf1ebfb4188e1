// acx_tile_io.h -- what moves a tile of rows between HBM and LDS: the wave-level barrier, the
// int32 <-> int8 letter and 2-bit code conversions, the 16-byte load / store helpers with their
// cache-policy constants, and the fallback-row codes of rows outside the packed domain.  Used by
// the tile classes (acx_tile_code.h, acx_tile_fast.h, acx_tile_generic.h; their interface is in
// acx_tile.h) and by the kernels.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace acx {

__device__ __forceinline__ void wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// int32 letter -> int8; values outside {-2..2} become 0x7F and set `bad`
__device__ __forceinline__ uint32_t to_i8(int32_t v, bool& bad) {
    const bool ok = (uint32_t)(v + 2) <= 4u;
    bad |= !ok;
    return ok ? ((uint32_t)v & 0xffu) : 0x7fu;
}

__device__ __forceinline__ int4 widen4(uint32_t p) {
    int4 x;
    x.x = (int32_t)(int8_t)(p & 0xffu);
    x.y = (int32_t)(int8_t)((p >> 8) & 0xffu);
    x.z = (int32_t)(int8_t)((p >> 16) & 0xffu);
    x.w = (int32_t)(int8_t)(p >> 24);
    return x;
}


constexpr int STAGE_UNROLL = 8;
// Cache-policy choices, each settled by an interleaved A/B on one buffer set (the measurements
// are cited where each is used; the losing variants live in commit history, not here):
//   * the rollout's write-once trajectory: non-temporal / sc1 stores (1.4 % faster at T = 200);
//     its reward/done/truncated stay plain (non-temporal cost 0.4 %);
//   * the in-place step's write-back of changed relators: non-temporal (L = 36) or an sc1
//     buffer store (L = 128); whole output rows stay plain;
//   * tile loads: non-temporal for the L = 128 step and the rollout's state in, plain for the
//     L = 36 step; expand12's parent loads and key stores non-temporal.
constexpr bool NT_OBS = true;

typedef int v4i_t __attribute__((ext_vector_type(4)));
template <bool NT>
__device__ __forceinline__ void st16(int4* p, const int4& v) {
    if constexpr (NT) {
        const v4i_t x = {v.x, v.y, v.z, v.w};
        __builtin_nontemporal_store(x, reinterpret_cast<v4i_t*>(p));
    } else {
        *p = v;
    }
}
// 16 bytes of a row: int32 letters, or (F32) the same letters as float32 (the PPO learner's
// observation buffer, training.py:151-153)
template <bool NT, bool F32>
__device__ __forceinline__ void out16(int4* p, const int4& v) {
    if constexpr (F32) {
        typedef float v4f_t __attribute__((ext_vector_type(4)));
        const v4f_t f = {(float)v.x, (float)v.y, (float)v.z, (float)v.w};
        if constexpr (NT) __builtin_nontemporal_store(f, reinterpret_cast<v4f_t*>(p));
        else *reinterpret_cast<v4f_t*>(p) = f;
    } else {
        st16<NT>(p, v);
    }
}
template <bool F32>
__device__ __forceinline__ void out8(int2* p, const int2& v) {
    if constexpr (F32) {
        float2 f;
        f.x = (float)v.x;
        f.y = (float)v.y;
        *reinterpret_cast<float2*>(p) = f;
    } else {
        *p = v;
    }
}
template <bool NT, class T>
__device__ __forceinline__ void st_scalar(T* p, T v) {
    if constexpr (NT) __builtin_nontemporal_store(v, p);
    else *p = v;
}

// 4 int8 letters (one dword) -> 8-bit code field (2 bits per letter, x=0 X=1 y=2 Y=3, zero
// letters -> 0) and a 4-bit non-zero mask.  A letter's low 3 bits index an 8-entry byte table
// (v_perm_b32: 0 -> 0, 1 (x), 2 (y), 6 (Y = -2), 7 (X = -1)), and v_dot4_u32_u8 folds the four
// per-byte results into their fields (weights 1, 4, 16, 64 for the codes, 1, 2, 4, 8 for the
// mask): 6 VALU where a shift-and-mask SWAR took ~16.  Bytes outside {0, +-1, +-2} give
// arbitrary codes (their rows are flagged and never decoded from the tile); 0x7F, to_i8's
// out-of-domain byte, counts as non-zero.
__device__ __forceinline__ void pack4_codes(uint32_t d, uint32_t& c8, uint32_t& nz4) {
    const uint32_t m = d & 0x07070707u;
    const uint32_t codes = __builtin_amdgcn_perm(0x01030000u, 0x00020000u, m);
    const uint32_t nz = __builtin_amdgcn_perm(0x01010101u, 0x01010100u, m);
    c8 = __builtin_amdgcn_udot4(codes, 0x40100401u, 0u, false);
    nz4 = __builtin_amdgcn_udot4(nz, 0x08040201u, 0u, false);
}

// Non-temporal stores for the in-place step's write-back of changed relators: nothing reads
// those lines again inside the launch, and plain stores kept them in L2 beside the tile loads
// (same buffers: L = 128 0.2727 -> 0.2581 ms, lengths-carrying 0.2302 -> 0.2102, L = 36
// 0.0742 -> 0.0697; profiles/r04/r04z_ab_nt*.json).  Whole output rows (the out-of-place step,
// the rollout's final state, canonicalized rows, expanded children) stay plain: non-temporal
// made the rollout slower (K = 20 int32 1.332 -> 1.351 ms, int8 0.447 -> 0.477; its next launch
// reads that state) and expand12's children no faster (0.778 -> 0.772 ms).
constexpr bool NT_WRITEBACK = true;
constexpr bool NT_STATE = false;
// Buffer-instruction cache policies (gfx950 cpol bits: sc0 1, nt 2, sc1 16).
// The L = 128 in-place step's write-back (CodeTile): sc1, same buffers: lengths-carrying 0.1993 ->
// 0.1791 ms, acx_step 0.2423 -> 0.2182 against nt; nt + sc1 0.1989 (profiles/r04/r04s_ab_wb_cpol.json).
// FastTile (L = 36) keeps the global non-temporal write-back: sc1 measured 0.0757 vs nt 0.0698 ms
// per 2^20-env step (r04s_ab_wb36_cpol.json).
constexpr int WB_CPOL = 16;
// The rollout's int32 trajectory stores (full tiles): sc1 (the line is not kept in the XCD's L2):
// same buffers, K = 20 on Samsung boxes 1.2377 -> 1.2059 and 1.3241 -> 1.3027 ms against nt,
// plain 1.2267 / 1.3195; K = 200 within 0.3 % (profiles/r04/r04s_ab_obs_cpol*.json).  The int8
// trajectory keeps global non-temporal stores: K = 20 0.4626 ms vs sc1 0.4862, plain 0.494
// (r04s_ab_obs8_cpol.json).
constexpr int OBS_CPOL = 16;
// expand12's parent loads and packed-key stores non-temporal (keys as 16-B stores): same buffers,
// 4M parents (profiles/r04/r04z_ab_keys.json): 0.4246 ms (0.71 of 8 TB/s) -> 0.380 ms (0.79) with
// both; the loads alone 0.4085, the stores alone 0.5101 (slower); the children kernel unchanged
constexpr bool NT_EXPAND_LOADS = true;
constexpr bool NT_KEYS = true;
// Non-temporal tile loads (NTL): the state rows are read once per launch.  Taken where it
// measured faster (same buffers, profiles/r04/r04z_ab_ld*.json): the L = 128 step (CodeTile:
// 0.2587 -> 0.2432 ms, lengths-carrying 0.2105 -> 0.1991) and the rollout's state in (int8
// trajectory 0.4635 -> 0.4402 ms, int32 1.3235 -> 1.3131); not the L = 36 step, whose write-back
// of relators that are not sector-aligned (288-B rows) then went 0.0699 -> 0.0944 ms.
template <bool NT>
__device__ __forceinline__ int4 ld_tile(const int4* p) {
    if constexpr (NT) {
        const v4i_t x = __builtin_nontemporal_load(reinterpret_cast<const v4i_t*>(p));
        return make_int4(x[0], x[1], x[2], x[3]);
    } else {
        return *p;
    }
}
constexpr int tile_cpol(bool nt) { return nt ? 2 : 0; }  // buffer-load cache policy: nt (gfx94x/950 bits)
// 16 bytes of a row (4 int32 letters) -> the dword of their low bytes (2 v_perm_b32 + or);
// bad = a letter outside {-2..2} (max / min of the four).  A bad chunk's bytes are arbitrary:
// its row is flagged and never decoded from the tile.
__device__ __forceinline__ uint32_t chunk_i8(const int4& v, bool& bad) {
    const uint32_t lo = __builtin_amdgcn_perm((uint32_t)v.y, (uint32_t)v.x, 0x0c0c0400u);  // x.b0, y.b0
    const uint32_t hi = __builtin_amdgcn_perm((uint32_t)v.w, (uint32_t)v.z, 0x04000c0cu);  // z.b0, w.b0
    const int mx = max(max(v.x, v.y), max(v.z, v.w));
    const int mn = min(min(v.x, v.y), min(v.z, v.w));
    bad = mx > 2 || mn < -2;
    return lo | hi;
}

// chunk_i8 with the range test folded into a running max / min of the letters (two v_max3 and
// two v_min3 per chunk, no compare): some letter is outside {-2..2} <=> mx > 2 or mn < -2
__device__ __forceinline__ uint32_t chunk_i8_acc(const int4& v, int& mx, int& mn) {
    const uint32_t lo = __builtin_amdgcn_perm((uint32_t)v.y, (uint32_t)v.x, 0x0c0c0400u);
    const uint32_t hi = __builtin_amdgcn_perm((uint32_t)v.w, (uint32_t)v.z, 0x04000c0cu);
    mx = max(max(mx, v.x), v.y);
    mx = max(max(mx, v.z), v.w);
    mn = min(min(mn, v.x), v.y);
    mn = min(min(mn, v.z), v.w);
    return lo | hi;
}

// 8-bit code field -> 4 int8 letters, the first s/8 kept (s = 8m, m = 0..4), the rest zero.
// The four 2-bit codes are spread to one per byte (two shift-or-mask rounds); a byte past m
// gets selector bit 2 set, so one v_perm_b32 reads either the letter table {1,-1,2,-2}
// (src1 bytes 0..3) or zero (src0 bytes 4..7).  ~7 full-rate VALU ops per 4 letters.
__device__ __forceinline__ uint32_t codes_to_i8x4(uint32_t c8, uint32_t s) {
    uint32_t x = (c8 | (c8 << 12)) & 0x000F000Fu;
    x = (x | (x << 6)) & 0x03030303u;
    const uint32_t z = (uint32_t)(0x04040404ull << s);  // 0x04 in bytes >= m (s = 32 -> none)
    return __builtin_amdgcn_perm(0u, 0xFE02FF01u, x | z);
}
__device__ __forceinline__ uint32_t clamp_bits(int s) { return (uint32_t)(s < 0 ? 0 : (s > 32 ? 32 : s)); }

// Rows outside the packed domain (a letter not in {-2..2}, a zero inside a relator) cannot be
// held in the LDS image; the stores copy their exact int32 values from a fallback row instead,
// chosen per row by its code in the tile's flags[]:
//   FB_IN     the row the kernel loaded (state_in / the rollout's input state)
//   FB_RESET  the env's starting row (reset_state): an autoreset to an out-of-domain row
constexpr uint32_t FB_IN = 1u, FB_RESET = 2u;
__device__ __forceinline__ const int32_t* fb_src(uint32_t code, const int32_t* fb_in, const int32_t* fb_reset) {
    return code == FB_RESET ? fb_reset : fb_in;
}

}  // namespace acx
