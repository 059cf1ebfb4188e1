// acx_tile_generic.h -- GenericTile: the LDS tile for a runtime L (parity at any L <= 128), letter
// by letter.  The interface the three tiles share is stated in acx_tile.h.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "acx_moves.h"
#include "acx_planes.h"
#include "acx_tile_io.h"

namespace acx {

template <int NW, int LC, int VEC>
struct GenericTile {
    static constexpr bool PREFETCH_OK = false;  // fetch_rows / put_rows: stubs (see the tile interface, acx_tile.h)
    static constexpr bool LIVE_ROWS = false;  // whole rows: set_lim is a no-op
    static constexpr int RPI = 1;
    __device__ __forceinline__ int4 fetch_rows(const int32_t*, uint64_t, int) const { return int4{0, 0, 0, 0}; }
    __device__ __forceinline__ void put_rows(const int4&, uint64_t, uint64_t, int) {}
    static constexpr bool NT_STEP_LOADS = false;  // see ld_tile
    static constexpr int LMAX = LC > 0 ? LC : 16 * NW;
    int L, twoL, rowb;
    char* base;
    uint8_t* flags;

    static __host__ __device__ int row_bytes(int L_) {
        const int bytes = (LC > 0) ? 2 * LC : (L_ + LMAX);
        return (((bytes + 3) >> 2) | 1) * 4;  // odd dword stride: conflict-free per-lane reads
    }
    static __host__ __device__ size_t wave_bytes(int L_) { return (size_t)WAVE * row_bytes(L_) + WAVE; }
    __device__ __forceinline__ GenericTile(char* b, int L_) {
        L = LC > 0 ? LC : L_;
        twoL = 2 * L;
        rowb = row_bytes(L);
        base = b;
        flags = reinterpret_cast<uint8_t*>(b + WAVE * rowb);
    }
    __device__ __forceinline__ int Lr() const { return L; }
    // contiguous rows
    template <bool NT>
    __device__ __forceinline__ void store_rows(int32_t* g, int R, int lane) const {
        store<false, NT>(g, 2 * L, R, nullptr, 0, lane);
    }
    // int8 rows, byte by byte (parity instantiations)
    template <bool NT>
    __device__ __forceinline__ void store_rows_i8(int8_t* g, int R, int lane) const {
        for (int i = lane; i < R * twoL; i += WAVE) g[i] = row(i / twoL)[i % twoL];
    }
    __device__ __forceinline__ void restore_flags(int lane, uint32_t code) {
        flags[lane] = (uint8_t)code;
        wave_sync();
    }
    __device__ __forceinline__ void flag_rows(int lane, uint32_t code) {
        if (code) flags[lane] = (uint8_t)code;
    }
    __device__ __forceinline__ int32_t letter(int r, int k) const { return row(r)[k]; }
    // the rows of the lanes in `rows` only, row by row (the generic-L instantiations serve
    // parity, not speed)
    __device__ __forceinline__ void load_rows(const int32_t* __restrict__ g, uint64_t rows, int R, int lane) {
        load_rows_from([&](int r) { return g + (int64_t)r * twoL; }, rows, R, lane);
    }
    template <class RowPtr>
    __device__ __forceinline__ void load_rows_from(RowPtr rp, uint64_t rows, int, int lane) {
        if ((rows >> lane) & 1ull) flags[lane] = 0;
        wave_sync();
        for (uint64_t m = rows; m; m &= m - 1) {
            const int r = __builtin_ctzll(m);
            const int32_t* row_src = rp(r);
            bool bad = false;
            for (int k = lane; k < twoL; k += WAVE)
                row(r)[k] = (int8_t)to_i8(row_src[k], bad);
            if (__any(bad) && lane == 0) flags[r] = 1;
        }
        wave_sync();
    }
    __device__ __forceinline__ int8_t* row(int r) const { return reinterpret_cast<int8_t*>(base + r * rowb); }

    // (row, pos) of a chunk of VEC int32; chunks never straddle rows (2L % VEC == 0)
    struct It {
        int row, pos, dq, dr, twoL;
        __device__ __forceinline__ It(int c0, int twoL_) : twoL(twoL_) {
            const int e0 = c0 * VEC;
            row = e0 / twoL;
            pos = e0 - row * twoL;
            dq = (WAVE * VEC) / twoL;
            dr = WAVE * VEC - dq * twoL;
        }
        __device__ __forceinline__ void next() {
            pos += dr;
            row += dq;
            if (pos >= twoL) { pos -= twoL; ++row; }
        }
    };

    // PIPE, LIVE: see CodeTile::load (the runtime-L path reads and writes whole rows)
    template <bool PIPE = false, bool LIVE = false, bool NTL = false, int BATCH = 0>
    __device__ __forceinline__ void load(const int32_t* __restrict__ g, int R, int lane) {
        flags[lane] = 0;
        wave_sync();
        const int nc = (R * twoL) / VEC;
        It it(lane, twoL);
        for (int b0 = lane; b0 < nc; b0 += WAVE * STAGE_UNROLL) {
            int rows[STAGE_UNROLL], poss[STAGE_UNROLL];
            int32_t v[STAGE_UNROLL][VEC];
#pragma unroll
            for (int u = 0; u < STAGE_UNROLL; ++u) {
                rows[u] = it.row;
                poss[u] = it.pos;
                it.next();
                if (b0 + u * WAVE < nc) {
                    const int32_t* src = g + (int64_t)rows[u] * twoL + poss[u];
                    if constexpr (VEC == 4) {
                        const int4 x = *reinterpret_cast<const int4*>(src);
                        v[u][0] = x.x; v[u][1] = x.y; v[u][2] = x.z; v[u][3] = x.w;
                    } else {
                        const int2 x = *reinterpret_cast<const int2*>(src);
                        v[u][0] = x.x; v[u][1] = x.y;
                    }
                }
            }
#pragma unroll
            for (int u = 0; u < STAGE_UNROLL; ++u) {
                if (b0 + u * WAVE < nc) {
                    bool bad = false;
                    char* dst = base + rows[u] * rowb + poss[u];
                    if constexpr (VEC == 4) {
                        *reinterpret_cast<uint32_t*>(dst) = to_i8(v[u][0], bad) | (to_i8(v[u][1], bad) << 8) |
                                                            (to_i8(v[u][2], bad) << 16) | (to_i8(v[u][3], bad) << 24);
                    } else {
                        *reinterpret_cast<uint16_t*>(dst) = (uint16_t)(to_i8(v[u][0], bad) | (to_i8(v[u][1], bad) << 8));
                    }
                    if (bad) flags[rows[u]] = 1;
                }
            }
        }
        wave_sync();
    }

    template <bool FB, bool NT = false, bool F32 = false>
    __device__ __forceinline__ void store(int32_t* g, int64_t gpitch, int R, const int32_t* fallback,
                                          int64_t fpitch, int lane, const int32_t* fallback2 = nullptr,
                                          uint64_t skip = 0) const {  // skip: see FastTile::store
        const int nc = (R * twoL) / VEC;
        It it(lane, twoL);
        for (int b0 = lane; b0 < nc; b0 += WAVE * STAGE_UNROLL) {
            int rows[STAGE_UNROLL], poss[STAGE_UNROLL];
            uint32_t p[STAGE_UNROLL];
#pragma unroll
            for (int u = 0; u < STAGE_UNROLL; ++u) {
                rows[u] = it.row;
                poss[u] = it.pos;
                it.next();
                p[u] = 0;
                if (b0 + u * WAVE < nc) {
                    const char* src = base + rows[u] * rowb + poss[u];
                    if constexpr (VEC == 4) p[u] = *reinterpret_cast<const uint32_t*>(src);
                    else p[u] = *reinterpret_cast<const uint16_t*>(src);
                }
            }
#pragma unroll
            for (int u = 0; u < STAGE_UNROLL; ++u) {
                if (b0 + u * WAVE >= nc || ((skip >> rows[u]) & 1ull)) continue;
                int32_t* dst = g + (int64_t)rows[u] * gpitch + poss[u];
                const uint32_t fc = FB ? flags[rows[u]] : 0u;
                const bool fb = fc != 0u;
                const int32_t* f = fb_src(fc, fallback, fallback2) + (int64_t)rows[u] * fpitch + poss[u];
                if constexpr (VEC == 4) {
                    out16<false, F32>(reinterpret_cast<int4*>(dst), fb ? *reinterpret_cast<const int4*>(f) : widen4(p[u]));
                } else {
                    int2 x;
                    x.x = (int32_t)(int8_t)(p[u] & 0xffu);
                    x.y = (int32_t)(int8_t)((p[u] >> 8) & 0xffu);
                    out8<F32>(reinterpret_cast<int2*>(dst), fb ? *reinterpret_cast<const int2*>(f) : x);
                }
            }
        }
    }

    // ---- bit-plane registers (acx_planes.h; the env-step kernels), letter by letter ----
    static constexpr int PW = PlaneWords<NW>::value;
    __device__ __forceinline__ void pack_relator(const int8_t* src, Planes<PW>& w, int& n, bool& bad) const {
#pragma unroll
        for (int j = 0; j < PW; ++j) w.s[j] = w.y[j] = 0ull;
        n = 0;
        bool zero_seen = false;
#pragma unroll
        for (int k = 0; k < LMAX; ++k) {
            int b = src[k];
            if (LC == 0) b = (k < L) ? b : 0;
            const bool nz = b != 0;
            w.s[k >> 6] |= (uint64_t)(nz && b < 0) << (k & 63);
            w.y[k >> 6] |= (uint64_t)(nz && (b & 1) == 0) << (k & 63);
            n += nz;
            bad |= nz && zero_seen;
            zero_seen |= !nz;
        }
    }
    template <bool LIVE = false>  // LIVE: ignored (see the tile interface, acx_tile.h)
    __device__ __forceinline__ bool pack(int lane, PlaneRegs<PW>& p) const {
        const int8_t* r = row(lane);
        bool bad = flags[lane] != 0;
        pack_relator(r, p.w0, p.n0, bad);
        pack_relator(r + L, p.w1, p.n1, bad);
        return bad;
    }
    __device__ __forceinline__ void unpack_relator(int8_t* dst, const Planes<PW>& w, int n) const {
#pragma unroll
        for (int k = 0; k < LMAX; ++k) {
            const uint32_t code = (uint32_t)(((w.y[k >> 6] >> (k & 63)) & 1ull) << 1 | ((w.s[k >> 6] >> (k & 63)) & 1ull));
            const uint32_t letter = (0xFE02FF01u >> (code << 3)) & 0xffu;  // code -> 1, -1, 2, -2
            if (LC > 0 || k < L) dst[k] = (int8_t)(k < n ? letter : 0u);
        }
    }
    __device__ __forceinline__ void unpack(int lane, const PlaneRegs<PW>& p) const {
        int8_t* r = row(lane);
        unpack_relator(r, p.w0, p.n0);
        unpack_relator(r + L, p.w1, p.n1);
    }
    __device__ __forceinline__ void unpack_half(int lane, const PlaneRegs<PW>& p, bool h1) const {
        unpack_relator(row(lane) + (h1 ? L : 0), pl::psel<PW>(h1, p.w1, p.w0), h1 ? p.n1 : p.n0);
    }
    template <bool LIVE = false>  // LIVE: ignored (see the tile interface, acx_tile.h)
    __device__ __forceinline__ uint32_t unpack_dirty(int lane, const PlaneRegs<PW>& p) const {
        unpack(lane, p);
        return 3u;
    }

    __device__ __forceinline__ void pack_relator(const int8_t* src, Word<NW>& w, int& n, bool& bad) const {
        w = wzero<NW>();
        n = 0;
        bool zero_seen = false;
#pragma unroll
        for (int k = 0; k < LMAX; ++k) {
            int b = src[k];
            if (LC == 0) b = (k < L) ? b : 0;
            const bool nz = b != 0;
            const uint32_t code = nz ? ((((uint32_t)~b & 1u) << 1) | (((uint32_t)b >> 7) & 1u)) : 0u;
            w.w[k >> 4] |= code << (2 * (k & 15));
            n += nz;
            bad |= nz && zero_seen;
            zero_seen |= !nz;
        }
    }
    __device__ __forceinline__ bool pack(int lane, PresRegs<NW>& p) const {
        const int8_t* r = row(lane);
        bool bad = flags[lane] != 0;
        pack_relator(r, p.w0, p.n0, bad);
        pack_relator(r + L, p.w1, p.n1, bad);
        return bad;
    }
    __device__ __forceinline__ void unpack_relator(int8_t* dst, const Word<NW>& w, int n) const {
#pragma unroll
        for (int k = 0; k < LMAX; ++k) {
            const uint32_t code = (w.w[k >> 4] >> (2 * (k & 15))) & 3u;
            const uint32_t letter = (0xFE02FF01u >> (code << 3)) & 0xffu;  // code -> 1, -1, 2, -2
            if (LC > 0 || k < L) dst[k] = (int8_t)(k < n ? letter : 0u);
        }
    }
    __device__ __forceinline__ void unpack(int lane, const PresRegs<NW>& p) const {
        int8_t* r = row(lane);
        unpack_relator(r, p.w0, p.n0);
        unpack_relator(r + L, p.w1, p.n1);
    }
    // relator h1 of the lane's row only (the rollout's clean moves change one relator)
    __device__ __forceinline__ void unpack_half(int lane, const PresRegs<NW>& p, bool h1) const {
        unpack_relator(row(lane) + (h1 ? L : 0), wsel<NW>(h1, p.w1, p.w0), h1 ? p.n1 : p.n0);
    }
    // runtime-L tiles (parity tests at any L) track no dirty relators: every row is written
    __device__ __forceinline__ uint32_t unpack_dirty(int lane, const PresRegs<NW>& p) const {
        unpack(lane, p);
        return 3u;
    }
    __device__ __forceinline__ void set_dirty(int, uint32_t) const {}
    __device__ __forceinline__ void set_lim(int, int, int) const {}  // whole rows: stubs (see the tile interface, acx_tile.h)
    __device__ __forceinline__ void widen_lim(int, int, int) const {}
    template <bool NT, bool LIVE = false>
    __device__ __forceinline__ void store_dirty(int32_t* g, int R, int lane, const int32_t* fallback2 = nullptr) const {
        store<true, NT>(g, twoL, R, g, twoL, lane, fallback2);
    }
};

}  // namespace acx
