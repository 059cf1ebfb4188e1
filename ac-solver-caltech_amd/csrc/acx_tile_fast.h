// acx_tile_fast.h -- FastTile: the LDS tile for a compile-time L with L % 4 == 0 below 64 (L = 36).
// The interface the three tiles share is stated in acx_tile.h.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "acx_moves.h"
#include "acx_planes.h"
#include "acx_tile_base.h"
#include "acx_tile_io.h"

namespace acx {

// LDS row stride (dwords) of the int8 image of a row of 2L letters: = 2 mod 4
constexpr int fast_tile_stride(int L) { return ((L / 2) % 4 == 2) ? L / 2 : L / 2 + 2; }

template <int NW, int LC>
struct FastTile : PackedTileBase<LC, fast_tile_stride(LC)> {
    static_assert(LC > 0 && LC % 4 == 0, "FastTile needs a compile-time L multiple of 4");
    using Base = PackedTileBase<LC, fast_tile_stride(LC)>;
    using Base::lds;
    using Base::flags;
    using Base::dirty;
    using Base::lim;
    using Base::live;
    using Base::live_chunks;
    static constexpr int L = LC;
    static constexpr int twoL = 2 * LC;
    static constexpr int CPR = LC / 2;  // 16-byte chunks (4 letters) per row
    static constexpr int S = Base::S;
    static constexpr int HALF = CPR / 2;  // dwords per relator
    static_assert(S % 4 == 2, "row stride must be 2 mod 4 dwords");
    static constexpr int LOAD_BATCH = 6;

    bool tile_bad = false;  // wave-uniform: some row of the last load was flagged
    __device__ __forceinline__ void restore_flags(int lane, uint32_t code) { tile_restore_flags(flags, tile_bad, lane, code); }
    __device__ __forceinline__ void flag_rows(int lane, uint32_t code) { tile_flag_rows(flags, tile_bad, lane, code); }
    // int8 letter k of row r of the LDS image (the rare fallback stores)
    __device__ __forceinline__ int32_t letter(int r, int k) const { return row(r)[k]; }
    __device__ __forceinline__ FastTile(char* base, int) : Base(base) {}
    // lengths-carrying step: row `lane` has relators of n0 / n1 letters -> its live chunk counts
    __device__ __forceinline__ void set_lim(int lane, int n0, int n1) const {
        lim[2 * lane] = (uint8_t)live_chunks(n0);
        lim[2 * lane + 1] = (uint8_t)live_chunks(n1);
    }
    // before the store: the live chunks of the row's old (set_lim) or new letters n0 / n1
    __device__ __forceinline__ void widen_lim(int lane, int n0, int n1) const {
        const int a = live_chunks(n0), b = live_chunks(n1);
        if (a > lim[2 * lane]) lim[2 * lane] = (uint8_t)a;
        if (b > lim[2 * lane + 1]) lim[2 * lane + 1] = (uint8_t)b;
    }
    __device__ __forceinline__ int8_t* row(int r) const { return reinterpret_cast<int8_t*>(lds + r * S); }

    // LDS dword index of chunk c = lane + 64u (compile-time u)
    __device__ __forceinline__ static int lds_index(int ln, int u) {
        if constexpr (S == CPR) return ln + WAVE * u;           // unpadded: LDS image is flat
        else if constexpr (CPR == WAVE) return u * S + ln;      // one row per wave-instruction
        else {
            const int c = ln + WAVE * u;
            const int r = c / CPR;
            return r * S + (c - r * CPR);
        }
    }

    // global rows (contiguous, 2L int32 each) -> LDS (PIPE: see CodeTile::load; this full-tile
    // loop is unrolled already).  LIVE (the lengths-carrying step; lim[] set for every row): only
    // the chunks inside each relator's letters are read, the rest of the image is zero (the rows
    // are canonical: letters, then zero padding)
    template <bool PIPE = false, bool LIVE = false, bool NTL = false, int BATCH = 0>
    __device__ __forceinline__ void load(const int32_t* __restrict__ g, int R, int lane) {
        int ln = lane;
        asm volatile("" : "+v"(ln));  // keep the address math here (no hoisting into the caller)
        flags[ln] = 0;
        wave_sync();
        const int nc = R * CPR;
        const int4* src = reinterpret_cast<const int4*>(g) + ln;
        bool any_bad = false;
        if (R == WAVE) {  // full tile (wave-uniform): unguarded, LOAD_BATCH loads in flight
            // LIVE: loads through a buffer descriptor over the tile's rows, a dead chunk at an
            // out-of-range offset (zeros, nothing read): no load under a branch (see CodeTile::load)
            const uint64_t gb = reinterpret_cast<uint64_t>(g);
            const uint32_t glo = __builtin_amdgcn_readfirstlane((uint32_t)gb);
            const uint32_t ghi = __builtin_amdgcn_readfirstlane((uint32_t)(gb >> 32));
            const __amdgpu_buffer_rsrc_t rows = __builtin_amdgcn_make_buffer_rsrc(
                reinterpret_cast<void*>(((uint64_t)ghi << 32) | glo), (short)0, WAVE * CPR * 16, 0x00020000);
            // BATCH (the small-batch step instance): loads in flight per batch, up to the whole
            // tile row (CPR: one round trip); LOAD_BATCH otherwise (the 8-wave/SIMD VGPR budget)
            constexpr int LB = BATCH > 0 ? BATCH : LOAD_BATCH;
#pragma unroll
            for (int u0 = 0; u0 < CPR; u0 += LB) {
                int4 v[LB];
                bool lv[LB];
#pragma unroll
                for (int u = 0; u < LB; ++u) {
                    if (u0 + u >= CPR) continue;
                    const int c = ln + (u0 + u) * WAVE;
                    lv[u] = true;
                    if constexpr (LIVE) {
                        const uint32_t off = live(c / CPR, c % CPR) ? (uint32_t)c * 16u : 0x80000000u;
                        const auto x = __builtin_amdgcn_raw_buffer_load_b128(rows, off, 0, tile_cpol(NTL));
                        v[u] = make_int4((int)x[0], (int)x[1], (int)x[2], (int)x[3]);
                    } else {
                        v[u] = ld_tile<NTL>(src + (u0 + u) * WAVE);
                    }
                }
#pragma unroll
                for (int u = 0; u < LB; ++u) {
                    if (u0 + u >= CPR) continue;
                    bool bad = false;
                    uint32_t p = 0;
                    if (lv[u]) p = chunk_i8(v[u], bad);
                    lds[lds_index(ln, u0 + u)] = p;
                    if (bad) flags[(ln + (u0 + u) * WAVE) / CPR] = 1;
                    any_bad |= bad;
                }
            }
        } else {
            for (int u = 0; u < CPR; ++u) {
                const int c = ln + u * WAVE;
                if (c < nc) {
                    const int r = c / CPR;
                    bool bad = false;
                    uint32_t p = 0;
                    if (!LIVE || live(r, c - r * CPR)) {
                        const int4 v = ld_tile<NTL>(src + u * WAVE);
                        p = to_i8(v.x, bad) | (to_i8(v.y, bad) << 8) | (to_i8(v.z, bad) << 16) | (to_i8(v.w, bad) << 24);
                    }
                    lds[r * S + (c - r * CPR)] = p;
                    if (bad) flags[r] = 1;
                    any_bad |= bad;
                }
            }
        }
        tile_bad = __any(any_bad);
        wave_sync();
        if (tile_bad) {
            // rare (wave-uniform): chunk_i8 left arbitrary bytes in the flagged rows; their image
            // is rebuilt with to_i8 (an out-of-domain letter -> 0x7f), so the letter counts the
            // contract reports for them (reward, lengths) are those of the input row
            if (ln < R && flags[ln]) {
                const int4* row = reinterpret_cast<const int4*>(g) + (int64_t)ln * CPR;
                for (int k = 0; k < CPR; ++k) {
                    if (LIVE && !live(ln, k)) continue;
                    const int4 v = row[k];
                    bool b = false;
                    lds[ln * S + k] = to_i8(v.x, b) | (to_i8(v.y, b) << 8) | (to_i8(v.z, b) << 16) | (to_i8(v.w, b) << 24);
                }
            }
            wave_sync();
        }
    }

    // all BLOCK threads load R rows into this tile (the block's one): consecutive threads on
    // consecutive 16-byte chunks, every load issued before any conversion; flags as load().
    // Block-wide barriers before and after (the expand kernels' shared parent tile: a quarter of
    // the per-lane round trips of one wave loading all 64 rows while three wait).
    __device__ __forceinline__ void load_block(const int32_t* __restrict__ g, int R) {
        constexpr int U = (WAVE * CPR + BLOCK - 1) / BLOCK;
        if (threadIdx.x < WAVE) flags[threadIdx.x] = 0;
        __syncthreads();
        const int nc = R * CPR;
        const int4* src = reinterpret_cast<const int4*>(g);
        int4 v[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int c = (int)threadIdx.x + u * BLOCK;
            if (c < nc) v[u] = ld_tile<NT_EXPAND_LOADS>(src + c);
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int c = (int)threadIdx.x + u * BLOCK;
            if (c >= nc) continue;
            bool bad = false;
            const uint32_t q = to_i8(v[u].x, bad) | (to_i8(v[u].y, bad) << 8) | (to_i8(v[u].z, bad) << 16) |
                               (to_i8(v[u].w, bad) << 24);
            const int r = c / CPR;
            lds[r * S + (c - r * CPR)] = q;
            if (bad) flags[r] = 1;
        }
        __syncthreads();
    }

    // the rows of the lanes in the wave-uniform mask `rows` only (a few resetting envs),
    // cooperatively: lane l loads 16-byte chunk l % CPR of the (l / CPR)-th selected row, so a
    // wave-instruction fetches 64 / CPR whole rows (3 at L = 36) with one round trip per group
    __device__ __forceinline__ void load_rows(const int32_t* __restrict__ g, uint64_t rows, int R, int lane) {
        load_rows_from([&](int r) { return g + (int64_t)r * twoL; }, rows, R, lane);
    }
    // rp(r): row r's source (called by every lane of the wave: it may read across lanes)
    template <class RowPtr>
    __device__ __forceinline__ void load_rows_from(RowPtr rp, uint64_t rows, int, int lane) {
        constexpr int RPI = WAVE / CPR;
        static_assert(RPI >= 1, "a row must fit one wave-instruction");
        const int s = lane / CPR, c = lane - s * CPR;
        const int n = __popcll(rows);
        if ((rows >> lane) & 1ull) flags[lane] = 0;
        wave_sync();
        bool any_bad = false;
        for (int k0 = 0; k0 < n; k0 += RPI) {
            const int k = k0 + s;
            const bool on = s < RPI && k < n;
            uint64_t m = rows;
            for (int i = 0; i < (on ? k : 0); ++i) m &= m - 1;
            const int r = __builtin_ctzll(m);
            const int32_t* row_src = rp(r);
            if (on) {
                const int4 v = reinterpret_cast<const int4*>(row_src)[c];
                bool bad = false;
                lds[r * S + c] = to_i8(v.x, bad) | (to_i8(v.y, bad) << 8) | (to_i8(v.z, bad) << 16) |
                                 (to_i8(v.w, bad) << 24);
                if (bad) flags[r] = 1;
                any_bad |= bad;
            }
        }
        tile_bad = tile_bad || __any(any_bad);
        wave_sync();
    }

    // load_rows in two halves, for rows known before they are needed (an env step's truncations:
    // step_count + 1 >= horizon before the move): fetch_rows issues the loads of the rows in the
    // wave-uniform mask `rows` (at most RPI of them: one wave-instruction) and returns each lane's
    // chunk; put_rows later writes the rows in `apply` (a subset) into the tile, as load_rows does
    static constexpr bool PREFETCH_OK = true;
    static constexpr bool LIVE_ROWS = true;  // set_lim selects the chunks a live load reads
    static constexpr int RPI = WAVE / CPR;  // rows per wave-instruction
    __device__ __forceinline__ int4 fetch_rows(const int32_t* __restrict__ g, uint64_t rows, int lane) const {
        const int s = lane / CPR, c = lane - s * CPR;
        uint64_t m = rows;
        for (int i = 0; i < (s < RPI ? s : 0); ++i) m &= m - 1;
        int4 v = {0, 0, 0, 0};
        if (s < RPI && m) v = reinterpret_cast<const int4*>(g + (int64_t)__builtin_ctzll(m) * twoL)[c];
        return v;
    }
    __device__ __forceinline__ void put_rows(const int4& v, uint64_t rows, uint64_t apply, int lane) {
        const int s = lane / CPR, c = lane - s * CPR;
        uint64_t m = rows;
        for (int i = 0; i < (s < RPI ? s : 0); ++i) m &= m - 1;
        if ((apply >> lane) & 1ull) flags[lane] = 0;
        wave_sync();
        bool bad = false;
        if (s < RPI && m) {
            const int r = __builtin_ctzll(m);
            if ((apply >> r) & 1ull) {
                lds[r * S + c] = to_i8(v.x, bad) | (to_i8(v.y, bad) << 8) | (to_i8(v.z, bad) << 16) |
                                 (to_i8(v.w, bad) << 24);
                if (bad) flags[r] = 1;
            }
        }
        tile_bad = tile_bad || __any(bad);
        wave_sync();
    }

    template <bool NT, bool F32, bool FULL, int UB = 0, int UE = CPR>
    __device__ __forceinline__ void store_flat(int4* dst, int ln, int nc) const {
#pragma unroll
        for (int u0 = UB; u0 < UE; u0 += STAGE_UNROLL) {
            uint32_t p[STAGE_UNROLL];
#pragma unroll
            for (int u = 0; u < STAGE_UNROLL; ++u)
                if (u0 + u < UE && (FULL || ln + (u0 + u) * WAVE < nc)) p[u] = lds[lds_index(ln, u0 + u)];
#pragma unroll
            for (int u = 0; u < STAGE_UNROLL; ++u)
                if (u0 + u < UE && (FULL || ln + (u0 + u) * WAVE < nc))
                    out16<NT, F32>(dst + (u0 + u) * WAVE, widen4(p[u]));
        }
    }

    // LDS -> R contiguous global rows, EXACTLY CPR store instructions on every path (a partial
    // tile's spare lanes re-store its last chunk, same data to the same address), so the
    // compiler's waitcnt pass can count them (rollout_kernel's one-step-ahead action load).
    // [UB, UE): a range of the lane's chunk slots only (the rollout's split obs store)
    static constexpr bool NT_STEP_LOADS = false;  // see ld_tile
    template <bool NT, int UB = 0, int UE = CPR>
    __device__ __forceinline__ void store_rows(int32_t* g, int R, int lane) const {
        int ln = lane;
        asm volatile("" : "+v"(ln));
        int4* dst = reinterpret_cast<int4*>(g);
        const int nc = R * CPR;
        if (R == WAVE) {
            if constexpr (NT) {  // the trajectory store with an explicit cache policy (OBS_CPOL)
                const uint64_t b = reinterpret_cast<uint64_t>(g);
                const uint32_t lo = __builtin_amdgcn_readfirstlane((uint32_t)b);
                const uint32_t hi = __builtin_amdgcn_readfirstlane((uint32_t)(b >> 32));
                const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(
                    reinterpret_cast<void*>(((uint64_t)hi << 32) | lo), (short)0, WAVE * CPR * 16, 0x00020000);
#pragma unroll
                for (int u0 = UB; u0 < UE; u0 += STAGE_UNROLL) {
                    uint32_t p[STAGE_UNROLL];
#pragma unroll
                    for (int u = 0; u < STAGE_UNROLL; ++u)
                        if (u0 + u < UE) p[u] = lds[lds_index(ln, u0 + u)];
#pragma unroll
                    for (int u = 0; u < STAGE_UNROLL; ++u)
                        if (u0 + u < UE) {
                            const int4 v = widen4(p[u]);
                            const v4i_t x = {v.x, v.y, v.z, v.w};
                            __builtin_amdgcn_raw_buffer_store_b128(x, rs, (uint32_t)(ln + (u0 + u) * WAVE) * 16u, 0,
                                                                   OBS_CPOL);
                        }
                }
                return;
            }
            store_flat<NT, false, true, UB, UE>(dst + ln, ln, nc);
            return;
        }
#pragma unroll
        for (int u0 = UB; u0 < UE; u0 += STAGE_UNROLL) {
            uint32_t p[STAGE_UNROLL];
            int cc[STAGE_UNROLL];
#pragma unroll
            for (int u = 0; u < STAGE_UNROLL; ++u) {
                if (u0 + u >= UE) continue;
                const int c0 = ln + (u0 + u) * WAVE;
                const int c = c0 < nc ? c0 : nc - 1;
                const int r = c / CPR;
                cc[u] = c;
                p[u] = lds[r * S + (c - r * CPR)];
            }
#pragma unroll
            for (int u = 0; u < STAGE_UNROLL; ++u)
                if (u0 + u < UE) out16<NT, false>(dst + cc[u], widen4(p[u]));
        }
    }

    // LDS -> R contiguous global rows as int8 letters (the observation_space dtype,
    // ac_env.py:64-70): the tile's LDS image IS the int8 tile, so a 16-byte LDS read is a
    // 16-byte global store; 2L bytes per row, (R * 2L) / 16 stores per wave (4.5 per lane at L = 36)
    template <bool NT>
    __device__ __forceinline__ void store_rows_i8(int8_t* g, int R, int lane) const {
        int ln = lane;
        asm volatile("" : "+v"(ln));
        const int nd = R * CPR;  // dwords of the int8 tile
        uint32_t* dst = reinterpret_cast<uint32_t*>(g);
        // rows are 2L = 8m bytes: a tile starts 16-byte aligned unless m and the row index are
        // both odd (L = 36 with an odd batch), then dword stores (wave-uniform branch)
        const bool al = (reinterpret_cast<uintptr_t>(g) & 15u) == 0;
        if constexpr (S == CPR) {
            if (R == WAVE && al) {
                // full aligned tile (wave-uniform; every step of a full batch): one 16-byte LDS
                // read and one 16-byte store per lane and chunk, no per-dword guards (the general
                // loop below costs ~150 VALU per wave-step at L = 36)
                constexpr int ND = WAVE * CPR;
#pragma unroll
                for (int u = 0; u < (ND + 4 * WAVE - 1) / (4 * WAVE); ++u) {
                    const int d0 = 4 * (ln + u * WAVE);
                    if ((u + 1) * 4 * WAVE > ND && d0 >= ND) continue;  // the last, partial chunk row
                    const v4i_t x = *reinterpret_cast<const v4i_t*>(lds + d0);
                    if constexpr (NT) __builtin_nontemporal_store(x, reinterpret_cast<v4i_t*>(dst + d0));
                    else *reinterpret_cast<v4i_t*>(dst + d0) = x;
                }
                return;
            }
        }
#pragma unroll
        for (int u = 0; u < (WAVE * CPR + 4 * WAVE - 1) / (4 * WAVE); ++u) {
            const int d0 = 4 * (ln + u * WAVE);
            if (d0 >= nd) continue;
            uint32_t v[4];
            if constexpr (S == CPR) {
                // flat image: one 16-byte LDS read per lane, consecutive lanes consecutive
                // 16 bytes (per-dword reads at a 16-byte lane stride were 8-way bank conflicts)
                if (d0 + 4 <= nd) {
                    const uint4 x = *reinterpret_cast<const uint4*>(lds + d0);
                    v[0] = x.x; v[1] = x.y; v[2] = x.z; v[3] = x.w;
                } else {
#pragma unroll
                    for (int j = 0; j < 4; ++j) v[j] = lds[d0 + j < nd ? d0 + j : d0];
                }
            } else {
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const int d = d0 + j < nd ? d0 + j : d0;
                    const int r = d / CPR;
                    v[j] = lds[r * S + (d - r * CPR)];
                }
            }
            if (al && d0 + 4 <= nd) {
                const v4i_t x = {(int)v[0], (int)v[1], (int)v[2], (int)v[3]};
                if constexpr (NT) __builtin_nontemporal_store(x, reinterpret_cast<v4i_t*>(dst + d0));
                else *reinterpret_cast<v4i_t*>(dst + d0) = x;
            } else {
                for (int j = 0; j < 4 && d0 + j < nd; ++j) dst[d0 + j] = v[j];
            }
        }
    }

    // LDS -> global rows with row pitch `gpitch` int32; FB: flagged rows copied from their
    // fallback row (fb_src: `fallback`, or `fallback2` for FB_RESET rows; both pitch fpitch)
    // skip (wave-uniform): rows left unwritten (the learner's finished envs when the curriculum
    // table surely lasts the launch: their copy writes them, step_body)
    template <bool FB, bool NT = false, bool F32 = false>
    __device__ __forceinline__ void store(int32_t* g, int64_t gpitch, int R, const int32_t* fallback,
                                          int64_t fpitch, int lane, const int32_t* fallback2 = nullptr,
                                          uint64_t skip = 0) const {
        int ln = lane;
        asm volatile("" : "+v"(ln));
        const int nc = R * CPR;
        if (gpitch == twoL && !(FB && tile_bad)) {
            // contiguous rows, nothing flagged: chunk c goes to g + 4c (immediate offsets); a
            // full tile (wave-uniform) needs no per-chunk guards
            int4* dst = reinterpret_cast<int4*>(g) + ln;
            if (skip) {  // the row of chunk c is c / CPR: one test against the scalar mask per chunk
#pragma unroll
                for (int u0 = 0; u0 < CPR; u0 += STAGE_UNROLL) {
                    uint32_t p[STAGE_UNROLL];
#pragma unroll
                    for (int u = 0; u < STAGE_UNROLL; ++u)
                        if (u0 + u < CPR && ln + (u0 + u) * WAVE < nc) p[u] = lds[lds_index(ln, u0 + u)];
#pragma unroll
                    for (int u = 0; u < STAGE_UNROLL; ++u) {
                        const int c = ln + (u0 + u) * WAVE;
                        if (u0 + u < CPR && c < nc && !((skip >> (c / CPR)) & 1ull))
                            out16<NT, F32>(dst + (u0 + u) * WAVE, widen4(p[u]));
                    }
                }
            } else if (R == WAVE) {
                store_flat<NT, F32, true>(dst, ln, nc);
            } else {
                store_flat<NT, F32, false>(dst, ln, nc);
            }
            return;
        }
#pragma unroll
        for (int u0 = 0; u0 < CPR; u0 += STAGE_UNROLL) {
            uint32_t p[STAGE_UNROLL];
#pragma unroll
            for (int u = 0; u < STAGE_UNROLL; ++u)
                if (u0 + u < CPR && ln + (u0 + u) * WAVE < nc) p[u] = lds[lds_index(ln, u0 + u)];
#pragma unroll
            for (int u = 0; u < STAGE_UNROLL; ++u) {
                const int c = ln + (u0 + u) * WAVE;
                if (u0 + u < CPR && c < nc && !((skip >> (c / CPR)) & 1ull)) {
                    const int r = c / CPR;
                    const int pos = 4 * (c - r * CPR);
                    int4* dst = reinterpret_cast<int4*>(g + (int64_t)r * gpitch + pos);
                    const uint32_t fc = FB ? flags[r] : 0u;
                    if (fc) out16<false, F32>(dst, *reinterpret_cast<const int4*>(fb_src(fc, fallback, fallback2) + (int64_t)r * fpitch + pos));
                    else out16<NT, F32>(dst, widen4(p[u]));
                }
            }
        }
    }

    // ---- bit-plane registers (acx_planes.h; the env-step kernels) ----
    static constexpr int PW = PlaneWords<NW>::value;

    // lane's row -> bit planes; returns true if the row is outside the domain.  Streams the row
    // 8 letters (two dwords) at a time through one gather per plane (pl::i8x8_to_bytes), so few
    // values are live at once: this pack sets the env-step kernels' register peak
    template <bool LIVE = false>  // LIVE: ignored (see the tile interface, acx_tile.h)
    __device__ __forceinline__ bool pack(int lane, PlaneRegs<PW>& p) const {
        int ln = lane;
        asm volatile("" : "+v"(ln));
        const uint32_t* src = lds + ln * S;
        bool bad = flags[ln] != 0;
#pragma unroll 1
        for (int h = 0; h < 2; ++h) {  // one relator at a time (register peak)
            Planes<PW> w;
            uint64_t nz[PW];
#pragma unroll
            for (int j = 0; j < PW; ++j) w.s[j] = w.y[j] = nz[j] = 0ull;
#pragma unroll
            for (int k = 0; k < HALF; k += 2) {
                const uint32_t d0 = src[h * HALF + k];
                const uint32_t d1 = k + 1 < HALF ? src[h * HALF + k + 1] : 0u;
                uint32_t s8, y8, z8;
                pl::i8x8_to_bytes(d0, d1, s8, y8, z8);
                const int sh = 4 * (k & 15);
                w.s[k >> 4] |= (uint64_t)s8 << sh;
                w.y[k >> 4] |= (uint64_t)y8 << sh;
                nz[k >> 4] |= (uint64_t)z8 << sh;
            }
            int n = 0;
#pragma unroll
            for (int j = 0; j < PW; ++j) n += __builtin_popcountll(nz[j]);
            const pl::Bits<PW> e = pl::bmask<PW>(n);  // zeros only as right padding <=> mask == low n bits
#pragma unroll
            for (int j = 0; j < PW; ++j) bad |= nz[j] != e.b[j];
            if (h == 0) { p.w0 = w; p.n0 = n; }
            else        { p.w1 = w; p.n1 = n; }
        }
        return bad;
    }
    __device__ __forceinline__ void unpack(int lane, const PlaneRegs<PW>& p) const {
        int ln = lane;
        asm volatile("" : "+v"(ln));
        uint32_t* dst = lds + ln * S;
        uint32_t d[CPR];
        image(p, d);
#pragma unroll
        for (int k = 0; k < CPR; k += 2) *reinterpret_cast<uint2*>(dst + k) = make_uint2(d[k], d[k + 1]);
    }
    template <bool LIVE = false>  // LIVE: ignored (see the tile interface, acx_tile.h)
    __device__ __forceinline__ uint32_t unpack_dirty(int lane, const PlaneRegs<PW>& p) const {
        int ln = lane;
        asm volatile("" : "+v"(ln));
        uint32_t* dst = lds + ln * S;
        uint32_t d[CPR];
        image(p, d);
        uint32_t x0 = 0, x1 = 0;
#pragma unroll
        for (int k = 0; k < CPR; k += 2) {
            const uint2 o = *reinterpret_cast<const uint2*>(dst + k);
            if (k < HALF) x0 |= o.x ^ d[k];
            else x1 |= o.x ^ d[k];
            if (k + 1 < HALF) x0 |= o.y ^ d[k + 1];
            else x1 |= o.y ^ d[k + 1];
            *reinterpret_cast<uint2*>(dst + k) = make_uint2(d[k], d[k + 1]);
        }
        return (x0 != 0u ? 1u : 0u) | (x1 != 0u ? 2u : 0u);
    }
    __device__ __forceinline__ void unpack_half(int lane, const PlaneRegs<PW>& p, bool h1) const {
        int ln = lane;
        asm volatile("" : "+v"(ln));
        const Planes<PW> w = pl::psel<PW>(h1, p.w1, p.w0);
        const int n8 = 8 * (h1 ? p.n1 : p.n0);
        uint32_t* dst = lds + ln * S + (h1 ? HALF : 0);
#pragma unroll
        for (int k = 0; k < HALF; ++k) dst[k] = pl::nibbles_to_i8x4(pl::nib<PW>(w.s, k), pl::nib<PW>(w.y, k), clamp_bits(n8 - 32 * k));
    }
    __device__ __forceinline__ static void image(const PlaneRegs<PW>& p, uint32_t (&d)[CPR]) {
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const Planes<PW>& w = h ? p.w1 : p.w0;
            const int n8 = 8 * (h ? p.n1 : p.n0);
#pragma unroll
            for (int k = 0; k < HALF; ++k)
                d[h * HALF + k] = pl::nibbles_to_i8x4(pl::nib<PW>(w.s, k), pl::nib<PW>(w.y, k), clamp_bits(n8 - 32 * k));
        }
    }

    // lane's row -> packed registers; returns true if the row is outside the domain
    __device__ __forceinline__ bool pack(int lane, PresRegs<NW>& p) const {
        int ln = lane;
        asm volatile("" : "+v"(ln));
        const uint32_t* src = lds + ln * S;
        uint32_t d[CPR];
#pragma unroll
        for (int k = 0; k < CPR; k += 2) {
            const uint2 x = *reinterpret_cast<const uint2*>(src + k);
            d[k] = x.x;
            d[k + 1] = x.y;
        }
        bool bad = flags[ln] != 0;
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            Word<NW> w = wzero<NW>();
            uint64_t mlo = 0, mhi = 0;
#pragma unroll
            for (int k = 0; k < HALF; ++k) {
                uint32_t c8, nz4;
                pack4_codes(d[h * HALF + k], c8, nz4);
                w.w[k >> 2] |= c8 << (8 * (k & 3));
                if (k < 16) mlo |= (uint64_t)nz4 << (4 * k);
                else mhi |= (uint64_t)nz4 << (4 * (k - 16));
            }
            const int n = __builtin_popcountll(mlo) + __builtin_popcountll(mhi);
            // zeros only as right padding <=> mask == low n bits
            const uint64_t elo = n >= 64 ? ~0ull : ((1ull << n) - 1ull);
            const uint64_t ehi = n <= 64 ? 0ull : (n >= 128 ? ~0ull : ((1ull << (n - 64)) - 1ull));
            bad |= (mlo != elo) || (mhi != ehi);
            if (h == 0) { p.w0 = w; p.n0 = n; }
            else        { p.w1 = w; p.n1 = n; }
        }
        return bad;
    }

    // packed registers -> lane's row
    __device__ __forceinline__ void unpack(int lane, const PresRegs<NW>& p) const {
        int ln = lane;
        asm volatile("" : "+v"(ln));
        uint32_t* dst = lds + ln * S;
        uint32_t d[CPR];
        image(p, d);
#pragma unroll
        for (int k = 0; k < CPR; k += 2) *reinterpret_cast<uint2*>(dst + k) = make_uint2(d[k], d[k + 1]);
    }

    // unpack, and return which relators differ from the row it overwrites (bit h = relator h):
    // the int8 image is canonical (zero letters past the length), so equal relators compare equal
    __device__ __forceinline__ uint32_t unpack_dirty(int lane, const PresRegs<NW>& p) const {
        int ln = lane;
        asm volatile("" : "+v"(ln));
        uint32_t* dst = lds + ln * S;
        uint32_t d[CPR];
        image(p, d);
        uint32_t x0 = 0, x1 = 0;
#pragma unroll
        for (int k = 0; k < CPR; k += 2) {
            const uint2 o = *reinterpret_cast<const uint2*>(dst + k);
            if (k < HALF) x0 |= o.x ^ d[k];
            else x1 |= o.x ^ d[k];
            if (k + 1 < HALF) x0 |= o.y ^ d[k + 1];
            else x1 |= o.y ^ d[k + 1];
            *reinterpret_cast<uint2*>(dst + k) = make_uint2(d[k], d[k + 1]);
        }
        return (x0 != 0u ? 1u : 0u) | (x1 != 0u ? 2u : 0u);
    }

    // relator h1 of the lane's row only: a clean move changes just its target relator, so the
    // rollout keeps the LDS tile as the int8 image of the current states and re-images one half
    // per step (the trajectory store then reads the whole tile)
    __device__ __forceinline__ void unpack_half(int lane, const PresRegs<NW>& p, bool h1) const {
        int ln = lane;
        asm volatile("" : "+v"(ln));
        const Word<NW> w = wsel<NW>(h1, p.w1, p.w0);
        const int n8 = 8 * (h1 ? p.n1 : p.n0);
        uint32_t* dst = lds + ln * S + (h1 ? HALF : 0);
#pragma unroll
        for (int k = 0; k < HALF; ++k)
            dst[k] = codes_to_i8x4((w.w[k >> 2] >> (8 * (k & 3))) & 0xffu, clamp_bits(n8 - 32 * k));
    }

    __device__ __forceinline__ void set_dirty(int lane, uint32_t m) const { dirty[lane] = (uint8_t)m; }

    // In-place state store (g is the row block the tile was loaded from): only the 16-byte
    // chunks of relators marked in dirty[] are written; every other chunk already holds its
    // value in HBM (a gated move, an unchanged relator, a failed env).  Needs set_dirty for every
    // row of the tile and a wave_sync after it.  Dirty rows flagged FB_RESET (an autoreset to an
    // out-of-domain starting row) are copied from fallback2 (same row pitch).
    // LIVE: a dirty relator's chunks past lim[] (the live chunks of its old and new letters, set
    // by the caller) already hold zero padding in HBM and are not written
    template <bool NT, bool LIVE = false>
    __device__ __forceinline__ void store_dirty(int32_t* g, int R, int lane, const int32_t* fallback2 = nullptr) const {
        int ln = lane;
        asm volatile("" : "+v"(ln));
        const int nc = R * CPR;
        int4* dst = reinterpret_cast<int4*>(g);
        if (tile_bad) {  // rare (wave-uniform): per-chunk fallback test
            for (int c = ln; c < nc; c += WAVE) {
                const int r = c / CPR;
                const int k = c - r * CPR;
                if (!((dirty[r] >> (k >= HALF ? 1 : 0)) & 1u)) continue;
                if (flags[r] == FB_RESET) dst[c] = reinterpret_cast<const int4*>(fallback2)[c];
                else if (!LIVE || live(r, k)) dst[c] = widen4(lds[r * S + k]);
            }
            return;
        }
#pragma unroll
        for (int u0 = 0; u0 < CPR; u0 += STAGE_UNROLL) {
            uint32_t p[STAGE_UNROLL];
            bool wr[STAGE_UNROLL];
#pragma unroll
            for (int u = 0; u < STAGE_UNROLL; ++u) {
                wr[u] = false;
                const int c = ln + (u0 + u) * WAVE;
                if (u0 + u < CPR && c < nc) {
                    const int r = c / CPR;
                    const int k = c - r * CPR;
                    wr[u] = ((dirty[r] >> (k >= HALF ? 1 : 0)) & 1u) && (!LIVE || live(r, k));
                    if (wr[u]) p[u] = lds[r * S + k];
                }
            }
#pragma unroll
            for (int u = 0; u < STAGE_UNROLL; ++u) {
                if (!wr[u]) continue;
                out16<NT, false>(dst + ln + (u0 + u) * WAVE, widen4(p[u]));
            }
        }
    }

  private:
    __device__ __forceinline__ static void image(const PresRegs<NW>& p, uint32_t (&d)[CPR]) {
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const Word<NW>& w = h ? p.w1 : p.w0;
            const int n = h ? p.n1 : p.n0;
            const int n8 = 8 * n;
#pragma unroll
            for (int k = 0; k < HALF; ++k)
                d[h * HALF + k] = codes_to_i8x4((w.w[k >> 2] >> (8 * (k & 3))) & 0xffu, clamp_bits(n8 - 32 * k));
        }
    }
};

}  // namespace acx
