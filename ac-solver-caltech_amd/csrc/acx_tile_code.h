// acx_tile_code.h -- CodeTile: the LDS tile for a compile-time L >= 64 with L % 8 == 0 (L = 128).
// The interface the three tiles share is stated in acx_tile.h.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "acx_moves.h"
#include "acx_planes.h"
#include "acx_tile_base.h"
#include "acx_tile_io.h"

namespace acx {

// CodeTile: compile-time L % 8 == 0, large L (128).  LDS holds, per 4-letter chunk, one
// 16-bit slot = 8-bit code field | 4-bit non-zero mask << 8 (half the bytes of an int8
// image: 8.5 KB per wave at L = 128, so LDS no longer caps occupancy); the SWAR
// conversion happens in the cooperative load/store, and a lane's pack/unpack is plain
// field assembly.  Row stride S dwords, S = 2 mod 4 (conflict-free 8-byte lane accesses).
// LDS row stride (dwords) of a row of L / 2 16-bit slots: = 2 mod 4
constexpr int code_tile_stride(int L) { return ((L / 4) % 4 == 2) ? L / 4 : L / 4 + ((6 - (L / 4) % 4) % 4); }

template <int NW, int LC>
struct CodeTile : PackedTileBase<LC, code_tile_stride(LC)> {
    static_assert(LC > 0 && LC % 8 == 0, "CodeTile needs a compile-time L multiple of 8");
    using Base = PackedTileBase<LC, code_tile_stride(LC)>;
    using Base::lds;
    using Base::flags;
    using Base::dirty;
    using Base::lim;
    using Base::live;
    using Base::live_chunks;
    static constexpr int L = LC;
    static constexpr int twoL = 2 * LC;
    static constexpr int CPR = LC / 2;   // 4-letter chunks per row (16-bit slots)
    static constexpr int RDW = CPR / 2;  // dwords per row
    static constexpr int S = Base::S;
    static constexpr int HALF = CPR / 2;  // chunks per relator
    static_assert(S % 4 == 2 && RDW % 2 == 0, "row layout");
    static constexpr int LOAD_BATCH = 8;

    uint32_t limv = 0;  // this lane's row's live chunk counts, lim0 | lim1 << 8 (set_lim)
    uint32_t dirtyv = 0;  // this lane's row's dirty bits (set_dirty)
    bool tile_bad = false;  // see tile_restore_flags
    __device__ __forceinline__ void restore_flags(int lane, uint32_t code) { tile_restore_flags(flags, tile_bad, lane, code); }
    __device__ __forceinline__ void flag_rows(int lane, uint32_t code) { tile_flag_rows(flags, tile_bad, lane, code); }

    static constexpr bool PREFETCH_OK = false;  // fetch_rows / put_rows: stubs (see the tile interface, acx_tile.h)
    static constexpr bool LIVE_ROWS = true;  // set_lim selects the chunks a live load reads
    static constexpr int RPI = 1;
    __device__ __forceinline__ int4 fetch_rows(const int32_t*, uint64_t, int) const { return int4{0, 0, 0, 0}; }
    __device__ __forceinline__ void put_rows(const int4&, uint64_t, uint64_t, int) {}
    static constexpr bool NT_STEP_LOADS = true;  // see ld_tile
    __device__ __forceinline__ int32_t letter(int r, int k) const {
        const uint32_t sl = slots(r)[k >> 2];
        const uint32_t d = codes_to_i8x4(sl & 0xffu, 8u * __builtin_popcount((sl >> 8) & 0xfu));
        return (int32_t)(int8_t)(d >> (8 * (k & 3)));
    }
    __device__ __forceinline__ CodeTile(char* base, int) : Base(base) {}
    // see FastTile::set_lim / live (chunks of 4 letters; HALF chunks per relator)
    __device__ __forceinline__ void set_lim(int lane, int n0, int n1) {
        lim[2 * lane] = (uint8_t)live_chunks(n0);
        lim[2 * lane + 1] = (uint8_t)live_chunks(n1);
        limv = (uint32_t)live_chunks(n0) | ((uint32_t)live_chunks(n1) << 8);
    }
    // see FastTile::widen_lim; rounded up to whole 64-byte sectors (4 chunks; relators start on a
    // sector at L % 32 == 0): the chunks past the letters in the last sector hold zero padding in
    // HBM and in the tile, and a partly written sector was a read-modify-write in HBM
    __device__ __forceinline__ void widen_lim(int lane, int n0, int n1) {
        int a = max((int)(limv & 0xffu), live_chunks(n0)), b = max((int)(limv >> 8), live_chunks(n1));
        if constexpr (L % 32 == 0) {
            a = min(HALF, (a + 3) & ~3);
            b = min(HALF, (b + 3) & ~3);
        }
        lim[2 * lane] = (uint8_t)a;
        lim[2 * lane + 1] = (uint8_t)b;
        limv = (uint32_t)a | ((uint32_t)b << 8);
    }
    // CPR == WAVE (one row per wave-instruction): chunk ln of row u is live, row u's counts read
    // from lane u's register (a scalar per compile-time u; no LDS read, no per-u VGPR)
    __device__ __forceinline__ bool live_lane(int u, int ln) const {
        const int lu = __builtin_amdgcn_readlane((int)limv, u);
        const int l0 = lu & 0xff, l1 = (lu >> 8) & 0xff;  // scalars
        return ln < l0 || (ln >= HALF && ln < HALF + l1);  // l0 <= HALF
    }
    __device__ __forceinline__ uint16_t* slots(int r) const { return reinterpret_cast<uint16_t*>(lds + r * S); }

    __device__ __forceinline__ void put(int c, uint32_t slot) const {
        const int r = c / CPR;
        slots(r)[c - r * CPR] = (uint16_t)slot;
    }
    __device__ __forceinline__ uint32_t get(int c) const {
        const int r = c / CPR;
        return slots(r)[c - r * CPR];
    }

    // PIPE (the step kernel; the rollout keeps the plain loop, whose register budget the
    // in-flight batch pair would exceed): full tiles software-pipelined, see below
    template <bool PIPE = false, bool LIVE = false, bool NTL = false, int BATCH = 0>
    __device__ __forceinline__ void load(const int32_t* __restrict__ g, int R, int lane) {
        int ln = lane;
        asm volatile("" : "+v"(ln));
        flags[ln] = 0;
        wave_sync();
        const int nc = R * CPR;
        const int4* src = reinterpret_cast<const int4*>(g) + ln;
        bool any_bad = false;
        if constexpr (CPR == WAVE) {
            if (PIPE && R == WAVE) {
                // full tile, one row per wave-instruction (row u, lane ln = its chunk ln):
                // software-pipelined as below; each chunk is converted by chunk_i8 and stored at
                // the lane's fixed slot address (row u at a compile-time offset).  Rows with a
                // letter outside {-2..2} (error inputs only) are found afterwards, when some
                // chunk was bad: each lane rescans its own row's loaded chunks
                // LIVE: every chunk is loaded through a buffer descriptor over the tile's rows, a
                // dead chunk at an out-of-range offset -- the hardware returns zeros and reads
                // nothing -- so no load sits under a branch (a conditional load made the
                // compiler wait for all of them, vmcnt(0), before each conversion) and a dead
                // chunk converts to an empty slot like any zero padding
                int4 va[LOAD_BATCH], vb[LOAD_BATCH];
                uint16_t* mine = reinterpret_cast<uint16_t*>(lds) + ln;
                const uint64_t gb = reinterpret_cast<uint64_t>(g);
                const uint32_t glo = __builtin_amdgcn_readfirstlane((uint32_t)gb);
                const uint32_t ghi = __builtin_amdgcn_readfirstlane((uint32_t)(gb >> 32));
                const __amdgpu_buffer_rsrc_t rows = __builtin_amdgcn_make_buffer_rsrc(
                    reinterpret_cast<void*>(((uint64_t)ghi << 32) | glo), (short)0, WAVE * CPR * 16, 0x00020000);
                const uint32_t lane_off = (uint32_t)ln * 16u;
                const uint32_t oob = 0x80000000u;
                auto issue = [&](int4* v, int u0) {
#pragma unroll
                    for (int u = 0; u < LOAD_BATCH; ++u) {
                        if constexpr (LIVE) {
                            // row u's live lanes as a 64-bit scalar mask (its counts read from lane
                            // u: one readlane, the rest scalar), then one v_cndmask on it picks the
                            // lane's offset or the out-of-range one; the row's base is the scalar
                            // offset (in range on either reading of the bounds check)
                            const uint32_t lu = (uint32_t)__builtin_amdgcn_readlane((int)limv, u0 + u);
                            const uint32_t l0 = lu & 0xffu, l1 = (lu >> 8) & 0xffu;
                            const uint64_t m = ((1ull << l0) - 1ull) | (((1ull << l1) - 1ull) << 32);
                            uint32_t off;
                            asm("v_cndmask_b32 %0, %1, %2, %3" : "=v"(off) : "v"(oob), "v"(lane_off), "s"(m));
                            const auto x = __builtin_amdgcn_raw_buffer_load_b128(rows, off, (u0 + u) * WAVE * 16, tile_cpol(NTL));
                            v[u] = make_int4((int)x[0], (int)x[1], (int)x[2], (int)x[3]);
                        } else {
                            v[u] = ld_tile<NTL>(src + (u0 + u) * WAVE);
                        }
                    }
                };
                int mx = 0, mn = 0;  // running max / min of every loaded letter (dead chunks load 0)
                auto convert = [&](const int4* v, int u0) {
#pragma unroll
                    for (int u = 0; u < LOAD_BATCH; ++u) {
                        uint32_t c8, nz4;
                        pack4_codes(chunk_i8_acc(v[u], mx, mn), c8, nz4);
                        mine[(u0 + u) * 2 * S] = (uint16_t)(c8 | (nz4 << 8));
                    }
                };
                static_assert(CPR % (2 * LOAD_BATCH) == 0, "pipelined tile load: whole batch pairs");
                issue(va, 0);
#pragma unroll
                for (int u0 = 0; u0 < CPR; u0 += 2 * LOAD_BATCH) {
                    issue(vb, u0 + LOAD_BATCH);
                    convert(va, u0);
                    if (u0 + 2 * LOAD_BATCH < CPR) issue(va, u0 + 2 * LOAD_BATCH);
                    convert(vb, u0 + LOAD_BATCH);
                }
                any_bad = mx > 2 || mn < -2;
                tile_bad = __any(any_bad);
                if (tile_bad) {  // rare (wave-uniform)
                    bool rb = false;
                    const int32_t* row = g + (int64_t)ln * twoL;
                    for (int k = 0; k < CPR; ++k) {
                        bool in = true;
                        if constexpr (LIVE) in = live(ln, k);
                        if (!in) continue;
                        const int4 v = reinterpret_cast<const int4*>(row)[k];
                        bool b = false;
                        chunk_i8(v, b);
                        rb |= b;
                    }
                    flags[ln] = rb ? 1 : 0;
                    // a flagged row's slots are rebuilt with to_i8 (an out-of-domain letter ->
                    // 0x7f, non-zero), so the letter counts reported for it are the input row's
                    if (rb) {
                        for (int k = 0; k < CPR; ++k) {
                            bool in = true;
                            if constexpr (LIVE) in = live(ln, k);
                            if (!in) continue;
                            const int4 v = reinterpret_cast<const int4*>(row)[k];
                            bool b = false;
                            const uint32_t d = to_i8(v.x, b) | (to_i8(v.y, b) << 8) | (to_i8(v.z, b) << 16) |
                                               (to_i8(v.w, b) << 24);
                            uint32_t c8, nz4;
                            pack4_codes(d, c8, nz4);
                            slots(ln)[k] = (uint16_t)(c8 | (nz4 << 8) | ((uint32_t)b << 12));
                        }
                    }
                }
                wave_sync();
                return;
            }
        }
        if (PIPE && R == WAVE) {
            // full tile (wave-uniform): software-pipelined, batch b + 1's loads are issued before
            // batch b is converted, so LOAD_BATCH..2*LOAD_BATCH loads stay in flight through the
            // whole 64 KB tile (L = 128) instead of draining to zero between batches
            // LIVE: a wave-instruction u covers row u (CPR == WAVE), lane ln its chunk ln
            int4 va[LOAD_BATCH], vb[LOAD_BATCH];
            auto lv = [&](int u) {
                if constexpr (!LIVE) return true;
                else if constexpr (CPR == WAVE) return live_lane(u, ln);
                else return live((ln + u * WAVE) / CPR, (ln + u * WAVE) % CPR);
            };
            auto issue = [&](int4* v, int u0) {
#pragma unroll
                for (int u = 0; u < LOAD_BATCH; ++u)
                    if (lv(u0 + u)) v[u] = ld_tile<NTL>(src + (u0 + u) * WAVE);
            };
            auto convert = [&](const int4* v, int u0) {
#pragma unroll
                for (int u = 0; u < LOAD_BATCH; ++u) {
                    const int c = ln + (u0 + u) * WAVE;
                    bool bad = false;
                    uint32_t slot = 0;
                    if (lv(u0 + u)) {
                        const uint32_t d = to_i8(v[u].x, bad) | (to_i8(v[u].y, bad) << 8) |
                                           (to_i8(v[u].z, bad) << 16) | (to_i8(v[u].w, bad) << 24);
                        uint32_t c8, nz4;
                        pack4_codes(d, c8, nz4);
                        slot = c8 | (nz4 << 8) | ((uint32_t)bad << 12);
                    }
                    put(c, slot);
                    if (bad) flags[c / CPR] = 1;
                    any_bad |= bad;
                }
            };
            static_assert(CPR % (2 * LOAD_BATCH) == 0, "pipelined tile load: whole batch pairs");
            issue(va, 0);
#pragma unroll
            for (int u0 = 0; u0 < CPR; u0 += 2 * LOAD_BATCH) {
                issue(vb, u0 + LOAD_BATCH);
                convert(va, u0);
                if (u0 + 2 * LOAD_BATCH < CPR) issue(va, u0 + 2 * LOAD_BATCH);
                convert(vb, u0 + LOAD_BATCH);
            }
            tile_bad = __any(any_bad);
            wave_sync();
            return;
        }
        for (int u0 = 0; u0 < CPR; u0 += LOAD_BATCH) {
            int4 v[LOAD_BATCH];
            bool lv[LOAD_BATCH];
#pragma unroll
            for (int u = 0; u < LOAD_BATCH; ++u) {
                const int c = ln + (u0 + u) * WAVE;
                lv[u] = c < nc && (!LIVE || live(c / CPR, c % CPR));
                if (lv[u]) v[u] = ld_tile<NTL>(src + (u0 + u) * WAVE);
            }
#pragma unroll
            for (int u = 0; u < LOAD_BATCH; ++u) {
                const int c = ln + (u0 + u) * WAVE;
                if (c < nc) {
                    bool bad = false;
                    uint32_t slot = 0;
                    if (lv[u]) {
                        const uint32_t d = to_i8(v[u].x, bad) | (to_i8(v[u].y, bad) << 8) |
                                           (to_i8(v[u].z, bad) << 16) | (to_i8(v[u].w, bad) << 24);
                        uint32_t c8, nz4;
                        pack4_codes(d, c8, nz4);
                        slot = c8 | (nz4 << 8) | ((uint32_t)bad << 12);
                    }
                    put(c, slot);
                    if (bad) flags[c / CPR] = 1;
                    any_bad |= bad;
                }
            }
        }
        tile_bad = __any(any_bad);
        wave_sync();
    }

    // see FastTile::load_block
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
            const uint32_t d = to_i8(v[u].x, bad) | (to_i8(v[u].y, bad) << 8) | (to_i8(v[u].z, bad) << 16) |
                               (to_i8(v[u].w, bad) << 24);
            uint32_t c8, nz4;
            pack4_codes(d, c8, nz4);
            put(c, c8 | (nz4 << 8) | ((uint32_t)bad << 12));
            if (bad) flags[c / CPR] = 1;
        }
        __syncthreads();
    }

    // the rows of the lanes in `rows` only (see FastTile::load_rows); a row is >= one
    // wave-instruction here (CPR >= 16 chunks), so row by row, lanes over its chunks
    __device__ __forceinline__ void load_rows(const int32_t* __restrict__ g, uint64_t rows, int R, int lane) {
        load_rows_from([&](int r) { return g + (int64_t)r * twoL; }, rows, R, lane);
    }
    template <class RowPtr>
    __device__ __forceinline__ void load_rows_from(RowPtr rp, uint64_t rows, int, int lane) {
        if ((rows >> lane) & 1ull) flags[lane] = 0;
        wave_sync();
        bool any_bad = false;
        for (uint64_t m = rows; m; m &= m - 1) {
            const int r = __builtin_ctzll(m);
            const int32_t* row_src = rp(r);
            for (int c = lane; c < CPR; c += WAVE) {
                const int4 v = reinterpret_cast<const int4*>(row_src)[c];
                bool bad = false;
                const uint32_t d = to_i8(v.x, bad) | (to_i8(v.y, bad) << 8) | (to_i8(v.z, bad) << 16) |
                                   (to_i8(v.w, bad) << 24);
                uint32_t c8, nz4;
                pack4_codes(d, c8, nz4);
                slots(r)[c] = (uint16_t)(c8 | (nz4 << 8) | ((uint32_t)bad << 12));
                if (bad) flags[r] = 1;
                any_bad |= bad;
            }
        }
        tile_bad = tile_bad || __any(any_bad);
        wave_sync();
    }

    // LDS -> R contiguous global rows, exactly CPR store instructions on every path (see
    // FastTile::store_rows)
    template <bool NT>
    __device__ __forceinline__ void store_rows(int32_t* g, int R, int lane) const {
        int ln = lane;
        asm volatile("" : "+v"(ln));
        const int nc = R * CPR;
        int4* dst = reinterpret_cast<int4*>(g);
        for (int u0 = 0; u0 < CPR; u0 += STAGE_UNROLL) {
            uint32_t p[STAGE_UNROLL];
            int cc[STAGE_UNROLL];
#pragma unroll
            for (int u = 0; u < STAGE_UNROLL; ++u) {
                const int c0 = ln + (u0 + u) * WAVE;
                cc[u] = c0 < nc ? c0 : nc - 1;
                p[u] = get(cc[u]);
            }
#pragma unroll
            for (int u = 0; u < STAGE_UNROLL; ++u) {
                const uint32_t nz4 = (p[u] >> 8) & 0xfu;
                out16<NT, false>(dst + cc[u], widen4(codes_to_i8x4(p[u] & 0xffu, 8u * __builtin_popcount(nz4))));
            }
        }
    }

    // see FastTile::store_rows_i8: slot c of the tile is int8 dword c of the global tile
    template <bool NT>
    __device__ __forceinline__ void store_rows_i8(int8_t* g, int R, int lane) const {
        int ln = lane;
        asm volatile("" : "+v"(ln));
        const int nc = R * CPR;
        uint32_t* dst = reinterpret_cast<uint32_t*>(g);
#pragma unroll
        for (int u = 0; u < (WAVE * CPR) / (4 * WAVE); ++u) {
            const int c0 = 4 * (ln + u * WAVE);
            if (c0 >= nc) continue;  // nc is a multiple of 4 (CPR % 4 == 0)
            // 4 slots of one row (CPR % 4 == 0): one 8-byte LDS read
            const int r = c0 / CPR;
            const uint2 q = *reinterpret_cast<const uint2*>(slots(r) + (c0 - r * CPR));
            const uint32_t sl[4] = {q.x & 0xffffu, q.x >> 16, q.y & 0xffffu, q.y >> 16};
            int x[4];
#pragma unroll
            for (int j = 0; j < 4; ++j)
                x[j] = (int)codes_to_i8x4(sl[j] & 0xffu, 8u * __builtin_popcount((sl[j] >> 8) & 0xfu));
            const v4i_t v = {x[0], x[1], x[2], x[3]};
            if constexpr (NT) __builtin_nontemporal_store(v, reinterpret_cast<v4i_t*>(dst + c0));
            else *reinterpret_cast<v4i_t*>(dst + c0) = v;
        }
    }

    template <bool FB, bool NT = false, bool F32 = false>
    __device__ __forceinline__ void store(int32_t* g, int64_t gpitch, int R, const int32_t* fallback,
                                          int64_t fpitch, int lane, const int32_t* fallback2 = nullptr,
                                          uint64_t skip = 0) const {  // skip: see FastTile::store
        int ln = lane;
        asm volatile("" : "+v"(ln));
        const int nc = R * CPR;
        for (int u0 = 0; u0 < CPR; u0 += STAGE_UNROLL) {
            uint32_t p[STAGE_UNROLL];
#pragma unroll
            for (int u = 0; u < STAGE_UNROLL; ++u)
                if (ln + (u0 + u) * WAVE < nc) p[u] = get(ln + (u0 + u) * WAVE);
#pragma unroll
            for (int u = 0; u < STAGE_UNROLL; ++u) {
                const int c = ln + (u0 + u) * WAVE;
                if (c >= nc) continue;
                const int r = c / CPR;
                if ((skip >> r) & 1ull) continue;
                const int pos = 4 * (c - r * CPR);
                int4* dst = reinterpret_cast<int4*>(g + (int64_t)r * gpitch + pos);
                if (FB && tile_bad && flags[r]) {
                    out16<false, F32>(dst, *reinterpret_cast<const int4*>(fb_src(flags[r], fallback, fallback2) +
                                                                          (int64_t)r * fpitch + pos));
                } else {
                    const uint32_t nz4 = (p[u] >> 8) & 0xfu;
                    out16<NT, F32>(dst, widen4(codes_to_i8x4(p[u] & 0xffu, 8u * __builtin_popcount(nz4))));
                }
            }
        }
    }

    // ---- bit-plane registers (acx_planes.h; the env-step kernels) ----
    // 4 slots (16 letters) per 8-byte LDS access: their code fields -> 32 bits of 2-bit codes ->
    // the even / odd bits compressed into the s / y planes (and back the same way)
    static constexpr int PW = PlaneWords<NW>::value;
    __device__ __forceinline__ static uint32_t compress_even(uint32_t x) {
        x &= 0x55555555u;
        x = (x | (x >> 1)) & 0x33333333u;
        x = (x | (x >> 2)) & 0x0F0F0F0Fu;
        x = (x | (x >> 4)) & 0x00FF00FFu;
        return (x | (x >> 8)) & 0x0000FFFFu;
    }
    __device__ __forceinline__ static uint32_t spread_even(uint32_t x) {
        x = (x | (x << 8)) & 0x00FF00FFu;
        x = (x | (x << 4)) & 0x0F0F0F0Fu;
        x = (x | (x << 2)) & 0x33333333u;
        return (x | (x << 1)) & 0x55555555u;
    }
    template <bool LIVE = false>  // LIVE: the tile was live-loaded (set_lim), see below
    __device__ __forceinline__ bool pack(int lane, PlaneRegs<PW>& p) const {
        static_assert(HALF % 4 == 0, "16-letter groups per relator");
        int ln = lane;
        asm volatile("" : "+v"(ln));
        const uint32_t* src = lds + ln * S;
        bool bad = flags[ln] != 0;
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            Planes<PW> w;
            uint64_t nz[PW];
#pragma unroll
            for (int j = 0; j < PW; ++j) w.s[j] = w.y[j] = nz[j] = 0ull;
            const int lim_h = (int)((limv >> (8 * h)) & 0xffu);
#pragma unroll
            for (int g = 0; g < HALF / 4; ++g) {  // 16 letters
                // LIVE (the first pack after a live load): a group past every row's live chunks
                // holds zero slots -- skipped when no lane of the wave has one (wave-uniform)
                if (LIVE && !__any(lim_h > 4 * g)) continue;
                const uint2 x = *reinterpret_cast<const uint2*>(src + (h * HALF + 4 * g) / 2);
                const uint32_t codes = __builtin_amdgcn_perm(x.y, x.x, 0x06040200u);
                uint32_t nzb = __builtin_amdgcn_perm(x.y, x.x, 0x07050301u) & 0x0F0F0F0Fu;
                nzb = (nzb | (nzb >> 4)) & 0x00FF00FFu;
                nzb = (nzb | (nzb >> 8)) & 0x0000FFFFu;
                const int sh = 16 * (g & 3);
                w.s[g >> 2] |= (uint64_t)compress_even(codes) << sh;
                w.y[g >> 2] |= (uint64_t)compress_even(codes >> 1) << sh;
                nz[g >> 2] |= (uint64_t)nzb << sh;
            }
            int n = 0;
#pragma unroll
            for (int j = 0; j < PW; ++j) n += __builtin_popcountll(nz[j]);
            const pl::Bits<PW> e = pl::bmask<PW>(n);
#pragma unroll
            for (int j = 0; j < PW; ++j) bad |= nz[j] != e.b[j];
            if (h == 0) { p.w0 = w; p.n0 = n; }
            else        { p.w1 = w; p.n1 = n; }
        }
        return bad;
    }
    // relator h of the lane's row from planes (canonical slots: codes and nz of absent letters 0)
    // glim >= 0: the slots past chunk glim are zero both in the tile and in the new image (a
    // live-loaded relator: max of its old and new live chunks); groups past every lane's glim
    // are neither compared nor written
    __device__ __forceinline__ uint32_t put_relator(uint32_t* dst, const Planes<PW>& w, int n, bool cmp,
                                                    int glim = -1) const {
        const pl::Bits<PW> m = pl::bmask<PW>(n);
        uint32_t x = 0;
#pragma unroll
        for (int g = 0; g < HALF / 4; ++g) {
            if (glim >= 0 && !__any(glim > 4 * g)) continue;
            const int sh = 16 * (g & 3);
            const uint32_t s16 = (uint32_t)(w.s[g >> 2] >> sh) & 0xffffu;
            const uint32_t y16 = (uint32_t)(w.y[g >> 2] >> sh) & 0xffffu;
            const uint32_t codes = spread_even(s16) | (spread_even(y16) << 1);
            uint32_t nzb = (uint32_t)(m.b[g >> 2] >> sh) & 0xffffu;
            nzb = (nzb | (nzb << 8)) & 0x00FF00FFu;
            nzb = (nzb | (nzb << 4)) & 0x0F0F0F0Fu;
            const uint2 v = make_uint2(__builtin_amdgcn_perm(nzb, codes, 0x05010400u),
                                       __builtin_amdgcn_perm(nzb, codes, 0x07030602u));
            uint2* q = reinterpret_cast<uint2*>(dst + 2 * g);
            if (cmp) {
                const uint2 o = *q;
                x |= (o.x ^ v.x) | (o.y ^ v.y);
            }
            *q = v;
        }
        return x;
    }
    __device__ __forceinline__ void unpack(int lane, const PlaneRegs<PW>& p) const {
        int ln = lane;
        asm volatile("" : "+v"(ln));
        uint32_t* dst = lds + ln * S;
        put_relator(dst, p.w0, p.n0, false);
        put_relator(dst + HALF / 2, p.w1, p.n1, false);
    }
    template <bool LIVE = false>  // LIVE: the tile was live-loaded (set_lim), see below
    __device__ __forceinline__ uint32_t unpack_dirty(int lane, const PlaneRegs<PW>& p) const {
        int ln = lane;
        asm volatile("" : "+v"(ln));
        uint32_t* dst = lds + ln * S;
        int g0 = -1, g1 = -1;
        if constexpr (LIVE) {
            g0 = max((int)(limv & 0xffu), live_chunks(p.n0));
            g1 = max((int)((limv >> 8) & 0xffu), live_chunks(p.n1));
        }
        const uint32_t x0 = put_relator(dst, p.w0, p.n0, true, g0);
        const uint32_t x1 = put_relator(dst + HALF / 2, p.w1, p.n1, true, g1);
        return (x0 != 0u ? 1u : 0u) | (x1 != 0u ? 2u : 0u);
    }
    __device__ __forceinline__ void unpack_half(int lane, const PlaneRegs<PW>& p, bool h1) const {
        int ln = lane;
        asm volatile("" : "+v"(ln));
        put_relator(lds + ln * S + (h1 ? HALF / 2 : 0), pl::psel<PW>(h1, p.w1, p.w0), h1 ? p.n1 : p.n0, false);
    }

    __device__ __forceinline__ bool pack(int lane, PresRegs<NW>& p) const {
        int ln = lane;
        asm volatile("" : "+v"(ln));
        const uint32_t* src = lds + ln * S;
        bool bad = flags[ln] != 0;
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            Word<NW> w = wzero<NW>();
            uint64_t mlo = 0, mhi = 0;
#pragma unroll
            for (int k = 0; k < HALF; k += 4) {  // 4 slots = one 8-byte LDS read
                const uint2 x = *reinterpret_cast<const uint2*>(src + (h * HALF + k) / 2);
                const uint32_t sl[4] = {x.x & 0xffffu, x.x >> 16, x.y & 0xffffu, x.y >> 16};
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const int kk = k + j;
                    w.w[kk >> 2] |= (sl[j] & 0xffu) << (8 * (kk & 3));
                    const uint64_t nz4 = (sl[j] >> 8) & 0xfu;
                    if (kk < 16) mlo |= nz4 << (4 * kk);
                    else mhi |= nz4 << (4 * (kk - 16));
                }
            }
            const int n = __builtin_popcountll(mlo) + __builtin_popcountll(mhi);
            const uint64_t elo = n >= 64 ? ~0ull : ((1ull << n) - 1ull);
            const uint64_t ehi = n <= 64 ? 0ull : (n >= 128 ? ~0ull : ((1ull << (n - 64)) - 1ull));
            bad |= (mlo != elo) || (mhi != ehi);
            if (h == 0) { p.w0 = w; p.n0 = n; }
            else        { p.w1 = w; p.n1 = n; }
        }
        return bad;
    }

    __device__ __forceinline__ void unpack(int lane, const PresRegs<NW>& p) const { unpack_impl<false>(lane, p); }
    // see FastTile::unpack_half
    __device__ __forceinline__ void unpack_half(int lane, const PresRegs<NW>& p, bool h1) const {
        int ln = lane;
        asm volatile("" : "+v"(ln));
        const Word<NW> w = wsel<NW>(h1, p.w1, p.w0);
        const int n = h1 ? p.n1 : p.n0;
        uint32_t* dst = lds + ln * S + (h1 ? HALF / 2 : 0);
#pragma unroll
        for (int k = 0; k < HALF; k += 4) {
            uint32_t sl[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int kk = k + j;
                const int nin = n - 4 * kk;
                const uint32_t nz4 = nin >= 4 ? 0xfu : (nin <= 0 ? 0u : ((1u << nin) - 1u));
                sl[j] = ((w.w[kk >> 2] >> (8 * (kk & 3))) & 0xffu) | (nz4 << 8);
            }
            *reinterpret_cast<uint2*>(dst + k / 2) = make_uint2(sl[0] | (sl[1] << 16), sl[2] | (sl[3] << 16));
        }
    }
    // see FastTile::unpack_dirty; the slots compared are canonical (codes of absent letters
    // masked to 0, as load writes them)
    __device__ __forceinline__ uint32_t unpack_dirty(int lane, const PresRegs<NW>& p) const {
        return unpack_impl<true>(lane, p);
    }
    __device__ __forceinline__ void set_dirty(int lane, uint32_t m) {
        dirty[lane] = (uint8_t)m;
        dirtyv = m;
    }

    // see FastTile::store_dirty
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
                if (flags[r] == FB_RESET) {
                    dst[c] = reinterpret_cast<const int4*>(fallback2)[c];
                } else if (!LIVE || live(r, k)) {
                    const uint32_t sl = slots(r)[k];
                    dst[c] = widen4(codes_to_i8x4(sl & 0xffu, 8u * __builtin_popcount((sl >> 8) & 0xfu)));
                }
            }
            return;
        }
        if constexpr (CPR == WAVE) {
            // one row per wave-instruction (row r, lane ln = its chunk ln): the lane's fixed slot
            // address, row r's dirty bits and live counts read from lane r's registers (scalars)
            const uint16_t* mine = reinterpret_cast<const uint16_t*>(lds) + ln;
            const int hs = ln >= HALF ? 1 : 0;
            const uint64_t gb = reinterpret_cast<uint64_t>(g);
            const uint32_t glo = __builtin_amdgcn_readfirstlane((uint32_t)gb);
            const uint32_t ghi = __builtin_amdgcn_readfirstlane((uint32_t)(gb >> 32));
            const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(
                reinterpret_cast<void*>(((uint64_t)ghi << 32) | glo), (short)0, WAVE * CPR * 16, 0x00020000);
            for (int r0 = 0; r0 < R; r0 += STAGE_UNROLL) {
                uint32_t p[STAGE_UNROLL];
                bool wr[STAGE_UNROLL];
#pragma unroll
                for (int u = 0; u < STAGE_UNROLL; ++u) {
                    const int r = r0 + u;
                    const uint32_t dr = (uint32_t)__builtin_amdgcn_readlane((int)dirtyv, r);
                    bool lv = true;
                    if constexpr (LIVE) lv = live_lane(r, ln);
                    wr[u] = r < R && ((dr >> hs) & 1u) && lv;
                    if (wr[u]) p[u] = mine[r * 2 * S];
                }
#pragma unroll
                for (int u = 0; u < STAGE_UNROLL; ++u) {
                    if (!wr[u]) continue;
                    const uint32_t nz4 = (p[u] >> 8) & 0xfu;
                    const int4 v = widen4(codes_to_i8x4(p[u] & 0xffu, 8u * __builtin_popcount(nz4)));
                    const v4i_t x = {v.x, v.y, v.z, v.w};
                    __builtin_amdgcn_raw_buffer_store_b128(x, rs, (uint32_t)(ln + (r0 + u) * WAVE) * 16u, 0, WB_CPOL);
                }
            }
            return;
        }
        for (int u0 = 0; u0 < CPR; u0 += STAGE_UNROLL) {
            uint32_t p[STAGE_UNROLL];
            bool wr[STAGE_UNROLL];
#pragma unroll
            for (int u = 0; u < STAGE_UNROLL; ++u) {
                wr[u] = false;
                const int c = ln + (u0 + u) * WAVE;
                if (c < nc) {
                    const int r = c / CPR;
                    const int k = c - r * CPR;
                    bool lv = true;
                    if constexpr (LIVE) lv = (CPR == WAVE) ? live_lane(u0 + u, ln) : live(r, k);
                    wr[u] = ((dirty[r] >> (k >= HALF ? 1 : 0)) & 1u) && lv;
                    if (wr[u]) p[u] = slots(r)[k];
                }
            }
#pragma unroll
            for (int u = 0; u < STAGE_UNROLL; ++u) {
                if (!wr[u]) continue;
                const uint32_t nz4 = (p[u] >> 8) & 0xfu;
                out16<NT, false>(dst + ln + (u0 + u) * WAVE,
                                 widen4(codes_to_i8x4(p[u] & 0xffu, 8u * __builtin_popcount(nz4))));
            }
        }
    }

  private:
    template <bool CMP>
    __device__ __forceinline__ uint32_t unpack_impl(int lane, const PresRegs<NW>& p) const {
        int ln = lane;
        asm volatile("" : "+v"(ln));
        uint32_t* dst = lds + ln * S;
        uint32_t x[2] = {0u, 0u};
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const Word<NW>& w = h ? p.w1 : p.w0;
            const int n = h ? p.n1 : p.n0;
#pragma unroll
            for (int k = 0; k < HALF; k += 4) {
                uint32_t sl[4];
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const int kk = k + j;
                    const int nin = n - 4 * kk;
                    const uint32_t nz4 = nin >= 4 ? 0xfu : (nin <= 0 ? 0u : ((1u << nin) - 1u));
                    uint32_t c8 = (w.w[kk >> 2] >> (8 * (kk & 3))) & 0xffu;
                    if constexpr (CMP) c8 &= nin >= 4 ? 0xffu : (nin <= 0 ? 0u : ((1u << (2 * nin)) - 1u));
                    sl[j] = c8 | (nz4 << 8);
                }
                uint2* q = reinterpret_cast<uint2*>(dst + (h * HALF + k) / 2);
                const uint2 v = make_uint2(sl[0] | (sl[1] << 16), sl[2] | (sl[3] << 16));
                if constexpr (CMP) {
                    const uint2 o = *q;
                    x[h] |= (o.x ^ v.x) | (o.y ^ v.y);
                }
                *q = v;
            }
        }
        return (x[0] != 0u ? 1u : 0u) | (x[1] != 0u ? 2u : 0u);
    }
};

}  // namespace acx
