// acx_step_pair.h -- the plain step of small batches at L <= 64: two lanes per env (step_pair_kernel).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <type_traits>
#include "acx.h"
#include "acx_kernel_common.h"
#include "acx_moves.h"
#include "acx_planes.h"
#include "acx_step_args.h"
#include "acx_tile.h"

namespace acx {

// ---------------------------------------------------------------------------------
// Small batches: two lanes per env (BASELINE configs[1]: 65,536 envs at L = 36).
//
// With one lane per env, 65,536 envs are 1,024 waves -- one per SIMD: nothing hides a wave's
// load -> pack -> move -> unpack -> store chain, and a lone wave issues a VALU instruction every
// 4 cycles instead of every 2 (MI355X_MICROARCH.md, "vector-instruction ISSUE cost").
// step_pair_kernel gives each env two lanes of a 32-env tile, lane 2e + h holding relator h of
// env e, so the same batch is 2,048 waves and the per-relator work is split between the lanes:
//   * the tile (32 rows, 18 16-byte chunks each) is read with 9 coalesced loads per lane into an
//     int8 image in LDS; relator q of the tile (q = 2e + h) is chunks [9q, 9q + 9) -- lane q's;
//   * lane q packs ITS relator into bit planes (pl::, one 64-bit word per plane at L <= 64) and
//     takes its partner's planes and length with four DPP quad-permutes (quad_perm [1,0,3,2]);
//   * the move is split over the pair (pl::pair_move_clean: the target lane moves its relator,
//     the junction cancellation count and the cyclic peel are the first set bit of a mismatch
//     mask, the splice is shifts of the planes); an unreduced env runs the general move on both;
//   * lane q decides on the planes whether its relator changed; in the common case (in place, full
//     tile, no out-of-domain reset) it writes that relator's 9 chunks straight from its planes.
//     Otherwise the moved relators are re-imaged into the tile and the "changed" bits, the rows'
//     fallback codes and the error flags -- wave ballots, one bit per relator, bit q <-> chunks
//     [9q, 9q + 9) -- steer a coalesced write-back that tests chunk c against bit c / 9.
// Results are those of step_body<..., LEARN = false, LIVE = false> (the same pack, move,
// image and error contract; tests/test_gpu_*: every acx_step test at L = 36 and B <= 131,072 runs
// here); only the instruction schedule differs.  launch_step takes it for B <= SMALL_STEP_MAX_B.
// ---------------------------------------------------------------------------------
constexpr int64_t SMALL_STEP_MAX_B = (int64_t)2 * 4 * 256 * WAVE;  // <= 4 pair-waves per SIMD on 256 CUs
template <int NW, int LC, int VEC>
constexpr bool small_step_ok() {
    return std::is_same<TileFor<NW, LC, VEC>, FastTile<NW, LC>>::value && LC <= 64;
}

// partner lane's value (lane ^ 1): DPP quad_perm [1,0,3,2], full-rate VALU, no LDS
__device__ __forceinline__ uint32_t pair_xchg(uint32_t v) {
    return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0xB1, 0xF, 0xF, false);
}
__device__ __forceinline__ uint64_t pair_xchg64(uint64_t v) {
    return (uint64_t)pair_xchg((uint32_t)v) | ((uint64_t)pair_xchg((uint32_t)(v >> 32)) << 32);
}

template <int LC>
struct PairLayout {
    static constexpr int CPR = LC / 2;          // 16-byte chunks per row
    static constexpr int HALF = CPR / 2;        // chunks (= image dwords) per relator
    static constexpr int ENVS = WAVE / 2;       // envs per wave
    static constexpr int NCH = ENVS * CPR;      // chunks per full tile
    static constexpr int U = NCH / WAVE;        // chunk loads per lane (full tile)
    static_assert(LC % 4 == 0 && LC <= 64 && HALF * 2 == CPR && U * WAVE == NCH, "pair tile layout");
    static constexpr size_t wave_bytes = (size_t)NCH * 4 + WAVE;  // int8 image + one flag byte per relator
};

// relator image (HALF dwords of int8 letters, zero padding) -> its planes and length; true if
// outside the domain (a zero inside the relator): FastTile::pack on one relator
template <int HALF>
__device__ __forceinline__ bool pair_pack(const uint32_t* src, Planes<1>& w, int& n) {
    uint64_t s = 0, y = 0, nz = 0;
#pragma unroll
    for (int k = 0; k < HALF; k += 2) {
        const uint32_t d0 = src[k];
        const uint32_t d1 = k + 1 < HALF ? src[k + 1] : 0u;
        uint32_t s8, y8, z8;
        pl::i8x8_to_bytes(d0, d1, s8, y8, z8);
        s |= (uint64_t)s8 << (4 * k);
        y |= (uint64_t)y8 << (4 * k);
        nz |= (uint64_t)z8 << (4 * k);
    }
    w.s[0] = s;
    w.y[0] = y;
    n = __builtin_popcountll(nz);
    return nz != pl::bmask<1>(n).b[0];  // zeros only as right padding <=> mask == low n bits
}

// planes -> the relator's int8 image in dst; returns true if it differs from what dst held
template <int HALF>
__device__ __forceinline__ bool pair_image(uint32_t* dst, const Planes<1>& w, int n) {
    uint32_t x = 0;
#pragma unroll
    for (int k = 0; k < HALF; ++k) {
        const uint32_t d = pl::nibbles_to_i8x4(pl::nib<1>(w.s, k), pl::nib<1>(w.y, k), clamp_bits(8 * n - 32 * k));
        x |= dst[k] ^ d;
        dst[k] = d;
    }
    return x != 0u;
}

// a relator's int32 letters (HALF chunks from src) -> its int8 image in dst; true if a letter is
// outside {-2..2} (the image then holds 0x7f there, as FastTile::load_rows)
template <int HALF>
__device__ __forceinline__ bool pair_load_relator(uint32_t* dst, const int32_t* src) {
    int4 v[HALF];
#pragma unroll
    for (int k = 0; k < HALF; ++k) v[k] = reinterpret_cast<const int4*>(src)[k];
    bool bad = false;
#pragma unroll
    for (int k = 0; k < HALF; ++k)
        dst[k] = to_i8(v[k].x, bad) | (to_i8(v[k].y, bad) << 8) | (to_i8(v[k].z, bad) << 16) | (to_i8(v[k].w, bad) << 24);
    return bad;
}

template <int NW, int LC, int VEC>
__global__ __launch_bounds__(BLOCK, 4) void step_pair_kernel(StepArgs a) {
    using PT = PairLayout<LC>;
    constexpr int L = LC, twoL = 2 * LC, CPR = PT::CPR, HALF = PT::HALF, ENVS = PT::ENVS;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int lane = threadIdx.x & (WAVE - 1);
    const int wid = __builtin_amdgcn_readfirstlane((int)(threadIdx.x / WAVE));
    const int64_t r0 = ((int64_t)blockIdx.x * WPB + wid) * ENVS;  // wave-uniform
    if (r0 >= a.B) return;
    const int R = (int)((a.B - r0) < ENVS ? (a.B - r0) : ENVS);
    const int er = lane >> 1, h = lane & 1;  // env (tile row) and relator of this lane
    const bool active = er < R;
    const int64_t env = r0 + er;
    uint32_t* img = reinterpret_cast<uint32_t*>(smem + wid * PT::wave_bytes);
    uint8_t* rflag = reinterpret_cast<uint8_t*>(img + PT::NCH);  // per relator: a bad chunk at load (rare path)
    uint32_t* mine = img + lane * HALF;                          // this lane's relator image

    // scalars first: their latency hides under the tile's loads (both lanes of an env read the
    // same words; the second is a cache hit)
    int act = 0, cnt0 = 0;
    bool pend = false;
    if (active) {
        act = a.action[env];
        cnt0 = a.step_count ? a.step_count[env] : 0;
        pend = a.pending && a.pending[env] != 0;  // next-step autoreset: reset now
    }
    // the tile: chunk c = lane + 64u of the tile's rows (coalesced), relator c / HALF
    bool flagged = false;  // this lane's relator has a chunk with a letter outside {-2..2}
    {
        const int4* src = reinterpret_cast<const int4*>(a.state_in + r0 * twoL) + lane;
        uint32_t badm = 0;  // bit u: chunk lane + 64u
        if (R == ENVS) {  // full tile (wave-uniform): every load in flight at once
            int4 v[PT::U];
#pragma unroll
            for (int u = 0; u < PT::U; ++u) v[u] = src[u * WAVE];
#pragma unroll
            for (int u = 0; u < PT::U; ++u) {
                bool bad;
                img[lane + u * WAVE] = chunk_i8(v[u], bad);
                badm |= (uint32_t)bad << u;
            }
        } else {
            const int nc = R * CPR;
#pragma unroll
            for (int u = 0; u < PT::U; ++u) {
                const int c = lane + u * WAVE;
                if (c < nc) {
                    bool bad;
                    img[c] = chunk_i8(src[u * WAVE], bad);
                    badm |= (uint32_t)bad << u;
                }
            }
        }
        if (__any(badm != 0u)) {
            // rare (wave-uniform): the flagged relators are found through LDS, and chunk_i8's
            // arbitrary bytes in them re-imaged letter by letter (an out-of-domain letter ->
            // 0x7f), so the letter counts the contract reports for the row (reward, lengths) are
            // those of the input row
            rflag[lane] = 0;
            wave_sync();
#pragma unroll
            for (int u = 0; u < PT::U; ++u)
                if ((badm >> u) & 1u) rflag[(lane + u * WAVE) / HALF] = 1;
            wave_sync();
            flagged = rflag[lane] != 0;
            if (active && flagged) pair_load_relator<HALF>(mine, a.state_in + env * twoL + h * L);
        }
        wave_sync();
    }

    // this lane's relator -> planes and its reversal; the partner's by DPP
    const bool cyc = a.cyclical != 0;
    Planes<1> w;
    int n;
    bool bad = pair_pack<HALF>(mine, w, n) || flagged;
    const Planes<1> w_in = w;  // the relator as loaded: "changed" is decided on the planes
    const int n_in = n;
    const Planes<1> rw = pl::prev<1>(w, n);
    bool clean = pl::relator_clean<1>(w, n, cyc);
    Planes<1> pw, prw;
    int pn;
    {
        pw.s[0] = pair_xchg64(w.s[0]);
        pw.y[0] = pair_xchg64(w.y[0]);
        prw.s[0] = pair_xchg64(rw.s[0]);
        prw.y[0] = pair_xchg64(rw.y[0]);
        const uint32_t x = pair_xchg((uint32_t)n | (bad ? 0x100u : 0u) | (clean ? 0x200u : 0u));
        pn = (int)(x & 0xffu);
        bad = bad || (x & 0x100u) != 0u;
        clean = clean && (x & 0x200u) != 0u;
    }

    // the env's move: on a clean env (both relators reduced) each lane runs its relator's part of
    // it (pl::pair_move_clean: the target lane moves, its partner keeps its relator); otherwise
    // (an unreduced start: rare) both lanes run the general move on the whole env
    int e = ACX_ERR_NONE;
    bool general = false;
    if (active) {
        if (pend) e = ACX_ERR_NONE;  // no move: the env resets (gymnasium >= 1.0 NEXT_STEP autoreset)
        else if (bad) e = ACX_ERR_DOMAIN;
        else if (clean) e = pl::pair_move_clean(w, n, rw, pw, pn, prw, h, act, L, cyc);
        else general = true;
    }
    if (general) {
        PlaneRegs<1> q;
        q.w0 = h ? pw : w;
        q.w1 = h ? w : pw;
        q.n0 = h ? pn : n;
        q.n1 = h ? n : pn;
        const pl::MoveOut<1> mo = pl::ac_move_call<1>(q, act, L, cyc);
        e = mo.e;
        w = h ? mo.p.w1 : mo.p.w0;
        n = h ? mo.p.n1 : mo.p.n0;
    }
    // the env's code is its target lane's (ac_moves.py:167-179: relator (id + 1) & 1; every other
    // outcome is the same on both lanes); the partner's new length and letter-0 y bit
    bool xy = false;  // the relators' first letters: one x^{+-1} and one y^{+-1}
    {
        const uint32_t x = pair_xchg((uint32_t)e | ((uint32_t)n << 8) | ((uint32_t)(w.y[0] & 1u) << 16));
        if (h != ((act + 1) & 1)) e = (int)(x & 0xffu);
        pn = (int)((x >> 8) & 0xffu);
        xy = ((x >> 16) & 1u) != (uint32_t)(w.y[0] & 1u);
    }
    const int n0 = h ? pn : n, n1 = h ? n : pn;
    int cnt = 0;
    bool keep = false, triv = false, trunc = false, fin = false, reset = false;
    int32_t rwd = 0;
    if (active) {
        cnt = a.step_count ? cnt0 + 1 : 0;
        keep = e != ACX_ERR_NONE;
        if (keep) cnt = cnt0;  // the reference raises before count_steps += 1 (ac_env.py:93-102)
        // strict triviality (pl::is_trivial): both relators one letter, one x and one y
        triv = !pend && !keep && n0 == 1 && n1 == 1 && xy;
        trunc = !pend && !keep && a.step_count && cnt >= a.horizon;
        rwd = pend ? 0 : triv ? a.horizon * L * 2 : -(n0 + n1);
        fin = triv || trunc;
        reset = a.pending ? pend : (fin && a.reset_state && !keep);
    }
    // this lane's relator changed (a failed env keeps its row): compared on the planes (canonical:
    // no bits past the letters), so the common store below needs no re-imaged tile
    bool chg = false;
    if (active && !keep) {
        const uint64_t m = pl::bmask<1>(n).b[0];
        chg = n != n_in || (((w.s[0] ^ w_in.s[0]) | (w.y[0] ^ w_in.y[0])) & m) != 0ull;
    }
    // same-step autoreset (or a pending env's reset): the lane loads its relator of the starting
    // row into the image (FastTile::load_rows' result; an out-of-domain starting row is taken as it
    // is and stored from reset_state, FB_RESET)
    bool rbad = false;
    int rn = n;
    if (active && reset) {
        if (a.final_obs) {  // final_obs <- the post-move state (rare): each lane its relator
            int32_t* fo = a.final_obs + env * twoL + h * L;
#pragma unroll 1
            for (int k = 0; k < L; ++k) {
                const uint32_t code = pl::pletter<1>(w, k);
                fo[k] = k < n ? (int32_t)(int8_t)((0xFE02FF01u >> (code << 3)) & 0xffu) : 0;
            }
        }
        rbad = pair_load_relator<HALF>(mine, a.reset_state + env * twoL + h * L);
        Planes<1> rw2;
        rbad = pair_pack<HALF>(mine, rw2, rn) || rbad;
        chg = true;  // dm = 3: the whole row is written
    }
    // the partner's starting-row length and domain flag (every lane takes part in the DPP)
    int ln0 = n0, ln1 = n1;  // lengths_out
    {
        const uint32_t x = pair_xchg((uint32_t)rn | (rbad ? 0x100u : 0u));
        if (reset) {
            rbad = rbad || (x & 0x100u) != 0u;
            ln0 = h ? (int)(x & 0xffu) : rn;
            ln1 = h ? rn : (int)(x & 0xffu);
        }
    }
    if (rbad) e = ACX_ERR_DOMAIN;  // lengths_out: the non-zero counts of the starting row
    if (reset) cnt = 0;
    // per-env outputs: lane 0 of the pair the env's scalars, lane 1 the lengths
    if (active) {
        if (h == 0) {
            if (a.reward) a.reward[env] = rwd;
            if (a.done) a.done[env] = (uint8_t)triv;
            if (a.truncated) a.truncated[env] = (uint8_t)trunc;
            if (a.pending) a.pending[env] = fin ? 1 : 0;
            if (a.step_count) a.step_count[env] = cnt;
            if (a.err) a.err[env] = (uint8_t)e;
            if (e != ACX_ERR_NONE && a.err_count) atomicAdd(a.err_count, 1);
        } else if (a.lengths_out) {
            a.lengths_out[2 * env] = ln0;
            a.lengths_out[2 * env + 1] = ln1;
        }
    }

    // the state store.  Relator masks, bit q = relator q of the tile (chunks [9q, 9q + 9)):
    //   fb_in    rows stored from their input row (out of domain, not reset: FB_IN)
    //   fb_rst   rows stored from their starting row (reset to an out-of-domain row: FB_RESET)
    //   dirty    relators that differ from state_in (in place: the only chunks written)
    const uint64_t fb_rst = __ballot(active && reset && rbad);
    const uint64_t fb_in = __ballot(active && !reset && e == ACX_ERR_DOMAIN);
    const uint64_t dirty = __ballot(active && chg);
    if (a.in_place && fb_rst == 0ull && R == ENVS) {
        // the common case (wave-uniform): each lane writes its own changed relator, 9 contiguous
        // 16-byte chunks, straight from its planes (or, reset, from the starting row it loaded
        // into its image) -- no re-imaged tile, no tile-wide LDS pass
        if (dirty == 0ull) return;
        if (chg) {
            int4* d = reinterpret_cast<int4*>(a.state_out + env * twoL + h * L);
            if (reset) {
#pragma unroll
                for (int k = 0; k < HALF; ++k) out16<NT_WRITEBACK, false>(d + k, widen4(mine[k]));
            } else {
#pragma unroll
                for (int k = 0; k < HALF; ++k)
                    out16<NT_WRITEBACK, false>(
                        d + k, widen4(pl::nibbles_to_i8x4(pl::nib<1>(w.s, k), pl::nib<1>(w.y, k), clamp_bits(8 * n - 32 * k))));
            }
        }
        return;
    }
    // otherwise the tile's image (moved relators re-imaged) and the coalesced stores below
    if (active && !keep && !reset) pair_image<HALF>(mine, w, n);
    wave_sync();
    const int nc = R * CPR;
    int4* dst = reinterpret_cast<int4*>(a.state_out + r0 * twoL);
    const int4* fin_row = reinterpret_cast<const int4*>(a.state_in + r0 * twoL);
    const int4* frs_row = reinterpret_cast<const int4*>(a.reset_state ? a.reset_state + r0 * twoL : a.state_in);
    if (a.in_place) {
        if (dirty == 0ull) return;
        // dirty and fb_in never share a relator (a failed env is not dirty)
        if (fb_rst == 0ull && R == ENVS) {
            // the common case (wave-uniform): every image dword read first (one LDS wait, not one
            // per chunk), then the dirty chunks stored
            uint32_t v[PT::U];
#pragma unroll
            for (int u = 0; u < PT::U; ++u) v[u] = img[lane + u * WAVE];
#pragma unroll
            for (int u = 0; u < PT::U; ++u) {
                const int c = lane + u * WAVE;
                if ((dirty >> (c / HALF)) & 1ull) out16<NT_WRITEBACK, false>(dst + c, widen4(v[u]));
            }
            return;
        }
#pragma unroll
        for (int u = 0; u < PT::U; ++u) {
            const int c = lane + u * WAVE;
            if (c >= nc) continue;
            const int q = c / HALF;
            if (!((dirty >> q) & 1ull)) continue;
            if ((fb_rst >> q) & 1ull) dst[c] = frs_row[c];
            else out16<NT_WRITEBACK, false>(dst + c, widen4(img[c]));
        }
    } else {
#pragma unroll
        for (int u = 0; u < PT::U; ++u) {
            const int c = lane + u * WAVE;
            if (c >= nc) continue;
            const int q = c / HALF;
            if ((fb_rst >> q) & 1ull) dst[c] = frs_row[c];
            else if ((fb_in >> q) & 1ull) dst[c] = fin_row[c];
            else dst[c] = widen4(img[c]);
        }
    }
}

}  // namespace acx
