// acx_key.h -- the packed-key format of acx_expand12 (acx.h), stated once: the 2-bit letter codes
// of r0 (from bit 0) and r1 (from bit 2L), then the letter counts n0 (8 bits at bit 4L) and n1
// (at bit 4L + 8), in acx_key_words(L) uint64 words.  A child whose move failed carries 0xFF in
// both count bytes.  Plain inline functions for the host compiler and for hipcc (host and device).
#pragma once
#include <stdint.h>

#ifdef __HIPCC__
#define ACX_HD __host__ __device__
#else
#define ACX_HD
#endif

namespace acx {

// letter <-> code: x = 0, x^-1 = 1, y = 2, y^-1 = 3 (letters 1, -1, 2, -2)
ACX_HD inline int32_t key_letter(uint32_t code) { return ((code & 2u) ? 2 : 1) * ((code & 1u) ? -1 : 1); }
ACX_HD inline uint64_t key_code(int32_t letter) { return letter == 1 ? 0 : letter == -1 ? 1 : letter == 2 ? 2 : 3; }

// the 8 bits from bit position `bit` on (they may straddle two words)
ACX_HD inline uint32_t key_byte(const uint64_t* k, int bit) {
    const int w = bit >> 6, o = bit & 63;
    uint64_t v = k[w] >> o;
    if (o > 56) v |= k[w + 1] << (64 - o);
    return (uint32_t)(v & 0xffu);
}
// the code of letter i of relator h
ACX_HD inline uint32_t key_code_at(const uint64_t* k, int L, int h, int i) {
    const int bit = 2 * (h * L + i);
    return (uint32_t)(k[bit >> 6] >> (bit & 63)) & 3u;
}

ACX_HD inline int key_len(const uint64_t* k, int L, int h) { return (int)key_byte(k, 4 * L + 8 * h); }
ACX_HD inline int key_total(const uint64_t* k, int L) { return key_len(k, L, 0) + key_len(k, L, 1); }
ACX_HD inline bool key_is_error(const uint64_t* k, int L) {
    return key_len(k, L, 0) == 0xff && key_len(k, L, 1) == 0xff;
}
ACX_HD inline void key_first_letters(const uint64_t* k, int L, int32_t out[2]) {
    for (int h = 0; h < 2; ++h) out[h] = key_letter(key_code_at(k, L, h, 0));
}

// host packing of a presentation (2L letters, zero-padded relators) into a key
inline void pack_key(const int32_t* pres, int L, int kw, uint64_t* out) {
    for (int k = 0; k < kw; ++k) out[k] = 0;
    int n[2] = {0, 0};
    for (int h = 0; h < 2; ++h) {
        for (int i = 0; i < L; ++i) {
            const int32_t v = pres[h * L + i];
            if (v == 0) continue;
            const int bit = 2 * (h * L + i);
            out[bit / 64] |= key_code(v) << (bit % 64);
            ++n[h];
        }
    }
    const uint64_t lens = (uint64_t)n[0] | ((uint64_t)n[1] << 8);
    const int bit = 4 * L;
    out[bit / 64] |= lens << (bit % 64);
    if (bit % 64 > 48 && bit / 64 + 1 < kw) out[bit / 64 + 1] |= lens >> (64 - bit % 64);
}

}  // namespace acx
