// CPU check of the solution cache's key algebra (ac-solver-caltech_amd/csrc/acx_cache.h, the part
// that the host compiler and hipcc both compile: rotating one relator inside a packed key, and the
// enumeration of a state's variants in the reference's order) against a per-letter restatement of
// value_search/value_guided_search.py:124-151.  Stand-alone: no libacx, no GPU
// (tests/test_cache_cpu.py builds and runs it, once more under -fsanitize=address,undefined).
//   cache_key_check [seed]   ->  "ok ..." and exit 0, or "FAIL ..." lines and exit 1
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

#include "acx_cache.h"
#include "acx_key.h"

using namespace acx;
using namespace acx::cache;

static int fails = 0;
static long checked = 0;
#define CHECK(cond, ...)                         \
    do {                                         \
        ++checked;                               \
        if (!(cond)) {                           \
            if (++fails <= 20) {                 \
                std::printf("FAIL %s: ", #cond); \
                std::printf(__VA_ARGS__);        \
                std::printf("\n");               \
            }                                    \
        }                                        \
    } while (0)

static int key_words(int L) { return (4 * L + 16 + 63) / 64; }

// a presentation as the reference holds it: 2L letters, zero-padded relators
using Pres = std::vector<int32_t>;

// the key in a buffer of exactly kw words (so that the sanitizers see a read past the key)
static std::vector<uint64_t> packed(const Pres& p, int L) {
    std::vector<uint64_t> k(key_words(L));
    pack_key(p.data(), L, key_words(L), k.data());
    return k;
}

// the reference's rotation by slicing: nz[k:] + nz[:k] in relator h (:145-146)
static Pres rotated_ref(const Pres& p, int L, int h, int n, int k) {
    Pres r = p;
    for (int i = 0; i < n; ++i) r[h * L + i] = p[h * L + (i + k) % n];
    return r;
}

static std::vector<uint64_t> rotated_key(const std::vector<uint64_t>& key, int L, int h, int n, int k) {
    std::vector<uint64_t> out(key.size());
    for (int w = 0; w < (int)key.size(); ++w) out[w] = key_rot_word(key.data(), L, h, n, k, w);
    return out;
}

static int32_t letter(std::mt19937_64& rng) {
    static const int32_t all[4] = {1, -1, 2, -2};
    return all[rng() & 3];
}

// every k of relator h at lengths (n0, n1); `cancel`: make relator h's ends cancel
static void one(std::mt19937_64& rng, int L, int n0, int n1, bool cancel0, bool cancel1) {
    Pres p(2 * L, 0);
    const int n[2] = {n0, n1};
    const bool cancel[2] = {cancel0, cancel1};
    for (int h = 0; h < 2; ++h) {
        for (int i = 0; i < n[h]; ++i) p[h * L + i] = letter(rng);
        if (n[h] > 1) {
            int32_t& last = p[h * L + n[h] - 1];
            if (cancel[h]) last = -p[h * L];
            else if (last == -p[h * L]) last = p[h * L];
        }
    }
    const std::vector<uint64_t> key = packed(p, L);
    // the variants, in the reference's order: the state, relator 0's rotations, relator 1's
    int c[2];
    const int total = variant_counts(key.data(), L, c);
    for (int h = 0; h < 2; ++h) {
        const int want = (n[h] <= 1 || cancel[h]) ? 0 : n[h] - 1;
        CHECK(c[h] == want && rot_count(key.data(), L, h) == want, "L %d h %d n %d cancel %d: %d", L, h, n[h],
              (int)cancel[h], c[h]);
    }
    CHECK(total == 1 + c[0] + c[1], "total");
    int v = 0, rel, k;
    variant_at(c[0], v++, rel, k);
    CHECK(rel == 0 && k == 0, "variant 0");
    for (int h = 0; h < 2; ++h) {
        for (int kk = 1; kk <= c[h]; ++kk) {
            variant_at(c[0], v++, rel, k);
            CHECK(rel == h && k == kk, "L %d variant %d: (%d, %d) for (%d, %d)", L, v - 1, rel, k, h, kk);
        }
    }
    CHECK(v == total, "count");
    // every rotation, the skipped relators' too: the function itself has no skip
    for (int h = 0; h < 2; ++h) {
        for (int kk = 0; kk < n[h]; ++kk) {
            const std::vector<uint64_t> got = rotated_key(key, L, h, n[h], kk);
            const std::vector<uint64_t> want = packed(rotated_ref(p, L, h, n[h], kk), L);
            CHECK(got == want, "L %d h %d n0 %d n1 %d k %d", L, h, n0, n1, kk);
        }
    }
}

int main(int argc, char** argv) {
    std::mt19937_64 rng(argc > 1 ? std::strtoull(argv[1], nullptr, 10) : 1);
    const int Ls[] = {7, 16, 18, 32, 33, 128};
    for (int L : Ls) {
        for (int n = 1; n <= L; ++n) {
            // relator 0 at every length beside a short, a full and a random relator 1, and the
            // other way round; the skip cases n <= 1 (n = 1 here) and cancelling ends
            const int others[3] = {1, L, 1 + (int)(rng() % L)};
            for (int o : others) {
                one(rng, L, n, o, false, false);
                one(rng, L, o, n, false, false);
                one(rng, L, n, o, true, false);
                one(rng, L, o, n, false, true);
            }
        }
        one(rng, L, L, L, true, true);
    }
    // the meta word round-trips its fields
    const uint64_t m = meta_pack(0xfedcba98ull, (1ull << META_STEP_BITS) - 1, 1, 127);
    CHECK((m >> 32) == 0xfedcba98ull && ((m >> 9) & ((1ull << META_STEP_BITS) - 1)) == (1ull << META_STEP_BITS) - 1 &&
              ((m >> 8) & 1) == 1 && (m & 0xff) == 127,
          "meta");
    if (fails) return 1;
    std::printf("ok %ld checks\n", checked);
    return 0;
}
