// acx_test_hash.h -- the one test seam of the search engines' key hashes (bfs::khash in
// acx_bfs_common.h, host_hash in acx_greedy.hip, Engine::hash_key in acx_search.cpp): every one
// ends in acx::test_hash::finish(h).
//
// The shipped build leaves ACX_TEST_HASH_CLASSES undefined and finish() is the identity.  A
// build with -DACX_TEST_HASH_CLASSES=K (1 <= K <= 8; build.py's libacx_weakhash.so) keeps only
// h % K, in the top three bits, over 61 low bits that are all ones: every probe starts in the
// last bucket of a masked (h & bmask) or a range-reduced (__umulhi((uint32_t)h, nb)) table and
// wraps at once, every fingerprint taken from below bit 61 is the same, the ones taken from the
// top bits have K values, and every state of a class collides with every other.  The visited
// sets must give the same searches under it: their results may depend on the keys alone.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define ACX_TEST_HASH_HD __host__ __device__
#else
#define ACX_TEST_HASH_HD
#endif

namespace acx {
namespace test_hash {

#ifdef ACX_TEST_HASH_CLASSES
static_assert(ACX_TEST_HASH_CLASSES >= 1 && ACX_TEST_HASH_CLASSES <= 8, "ACX_TEST_HASH_CLASSES: 1..8 (three bits)");
constexpr int CLASSES = ACX_TEST_HASH_CLASSES;
ACX_TEST_HASH_HD inline uint64_t finish(uint64_t h) {
    return ((h % (uint64_t)ACX_TEST_HASH_CLASSES) << 61) | 0x1fffffffffffffffull;
}
#else
constexpr int CLASSES = 0;
ACX_TEST_HASH_HD inline uint64_t finish(uint64_t h) { return h; }
#endif

}  // namespace test_hash
}  // namespace acx
