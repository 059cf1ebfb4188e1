// CPU check of the batched greedy search's frontier order (ac-solver-caltech_amd/csrc/acx_prio.h,
// the header csrc/acx_mgreedy.hip compares heap entries with) against the host engines' priority
// key (prio_key in acx_frontier.h, both of its paths) and against the definition: Python's order on
// (total, path length, tuple(state)) of greedy.py:55-64,104-113.  Stand-alone: no libacx, no GPU
// (tests/test_greedy_many_cpu.py builds and runs it).
//   prio_check [seed]  ->  "ok ..." and exit 0, or "FAIL ..." lines and exit 1
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

#include "acx_frontier.h"
#include "acx_key.h"
#include "acx_prio.h"

using namespace acx;

static int fails = 0;
static long checked = 0;
#define CHECK(cond, ...)                         \
    do {                                         \
        if (!(cond)) {                           \
            if (++fails <= 20) {                 \
                std::printf("FAIL %s: ", #cond); \
                std::printf(__VA_ARGS__);        \
                std::printf("\n");               \
            }                                    \
        }                                        \
    } while (0)

static std::mt19937_64 rng;
static int rnd(int lo, int hi) { return lo + (int)(rng() % ((uint64_t)(hi - lo) + 1)); }
static int key_words(int L) { return (4 * L + 16 + 63) / 64; }  // acx_key_words (acx.h)
static const int32_t LET[4] = {1, -1, 2, -2};

struct Node {
    std::vector<int32_t> p;  // 2L letters, zero-padded relators
    int tot, dep;
};

static Node random_node(int L, int n0, int n1) {
    Node x{std::vector<int32_t>(2 * L, 0), 0, rnd(0, 5)};
    for (int i = 0; i < n0; ++i) x.p[i] = LET[rng() & 3];
    for (int i = 0; i < n1; ++i) x.p[L + i] = LET[rng() & 3];
    x.tot = n0 + n1;
    return x;
}

static int sgn(int v) { return v < 0 ? -1 : v > 0 ? 1 : 0; }

// the definition: tuple order of (total, path length, letters as integers)
static int def_cmp(const Node& a, const Node& b, bool states_only) {
    if (!states_only) {
        if (a.tot != b.tot) return sgn(a.tot - b.tot);
        if (a.dep != b.dep) return sgn(a.dep - b.dep);
    }
    for (size_t i = 0; i < a.p.size(); ++i)
        if (a.p[i] != b.p[i]) return sgn(a.p[i] - b.p[i]);
    return 0;
}

// one pair through every form of the order
static void check_pair(int L, const Node& a, const Node& b, const char* what) {
    const int kw = key_words(L), pk = prio_words(L);
    std::vector<uint64_t> ka(kw), kb(kw);
    pack_key(a.p.data(), L, kw, ka.data());
    pack_key(b.p.data(), L, kw, kb.data());
    const int want = def_cmp(a, b, false);
    const int got = prio_less(ka.data(), a.tot, a.dep, kb.data(), b.tot, b.dep, L)   ? -1
                    : prio_less(kb.data(), b.tot, b.dep, ka.data(), a.tot, a.dep, L) ? 1
                                                                                     : 0;
    CHECK(got == want, "L %d %s: prio_less order %d, definition %d", L, what, got, want);
    const int st = prio_cmp_states(ka.data(), kb.data(), L);
    CHECK(st == def_cmp(a, b, true), "L %d %s: prio_cmp_states %d, definition %d", L, what, st, def_cmp(a, b, true));
    CHECK(prio_cmp_states(kb.data(), ka.data(), L) == -st, "L %d %s: prio_cmp_states is not antisymmetric", L, what);
    for (int generic = 0; generic < 2; ++generic) {
        std::vector<uint64_t> pa(pk), pb(pk);
        prio_key(ka.data(), L, kw, pk, a.tot, a.dep, pa.data(), generic != 0);
        prio_key(kb.data(), L, kw, pk, b.tot, b.dep, pb.data(), generic != 0);
        const int words = pa < pb ? -1 : pb < pa ? 1 : 0;  // vector order = unsigned word order
        CHECK(words == got, "L %d %s: prio_key (generic %d) word order %d, acx_prio.h %d", L, what, generic, words,
              got);
        CHECK(prio_k0(ka.data(), L, a.tot, a.dep) == pa[0], "L %d %s: prio_k0 is not prio_key's first word", L, what);
        CHECK(prio_k0(kb.data(), L, b.tot, b.dep) == pb[0], "L %d %s: prio_k0 is not prio_key's first word", L, what);
    }
    // k0 is monotone in the order: it never contradicts the full comparison
    const uint64_t k0a = prio_k0(ka.data(), L, a.tot, a.dep), k0b = prio_k0(kb.data(), L, b.tot, b.dep);
    if (k0a != k0b) CHECK((k0a < k0b ? -1 : 1) == want, "L %d %s: k0 order against the definition", L, what);
    ++checked;
}

// letter `to` at global position pos (r0 then r1) of a copy of x; total and depth kept
static Node with_letter(const Node& x, int pos, int32_t to) {
    Node y = x;
    y.p[pos] = to;
    return y;
}

static void planted(int L) {
    // full relators: every position holds a letter
    const Node full = random_node(L, L, L);
    // only the last letter of r1 differs
    for (int32_t u : LET)
        for (int32_t v : LET)
            if (u != v)
                check_pair(L, with_letter(full, 2 * L - 1, u), with_letter(full, 2 * L - 1, v), "last letter of r1");
    // only the letter on one side of a 64-bit word boundary of the packed key differs (32 letters per word)
    for (int pos = 32; pos < 2 * L; pos += 32)
        for (int side = -1; side <= 0; ++side)
            for (int32_t u : LET)
                for (int32_t v : LET)
                    if (u != v)
                        check_pair(L, with_letter(full, pos + side, u), with_letter(full, pos + side, v),
                                   "word boundary");
    // the same with an earlier difference absent and a later one present: the first difference decides
    for (int pos = 32; pos < 2 * L; pos += 32)
        for (int side = -1; side <= 0; ++side) {
            Node a = with_letter(full, pos + side, 1), b = with_letter(full, pos + side, -2);
            if (pos + side + 1 < 2 * L) {
                a.p[pos + side + 1] = -2;
                b.p[pos + side + 1] = 2;
            }
            check_pair(L, a, b, "word boundary, later difference");
        }
    // a padding position against each of the four letters, in either relator, at every length m
    // (total and depth held equal, so the letters decide)
    for (int h = 0; h < 2; ++h)
        for (int m = 1; m < L; ++m) {
            if (L > 20 && m > 3 && m < L - 3 && m % 16 > 1 && m % 16 < 15) continue;  // ends and word boundaries
            Node a = random_node(L, h ? L : m, h ? m : L);
            a.dep = 3;
            for (int32_t u : LET) {
                Node b = with_letter(a, h * L + m, u);
                b.tot = a.tot;
                check_pair(L, a, b, "padding against a letter");
                check_pair(L, b, a, "a letter against padding");
                // the longer relator goes on: what follows must not matter
                if (m + 1 < L) {
                    Node c = with_letter(b, h * L + m + 1, -u);
                    check_pair(L, a, c, "padding against a longer relator");
                }
            }
        }
    // equal letters, different depth; equal depth, different total
    {
        Node a = random_node(L, rnd(1, L), rnd(1, L)), b = a;
        b.dep = a.dep + 1;
        check_pair(L, a, b, "depth");
        check_pair(L, b, a, "depth");
        Node c = random_node(L, rnd(1, L), rnd(1, L));
        c.dep = a.dep;
        c.tot = a.tot + 1;  // (the total is the caller's: it outranks whatever the letters say)
        check_pair(L, a, c, "total");
        check_pair(L, c, a, "total");
        check_pair(L, a, a, "equal");
    }
}

static void random_pairs(int L) {
    for (int it = 0; it < 3000; ++it) {
        const Node a = random_node(L, rnd(1, L), rnd(1, L));
        Node b = random_node(L, rnd(1, L), rnd(1, L));
        switch (it % 4) {
            case 0: break;  // unrelated
            case 1:         // a copy with one letter changed: a long common prefix
                b = a;
                {
                    std::vector<int> live;
                    for (int i = 0; i < 2 * L; ++i)
                        if (a.p[i]) live.push_back(i);
                    b.p[live[rng() % live.size()]] = LET[rng() & 3];
                }
                break;
            case 2: {  // a copy with one relator cut short (total and depth as given)
                b = a;
                const int h = (int)(rng() & 1);
                int n = 0;
                while (n < L && a.p[h * L + n]) ++n;
                for (int i = rnd(1, n); i < n; ++i) b.p[h * L + i] = 0;
                break;
            }
            default:  // same total and depth, other letters
                b.tot = a.tot;
                b.dep = a.dep;
                break;
        }
        check_pair(L, a, b, "random");
    }
}

int main(int argc, char** argv) {
    rng.seed(argc > 1 ? std::strtoull(argv[1], nullptr, 10) : 1);
    for (int L : {1, 16, 17, 32, 33, 40, 41, 64, 65, 127, 128}) {
        planted(L);
        random_pairs(L);
    }
    if (fails) {
        std::printf("FAIL %d checks\n", fails);
        return 1;
    }
    std::printf("ok %ld pairs\n", checked);
    return 0;
}
