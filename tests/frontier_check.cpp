// CPU check of the search engines' shared host code (ac-solver-caltech_amd/csrc/acx_key.h and
// acx_frontier.h): the packed-key fields, greedy's priority key (fast path = generic path = the
// definition), the BucketHeap's pop order, the two-generation in-flight table and the per-child
// replay of a popped node (greedy.py:76-119).  Stand-alone:
// no libacx, no GPU (tests/test_frontier_host.py builds and runs it).  Reference behaviour: the
// heap tuple (total, path length, state tuple) of greedy.py:55-64,104-113 and the key layout of
// include/acx.h.
//   frontier_check [seed]  ->  "ok ..." and exit 0, or "FAIL ..." lines and exit 1
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <set>
#include <utility>
#include <vector>

#include "acx_frontier.h"
#include "acx_key.h"

using namespace acx;

static int fails = 0;
#define CHECK(cond, ...)                      \
    do {                                      \
        if (!(cond)) {                        \
            if (++fails <= 20) {              \
                std::printf("FAIL %s: ", #cond); \
                std::printf(__VA_ARGS__);     \
                std::printf("\n");            \
            }                                 \
        }                                     \
    } while (0)

static std::mt19937_64 rng;
static int rnd(int lo, int hi) { return lo + (int)(rng() % ((uint64_t)(hi - lo) + 1)); }
static int key_words(int L) { return (4 * L + 16 + 63) / 64; }  // acx_key_words (acx.h)

// a presentation with relators of n0 and n1 random letters, zero-padded to L each
static std::vector<int32_t> random_pres(int L, int n0, int n1) {
    static const int32_t let[4] = {1, -1, 2, -2};
    std::vector<int32_t> p(2 * L, 0);
    for (int i = 0; i < n0; ++i) p[i] = let[rng() & 3];
    for (int i = 0; i < n1; ++i) p[L + i] = let[rng() & 3];
    return p;
}

// the harness's own writer of a length byte (8 single bits at bit 4L + 8h)
static void set_len_byte(uint64_t* k, int L, int h, uint32_t v) {
    for (int j = 0; j < 8; ++j) {
        const int bit = 4 * L + 8 * h + j;
        k[bit >> 6] = (k[bit >> 6] & ~(1ull << (bit & 63))) | ((uint64_t)((v >> j) & 1u) << (bit & 63));
    }
}

static void check_key_fields() {
    for (int L : {1, 12, 13, 14, 15, 16, 36, 128}) {
        const int kw = key_words(L);
        for (int it = 0; it < 300; ++it) {
            // the extreme lengths first, then random ones
            const int n0 = it == 0 ? 0 : it == 1 ? L : rnd(0, L), n1 = it == 0 ? L : it == 1 ? 0 : rnd(0, L);
            const std::vector<int32_t> p = random_pres(L, n0, n1);
            std::vector<uint64_t> k(kw + 1, 0xdeadbeefdeadbeefull);  // pack_key must write all kw words
            pack_key(p.data(), L, kw, k.data());
            CHECK(k[kw] == 0xdeadbeefdeadbeefull, "L %d: pack_key wrote past kw", L);
            CHECK(key_len(k.data(), L, 0) == n0 && key_len(k.data(), L, 1) == n1, "L %d n %d %d: got %d %d", L, n0, n1,
                  key_len(k.data(), L, 0), key_len(k.data(), L, 1));
            CHECK(key_total(k.data(), L) == n0 + n1, "L %d: total %d != %d", L, key_total(k.data(), L), n0 + n1);
            CHECK(!key_is_error(k.data(), L), "L %d n %d %d: a good key reads as an error", L, n0, n1);
            int32_t first[2];
            key_first_letters(k.data(), L, first);
            if (n0 > 0) CHECK(first[0] == p[0], "L %d: first letter of r0 %d != %d", L, first[0], p[0]);
            if (n1 > 0) CHECK(first[1] == p[L], "L %d: first letter of r1 %d != %d", L, first[1], p[L]);
            for (int h = 0; h < 2; ++h)
                for (int i = 0; i < (h ? n1 : n0); ++i)
                    CHECK(key_letter(key_code_at(k.data(), L, h, i)) == p[h * L + i], "L %d: letter %d of r%d", L, i, h);
            // one length byte 0xFF is not the sentinel; both are
            for (int h = 0; h < 2; ++h) {
                std::vector<uint64_t> one(k);
                set_len_byte(one.data(), L, h, 0xffu);
                CHECK(!key_is_error(one.data(), L), "L %d: only byte %d is 0xFF, read as an error", L, h);
                CHECK(key_len(one.data(), L, h) == 0xff && key_len(one.data(), L, 1 - h) == (h ? n0 : n1),
                      "L %d: length bytes after writing byte %d", L, h);
            }
            set_len_byte(k.data(), L, 0, 0xffu);
            set_len_byte(k.data(), L, 1, 0xffu);
            CHECK(key_is_error(k.data(), L), "L %d: the sentinel is not seen", L);
        }
    }
}

// the definition: the integer total (9 bits) | depth (31) | letter + 2 (3 bits each, r0 then r1
// with padding), written MSB first into pk words, one bit at a time
static std::vector<uint64_t> prio_definition(const std::vector<int32_t>& p, int L, int tot, int dep) {
    const int pk = (40 + 6 * L + 63) / 64;
    std::vector<uint64_t> out(pk, 0);
    int pos = 0;
    auto put = [&](uint64_t v, int nbits) {
        for (int b = nbits - 1; b >= 0; --b, ++pos)
            if ((v >> b) & 1u) out[pos >> 6] |= 1ull << (63 - (pos & 63));
    };
    put((uint64_t)tot, 9);
    put((uint64_t)dep, 31);
    for (int i = 0; i < 2 * L; ++i) put((uint64_t)(p[i] + 2), 3);
    return out;
}

static void check_prio_key() {
    const int deps[] = {0, 1, 12345, 0x7fffffff};
    for (int L : {1, 4, 5, 20, 21, 40, 41, 128}) {
        const int kw = key_words(L), pk = prio_words(L);
        CHECK(pk == (40 + 6 * L + 63) / 64, "L %d: prio_words", L);
        for (int it = 0; it < 200; ++it) {
            const int n0 = it == 0 ? L : it == 1 ? 0 : rnd(0, L), n1 = it == 0 ? L : it == 1 ? L : rnd(0, L);
            const std::vector<int32_t> p = random_pres(L, n0, n1);
            std::vector<uint64_t> k(kw);
            pack_key(p.data(), L, kw, k.data());
            // the real total (up to 2L = 256) and the field's ends
            const int tots[] = {n0 + n1, 0, 255, 256};
            for (int tot : tots)
                for (int dep : {deps[it & 3], rnd(0, 0x7fffffff)}) {
                    // one spare word each: the key must not be written past pk words
                    std::vector<uint64_t> fast(pk + 1, 0xa5a5a5a5a5a5a5a5ull), gen(pk + 1, 0xa5a5a5a5a5a5a5a5ull);
                    prio_key(k.data(), L, kw, pk, tot, dep, fast.data(), false);
                    prio_key(k.data(), L, kw, pk, tot, dep, gen.data(), true);
                    CHECK(fast[pk] == 0xa5a5a5a5a5a5a5a5ull && gen[pk] == 0xa5a5a5a5a5a5a5a5ull, "L %d: written past pk", L);
                    fast.resize(pk);
                    gen.resize(pk);
                    const std::vector<uint64_t> def = prio_definition(p, L, tot, dep);
                    CHECK(fast == gen, "L %d n %d %d tot %d dep %d: fast path != generic path", L, n0, n1, tot, dep);
                    CHECK(gen == def, "L %d n %d %d tot %d dep %d: generic path != definition", L, n0, n1, tot, dep);
                }
        }
    }
}

// N nodes at L; at L = 12 most share total, depth and r0's first 8 letters (the entry's first
// word: 40 header bits + 24 letter bits), so the later words in pkeys decide
static void check_heap(int L, int N) {
    const int kw = key_words(L), pk = prio_words(L);
    std::vector<int32_t> base = random_pres(L, L, L);
    std::vector<uint64_t> pkeys;
    std::vector<std::vector<uint64_t>> key_of_id;
    auto new_node = [&]() -> int64_t {
        std::vector<int32_t> p;
        int dep;
        if (L >= 12 && rnd(0, 9) < 8) {  // the tied family: full relators, letters 0..7 of r0 fixed
            p = random_pres(L, L, L);
            std::copy(base.begin(), base.begin() + 8, p.begin());
            dep = 3;
        } else {
            p = random_pres(L, rnd(0, L), rnd(0, L));
            dep = rnd(0, 5);
        }
        int tot = 0;
        for (int32_t v : p) tot += v != 0;
        std::vector<uint64_t> k(kw);
        pack_key(p.data(), L, kw, k.data());
        const int64_t id = (int64_t)key_of_id.size();
        pkeys.resize(pkeys.size() + pk);
        prio_key(k.data(), L, kw, pk, tot, dep, &pkeys[(size_t)id * pk]);
        key_of_id.emplace_back(pkeys.begin() + id * pk, pkeys.begin() + (id + 1) * pk);
        return id;
    };
    // push all, pop all: the keys sorted as unsigned word strings
    BucketHeap heap;
    heap.init(pk, &pkeys);
    for (int i = 0; i < N; ++i) {
        const int64_t id = new_node();
        heap.push(pkeys[(size_t)id * pk], id);
    }
    CHECK(heap.size() == (size_t)N, "L %d: size %zu", L, heap.size());
    std::vector<std::vector<uint64_t>> sorted(key_of_id);
    std::sort(sorted.begin(), sorted.end());
    size_t ties = 0;
    for (int i = 1; i < N; ++i) ties += sorted[i][0] == sorted[i - 1][0] && sorted[i] != sorted[i - 1];
    if (pk > 1) CHECK(ties > (size_t)N / 2, "L %d: only %zu keys tie on the first word", L, ties);
    for (int i = 0; i < N; ++i) {
        CHECK(!heap.empty(), "L %d: empty after %d pops", L, i);
        if (heap.empty()) return;
        CHECK(key_of_id[(size_t)heap.top()] == sorted[i], "L %d: pop %d out of order", L, i);
        heap.pop();
    }
    CHECK(heap.empty() && heap.size() == 0, "L %d: not empty after all pops", L);
    // pushes and pops interleaved, against an ordered multiset of (key, id)
    std::multiset<std::vector<uint64_t>> ref;
    for (int round = 0; round < 200; ++round) {
        for (int i = rnd(0, 30); i > 0; --i) {
            const int64_t id = new_node();
            heap.push(pkeys[(size_t)id * pk], id);
            ref.insert(key_of_id[(size_t)id]);
        }
        for (int i = rnd(0, 25); i > 0 && !ref.empty(); --i) {
            CHECK(key_of_id[(size_t)heap.top()] == *ref.begin(), "L %d: interleaved pop out of order (round %d)", L, round);
            heap.pop();
            ref.erase(ref.begin());
        }
        CHECK(heap.size() == ref.size() && heap.empty() == ref.empty(), "L %d: size %zu != %zu", L, heap.size(), ref.size());
    }
}

struct StoredKey {
    const std::vector<uint64_t>* v = nullptr;
    const uint64_t* operator()(int64_t id) const { return &(*v)[(size_t)id]; }
};

// age = 4: ids 0..3, 4..7, ... are the generations; after id n is inserted the live ones are the
// current generation and the one before it.  same_chain: every key with one hash (same slot
// chain, same tag), so only the key compare and the id limits tell them apart.
static void check_recent(bool same_chain) {
    const int64_t age = 4;
    std::vector<uint64_t> store, hash;
    store.reserve(20);
    Recent<StoredKey> recent(age, 1, StoredKey{&store});
    for (int64_t n = 0; n < 20; ++n) {
        store.push_back(1000 + (uint64_t)n);  // distinct keys
        hash.push_back(same_chain ? 0x1234000000000005ull : rng());
        recent.insert(n, hash[(size_t)n]);
        const int64_t cur_lo = n / age * age, older_lo = cur_lo >= age ? cur_lo - age : 0;
        CHECK(recent.gen_lo[recent.cur] == cur_lo, "after id %lld: gen_lo %lld", (long long)n,
              (long long)recent.gen_lo[recent.cur]);
        for (int64_t i = 0; i <= n; ++i)
            for (int64_t from = 0; from <= n + 1; ++from) {
                const int64_t want = i >= from && i >= older_lo ? i : -1;
                const int64_t got = recent.find(&store[(size_t)i], hash[(size_t)i], from);
                CHECK(got == want, "after id %lld: find(key of %lld, from %lld) = %lld, want %lld", (long long)n,
                      (long long)i, (long long)from, (long long)got, (long long)want);
                CHECK(got < 0 || got >= older_lo, "after id %lld: id %lld of a retired generation", (long long)n,
                      (long long)got);
            }
        const uint64_t absent = 999;
        CHECK(recent.find(&absent, hash[(size_t)n], 0) == -1, "after id %lld: a key never inserted was found", (long long)n);
    }
}

// replay_children on 12 hand-made children at L = 4: totals 6 5 5 7 | 4 ... ; child 2 repeats
// child 1 (seen), `special` is the success (total 2) or the move error, or -1 for neither
static void check_replay(int special, bool error, int64_t max_nodes) {
    const int L = 4, kw = key_words(L);
    const int n0s[ACT] = {3, 3, 3, 4, 2, 3, 3, 3, 3, 3, 3, 3}, n1s[ACT] = {3, 2, 2, 3, 2, 3, 3, 3, 3, 3, 3, 3};
    std::vector<uint64_t> ck((size_t)ACT * kw), hs(ACT);
    std::set<std::vector<uint64_t>> nodes;
    for (int a = 0; a < ACT; ++a) {
        std::vector<int32_t> p;
        do {
            p = a == special && !error ? random_pres(L, 1, 1) : random_pres(L, n0s[a], n1s[a]);
            pack_key(p.data(), L, kw, &ck[(size_t)a * kw]);
        } while (a != 2 && !nodes.insert({ck.begin() + a * kw, ck.begin() + (a + 1) * kw}).second);
        if (a == 2) std::copy(ck.begin() + kw, ck.begin() + 2 * kw, ck.begin() + 2 * kw);
        for (int h = 0; h < 2 && a == special && error; ++h) set_len_byte(&ck[(size_t)a * kw], L, h, 0xffu);
        hs[a] = 100 + (uint64_t)a;
    }
    Outcome o;
    o.min_length = 6;
    std::vector<int> added, asked;
    std::set<std::vector<uint64_t>> have;
    const int64_t n_nodes = 50, n_open = 20;
    const bool ended = replay_children(
        ck.data(), hs.data(), L, kw, o, 7, n_nodes, n_open, max_nodes,
        [&](const uint64_t* k, uint64_t h, int a) {
            CHECK(h == hs[a] && k == &ck[(size_t)a * kw], "seen: child %d", a);
            asked.push_back(a);
            return have.count({k, k + kw}) != 0;
        },
        [&](const uint64_t* k, uint64_t h, int a, int len) {
            CHECK(h == hs[a] && len == key_total(k, L), "add: child %d", a);
            added.push_back(a);
            have.insert({k, k + kw});
        });
    const int stop = special < 0 ? ACT : special;  // children before `stop` go through seen / add
    std::vector<int> want_asked, want_added, want_trace;
    for (int a = 0; a < stop; ++a) {
        want_asked.push_back(a);
        if (a != 2) want_added.push_back(a);
    }
    if (stop > 1) want_trace.push_back(5);
    if (stop > 4) want_trace.push_back(4);
    if (special >= 0 && !error) want_trace.push_back(2);
    CHECK(asked == want_asked && added == want_added, "special %d: %zu asked, %zu added", special, asked.size(), added.size());
    CHECK(o.trace == std::vector<int32_t>(want_trace.begin(), want_trace.end()), "special %d: trace", special);
    CHECK(o.min_length == (want_trace.empty() ? 6 : want_trace.back()), "special %d: min_length %d", special, o.min_length);
    CHECK(o.last_popped == 7 && o.popped == std::vector<int64_t>{7}, "special %d: popped", special);
    const int last = special >= 0 && error ? special - 1 : stop < ACT ? stop : ACT - 1;
    if (last >= 0) CHECK(o.last_action == last && o.last_len == key_total(&ck[(size_t)last * kw], L), "special %d: last child %d", special, o.last_action);
    const bool budget = special < 0 && n_nodes + (int64_t)want_added.size() >= max_nodes;
    CHECK(o.status == (special >= 0 ? (error ? 3 : 1) : budget ? 2 : 0) && o.budget_hit == (int)budget && ended == (o.status != 0),
          "special %d error %d: status %d budget %d ended %d", special, (int)error, o.status, o.budget_hit, (int)ended);
    if (o.status == 1) {
        int32_t first[2];
        CHECK(read_found(o, L, first, nullptr) == 1 && first[0] == key_letter(key_code_at(&ck[(size_t)special * kw], L, 0, 0)),
              "special %d: found letters", special);
        // len(tree_nodes) - len(to_explore): the appends before the success went to both
        CHECK(o.found_parent == 7 && o.found_action == special && o.found_explored == n_nodes - n_open,
              "special %d: found parent %lld action %d explored %lld", special, (long long)o.found_parent, o.found_action,
              (long long)o.found_explored);
    }
}

int main(int argc, char** argv) {
    rng.seed(argc > 1 ? std::strtoull(argv[1], nullptr, 10) : 1);
    check_key_fields();
    check_prio_key();
    check_heap(4, 4000);
    check_heap(12, 4000);
    check_recent(true);
    check_recent(false);
    for (int special : {-1, 0, 5, 11})
        for (bool error : {false, true})
            for (int64_t max_nodes : {61, 62})  // 50 nodes + 11 appends: the budget reached / not
                if (special >= 0 || !error) check_replay(special, error, max_nodes);
    if (fails) {
        std::printf("FAILED: %d checks\n", fails);
        return 1;
    }
    std::printf("ok: key fields, priority key, heap order, in-flight table, per-child replay\n");
    return 0;
}
