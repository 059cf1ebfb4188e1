// acx_frontier.h -- the host half of greedy_search (ac_solver/search/greedy.py:71-119) shared by
// the host engine (acx_search.cpp) and the device-visited-set engine (acx_greedy.hip): the
// priority key, the ordered frontier, the in-flight table, the per-child replay of a popped node
// and the result readers.  Host only, plain C++17 (tests/frontier_check.cpp runs it on the CPU).
#pragma once
#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "acx.h"
#include "acx_key.h"

namespace acx {

constexpr int ACT = 12;
constexpr int PRIO_HDR = 40;  // priority-key header bits: total (9) | path length (31)
inline int prio_words(int L) { return (PRIO_HDR + 6 * L + 63) / 64; }

// the heap key: total (9 bits) | path length (31) | every letter + 2 in 3 bits, MSB first
// (x = 3, x^-1 = 1, y = 4, y^-1 = 0, padding = 2; r0 then r1), pk = prio_words(L) words: unsigned
// word order = Python's tuple order of (total, path length, state tuple) (greedy.py:55-64,
// 104-113).  generic: the per-group path at every L (tests; it is the only one above L = 40).
inline void prio_key(const uint64_t* k, int L, int kw, int pk, int tot, int dep, uint64_t* out, bool generic = false) {
    static const uint32_t val[4] = {3, 1, 4, 0};
    struct Tbl {  // 4 letters (one byte of codes) -> their 12 bits
        uint16_t t[256];
        Tbl() {
            for (int b = 0; b < 256; ++b) {
                uint32_t v = 0;
                for (int j = 0; j < 4; ++j) v = (v << 3) | val[(b >> (2 * j)) & 3];
                t[b] = (uint16_t)v;
            }
        }
    };
    static const Tbl T;
    const uint16_t* tbl = T.t;
    for (int i = 0; i < pk; ++i) out[i] = 0;
    out[0] = ((uint64_t)(tot & 0x1ff) << 55) | ((uint64_t)(dep & 0x7fffffff) << 24);
    int pos = PRIO_HDR;
    auto put = [&](uint64_t v, int nbits) {  // append nbits (<= 61) MSB-first
        const int w = pos >> 6, o = pos & 63;
        if (o + nbits <= 64) {
            out[w] |= v << (64 - o - nbits);
        } else {
            out[w] |= v >> (o + nbits - 64);
            out[w + 1] |= v << (128 - o - nbits);
        }
        pos += nbits;
    };
    constexpr uint64_t PAD20 = 0x492492492492492ull;  // 20 x 010 (60 bits): padding letters
    if (L <= 40 && !generic) {
        // a relator's 2L code bits are taken in one 128-bit shift and mapped 4 letters per
        // table lookup into two 60-bit parts (letters 0..19, 20..L-1); the padding letters'
        // fields replaced by 010s with one mask per part -- a few appends instead of one per
        // 4 letters (the general path below, which this reproduces bit for bit)
        using u128 = unsigned __int128;
        for (int h = 0; h < 2; ++h) {
            const int n = key_len(k, L, h);
            const int b0 = 2 * h * L, w = b0 >> 6, o = b0 & 63;
            u128 codes = ((u128)k[w] | ((u128)(w + 1 < kw ? k[w + 1] : 0ull) << 64)) >> o;
            if (o + 2 * L > 128 && w + 2 < kw) codes |= (u128)k[w + 2] << (128 - o);
            auto part = [&](int f, int cnt) -> uint64_t {  // letters [f, f + cnt), cnt <= 20
                const int groups = (cnt + 3) / 4;
                uint64_t v = 0;
                for (int g = 0; g < groups; ++g) v = (v << 12) | tbl[(uint32_t)(codes >> (2 * f + 8 * g)) & 0xffu];
                v >>= 3 * (4 * groups - cnt);  // the letters past the part in its last group
                const int live = n - f < 0 ? 0 : (n - f > cnt ? cnt : n - f);
                if (live < cnt) {
                    const uint64_t mask = (1ull << (3 * (cnt - live))) - 1;
                    v = (v & ~mask) | (PAD20 & mask);
                }
                return v;
            };
            const int c0 = L < 20 ? L : 20;
            put(part(0, c0), 3 * c0);
            if (L > 20) put(part(20, L - 20), 3 * (L - 20));
        }
        return;
    }
    for (int h = 0; h < 2; ++h) {
        const int n = key_len(k, L, h);
        int i = 0;
        for (; i + 4 <= n; i += 4) put(tbl[key_byte(k, 2 * (h * L + i))], 12);
        for (; i < n; ++i) put(val[key_code_at(k, L, h, i)], 3);
        for (int m = L - n; m > 0; m -= 20) {
            const int c = m < 20 ? m : 20;
            put(PAD20 >> (3 * (20 - c)), 3 * c);
        }
    }
}

// 4-ary min-heap of node ids ordered by their heap keys (pk words per id in *keys, written once
// when a node is appended).  An entry is the key's first word (total | path length | the first 24
// letter bits: nearly always decides) and the id, 16 bytes; the rest of the key is read from
// *keys only on a tie of first words, so a sift copies 16 bytes per level whatever pk is.
struct Heap {
    struct Ent {
        uint64_t k0;
        int64_t id;
    };
    int pk = 0;
    const std::vector<uint64_t>* keys = nullptr;
    std::vector<Ent> e;
    bool less(const Ent& x, const Ent& y) const {
        if (x.k0 != y.k0) return x.k0 < y.k0;
        const uint64_t* a = keys->data() + (size_t)x.id * pk;
        const uint64_t* b = keys->data() + (size_t)y.id * pk;
        for (int i = 1; i < pk; ++i)
            if (a[i] != b[i]) return a[i] < b[i];
        return false;
    }
    bool empty() const { return e.empty(); }
    size_t size() const { return e.size(); }
    int64_t top() const { return e[0].id; }
    void push(uint64_t k0, int64_t v) {
        size_t i = e.size();
        e.push_back(Ent{k0, v});
        const Ent x{k0, v};
        while (i > 0) {
            const size_t par = (i - 1) / 4;
            if (!less(x, e[par])) break;
            e[i] = e[par];
            i = par;
        }
        e[i] = x;
    }
    void pop() {
        const size_t n = e.size() - 1;
        const Ent x = e[n];
        e.pop_back();
        if (n == 0) return;
        size_t i = 0;
        while (true) {
            const size_t c0 = 4 * i + 1;
            if (c0 >= n) break;
            size_t best = c0;
            const size_t ce = c0 + 4 < n ? c0 + 4 : n;
            for (size_t c = c0 + 1; c < ce; ++c)
                if (less(e[c], e[best])) best = c;
            if (!less(e[best], x)) break;
            e[i] = e[best];
            i = best;
        }
        e[i] = x;
    }
};
// one heap per total (the priority key's top 9 bits): a pop sifts through the nodes of the
// smallest total only, not the whole frontier (10^6 nodes: ~10 cold levels per pop); the order
// is the single heap's, since the total is the key's most significant field
struct BucketHeap {
    static constexpr int NB = 512;
    int minb = NB;  // the smallest non-empty bucket (NB: none)
    size_t n = 0;
    std::vector<Heap> b;
    void init(int pk, const std::vector<uint64_t>* keys) {
        b.assign(NB, Heap{});
        for (Heap& h : b) {
            h.pk = pk;
            h.keys = keys;
        }
        minb = NB;
        n = 0;
    }
    bool empty() const { return n == 0; }
    size_t size() const { return n; }
    void push(uint64_t k0, int64_t v) {
        const int i = (int)(k0 >> 55);
        b[(size_t)i].push(k0, v);
        if (i < minb) minb = i;
        ++n;
    }
    int64_t top() const { return b[(size_t)minb].top(); }
    void pop() {
        b[(size_t)minb].pop();
        --n;
        while (minb < NB && b[(size_t)minb].empty()) ++minb;
    }
};

// The recently appended nodes (the device engine's in-flight set), two generations of up to `age`
// ids each (age a power of two): gen[cur] holds ids >= gen_lo[cur], gen[cur ^ 1] the `age` ids
// before them; open addressing with entries (id + 1) << 16 | 16-bit tag, so a probe reads a
// node's key (key_of(id), kw words) only on a tag hit.
template <class KeyOf>
struct Recent {
    int64_t age = 0;
    int kw = 0;
    KeyOf key_of{};
    std::vector<uint64_t> gen[2];
    int64_t gen_lo[2] = {0, 0};
    int cur = 0;
    uint64_t gmask = 0;
    Recent() = default;
    Recent(int64_t age_, int kw_, KeyOf key_of_) : age(age_), kw(kw_), key_of(key_of_), gmask(2 * (uint64_t)age_ - 1) {
        for (auto& g : gen) g.assign((size_t)2 * age, 0ull);
    }
    static uint64_t tag_of(uint64_t h) { return (h >> 48) & 0xffffu; }
    void insert(int64_t id, uint64_t h) {
        if (id - gen_lo[cur] >= age) {  // the current generation is full: it becomes the older one
            cur ^= 1;
            std::fill(gen[cur].begin(), gen[cur].end(), 0ull);
            gen_lo[cur] = id;
        }
        std::vector<uint64_t>& g = gen[cur];
        uint64_t s = h & gmask;
        while (g[s]) s = (s + 1) & gmask;
        g[s] = ((uint64_t)(id + 1) << 16) | tag_of(h);
    }
    // a node with id >= from equal to key k, or -1 (from >= the older generation's first id: the
    // caller admits only children probed fewer than `age` appends ago)
    int64_t find(const uint64_t* k, uint64_t h, int64_t from) const {
        const uint64_t tag = tag_of(h);
        for (int i = 0; i < 2; ++i) {
            if (i == 1 && gen_lo[cur] <= from) break;  // every id >= from is in the current one
            const std::vector<uint64_t>& g = gen[cur ^ i];
            for (uint64_t s = h & gmask; g[s]; s = (s + 1) & gmask) {
                if ((g[s] & 0xffffu) != tag) continue;
                const int64_t id = (int64_t)(g[s] >> 16) - 1;
                if (id >= from && memcmp(key_of(id), k, 8 * (size_t)kw) == 0) return id;
            }
        }
        return -1;
    }
};

// what a search leaves behind (greedy.py:86-121, breadth_first.py:76-97)
struct Outcome {
    int status = 0;  // 0 running, 1 success, 2 failed (budget or exhausted), 3 move error
    int budget_hit = 0;
    int min_length = 0;
    std::vector<int32_t> trace;   // each new minimum total, in the order found
    std::vector<int64_t> popped;  // node ids in expansion (pop) order
    int64_t found_parent = -1, last_popped = -1;
    int64_t found_explored = 0;  // len(tree_nodes) - len(to_explore) at the success (greedy.py:94)
    int found_action = -1, last_action = -1, last_len = -1;
    uint64_t found_key[ACX_MAX_L / 16 + 2] = {0};
};

// Expand the popped node `id` from its 12 child keys ck (hashes hs) in the reference's per-child
// order: move error (utils.py:264-266, before any test), new minimum (greedy.py:86-89), success
// (:91-100), dedup (:102), append (:104-113); then the budget test (:115-119).  seen(k, h, a)
// answers "already a node", add(k, h, a, len) appends one.  n_nodes = len(tree_nodes) and n_open
// = len(to_explore) as the node is popped.  Returns true when the search ends here.
template <class Seen, class Add>
bool replay_children(const uint64_t* ck, const uint64_t* hs, int L, int kw, Outcome& o, int64_t id, int64_t n_nodes,
                     int64_t n_open, int64_t max_nodes, Seen&& seen, Add&& add) {
    o.last_popped = id;
    o.popped.push_back(id);
    const int64_t explored = n_nodes - n_open;  // unchanged by the appends: each goes to both
    for (int a = 0; a < ACT; ++a) {
        const uint64_t* k = ck + (size_t)a * kw;
        if (key_is_error(k, L)) {
            o.status = 3;
            return true;
        }
        const int len = key_total(k, L);
        o.last_action = a;
        o.last_len = len;
        if (len < o.min_length) {
            o.min_length = len;
            o.trace.push_back(len);
        }
        if (len == 2) {
            o.status = 1;
            o.found_parent = id;
            o.found_action = a;
            o.found_explored = explored;
            memcpy(o.found_key, k, 8 * (size_t)kw);
            return true;
        }
        if (seen(k, hs[a], a)) continue;
        add(k, hs[a], a, len);
        ++n_nodes;
    }
    if (n_nodes >= max_nodes) {
        o.status = 2;
        o.budget_hit = 1;
        return true;
    }
    return false;
}

// ---- result readers (the acx_search_* / acx_greedy_* C functions of acx.h) over raw node arrays

inline int32_t read_status(const Outcome& o, int64_t nodes, int32_t* budget_hit, int32_t* min_length,
                           int64_t* n_nodes) {
    if (budget_hit) *budget_hit = o.budget_hit;
    if (min_length) *min_length = o.min_length;
    if (n_nodes) *n_nodes = nodes;
    return o.status;
}

// the returned path as (action, total) pairs from the root (root = (-1, total)): success -> the
// found child's; otherwise the last popped node's plus its last child (greedy.py:100,121).
// Returns the number of entries (which may exceed cap).
inline int64_t read_path(const Outcome& o, const int64_t* parent, const int8_t* action, const int16_t* total,
                         int32_t* acts, int32_t* lens, int64_t cap) {
    const bool found = o.status == 1;
    const int64_t v0 = found ? o.found_parent : o.last_popped;
    if (v0 < 0) return 0;
    std::vector<int64_t> chain;
    for (int64_t v = v0; v >= 0; v = parent[v]) chain.push_back(v);
    int64_t n = 0;
    for (auto it = chain.rbegin(); it != chain.rend(); ++it, ++n)
        if (n < cap) {
            acts[n] = action[*it];
            lens[n] = total[*it];
        }
    if (n < cap) {
        acts[n] = found ? o.found_action : o.last_action;
        lens[n] = found ? 2 : o.last_len;
    }
    return n + 1;
}

// after a success: the first letters of both relators of the found child (each of length 1) and
// len(tree_nodes) - len(to_explore) at that moment (greedy.py:92-95); returns 1, else 0
inline int32_t read_found(const Outcome& o, int L, int32_t* first_letters, int64_t* explored) {
    if (o.status != 1) return 0;
    if (first_letters) key_first_letters(o.found_key, L, first_letters);
    if (explored) *explored = o.found_explored;
    return 1;
}

// copy the first min(n, cap) of src's n elements (w words each); returns n
template <class T>
int64_t read_array(const T* src, int64_t n, T* out, int64_t cap, int w = 1) {
    const int64_t m = n < cap ? n : cap;
    if (out && m > 0) memcpy(out, src, sizeof(T) * (size_t)m * w);
    return n;
}

}  // namespace acx
