"""Presentations with a cancellation of a chosen depth planted in them (numpy only, no torch, no
kernel): the inputs of tests/test_gpu_deep_cancellation.py, checked against the oracle alone by
tests/test_planted_rows.py.  All letters are +-1 / +-2 (the packed domain).

Every kernel finds a concatenation's junction cancellation count, and the cyclic peel after it, as
the first set bit of a mismatch mask spread over several machine words (16 letters per 32-bit packed
word, 64 per plane word), so the depths planted are the ones next to a word boundary:

    DEPTHS(L) = {0, 1} + {16j - 1, 16j, 16j + 1 : j = 1..7} + {L - 2}

plant() builds one row for a concatenation move id a in 0..3 (r_i <- r_i r_j^sign, oracle
acx_oracle_decode: id 0 r1 r0, id 1 r0 r1^-1, id 2 r1 r0^-1, id 3 r0 r1):

    r_i       = p A u                       |u| = k, the junction depth
    r_j^sign  = u^-1 B p^-1                 |p| = m, the cyclic peel's depth
    product   = p A B p^-1  (not cyclical)  ->  A B  (cyclical)

with both relators freely and cyclically reduced, p A B p^-1 freely reduced (so the junction stops
after exactly k letters) and A B not peelable (so the peel stops after exactly m).  The move is
applied when the product before the peel, 2m + |A| + |B| letters, is at most L; otherwise it leaves
the row as it is with err 0 (the reference's length gate comes before its cyclic reduction).

A set of rows is a dict of arrays of equal first dimension: rows (N, 2L) int32, ids, k, m, ta, tb
(|A|, |B|), applies (the gate), want_flat / want_cyc (the row after the move, not cyclical /
cyclical -- the constructed result, not the oracle's).
"""
import functools

import numpy as np

PLANTED_L = [17, 32, 33, 36, 48, 49, 64, 65, 100, 127, 128]
TAILS = ((1, 1), (0, 2), (2, 0), (3, 5))
LETTERS = (1, 2, -1, -2)
# move id -> (target relator i, sign of the appended relator), oracle/acx_oracle.c acx_oracle_decode
CONCAT = {0: (1, 1), 1: (0, -1), 2: (1, -1), 3: (0, 1)}


def depths(L):
    d = {0, 1, L - 2}
    for j in range(1, 8):
        d |= {16 * j - 1, 16 * j, 16 * j + 1}
    return sorted(x for x in d if 0 <= x < L)


def inv(w):
    return [-x for x in reversed(w)]


def is_reduced(w):
    return all(w[i] != -w[i + 1] for i in range(len(w) - 1))


def is_cyc_reduced(w):
    return is_reduced(w) and (len(w) < 2 or w[0] != -w[-1])


def reduced_word(rng, n, after=0):
    """n random letters, freely reduced, the first one not the inverse of `after`"""
    w = []
    for _ in range(n):
        c = [x for x in LETTERS if x != -after]
        after = c[int(rng.integers(len(c)))]
        w.append(after)
    return w


def junction_depth(left, right):
    """letters that cancel at the junction of left . right"""
    k = 0
    while k < min(len(left), len(right)) and left[-1 - k] == -right[k]:
        k += 1
    return k


def peel_depth(w):
    """letters the cyclic reduction takes off each end of the freely reduced word w"""
    p = 0
    while p < len(w) and w[p] == -w[len(w) - 1 - p]:
        p += 1
    return p


def relators(row, L):
    row = [int(x) for x in row]
    return [x for x in row[:L] if x], [x for x in row[L:] if x]


def pad_row(r0, r1, L):
    assert 0 < len(r0) <= L and 0 < len(r1) <= L
    row = np.zeros(2 * L, np.int32)
    row[:len(r0)] = r0
    row[L:L + len(r1)] = r1
    return row


def fits(L, k, m, tail):
    """both relators of plant(L, ., k, m, tail) have at most L letters"""
    return k + m + max(tail) <= L and k + m + min(tail) >= 1


def applies(L, m, tail):
    return 2 * m + tail[0] + tail[1] <= L


def plant(L, a, k, m, tail, rng):
    """one row for move id a with junction depth k, peel depth m and tails (|A|, |B|): (row,
    want_flat, want_cyc) -- a rejection loop over seeded reduced words"""
    i, sign = CONCAT[a]
    ta, tb = tail
    assert fits(L, k, m, tail), (L, k, m, tail)
    for _ in range(10000):
        p = reduced_word(rng, m)
        A = reduced_word(rng, ta, p[-1] if p else 0)
        u = reduced_word(rng, k, (p + A)[-1] if p or A else 0)
        B = reduced_word(rng, tb, -u[0] if u else 0)
        ri, w, prod, core = p + A + u, inv(u) + B + inv(p), p + A + B + inv(p), A + B
        if is_cyc_reduced(ri) and is_cyc_reduced(w) and is_reduced(prod) and is_cyc_reduced(core):
            break
    else:
        raise AssertionError(("no row found", L, a, k, m, tail))
    rj = w if sign == 1 else inv(w)
    rel = [None, None]
    rel[i], rel[1 - i] = ri, rj
    row = pad_row(rel[0], rel[1], L)
    if not applies(L, m, tail):
        return row, row.copy(), row.copy()
    rel[i] = prod
    flat = pad_row(rel[0], rel[1], L)
    rel[i] = core
    return row, flat, pad_row(rel[0], rel[1], L)


def _collect(L, specs, rng):
    keys = ("rows", "ids", "k", "m", "ta", "tb", "applies", "want_flat", "want_cyc")
    out = {x: [] for x in keys}
    for a, k, m, tail in specs:
        row, flat, cyc = plant(L, a, k, m, tail, rng)
        for x, v in zip(keys, (row, a, k, m, tail[0], tail[1], applies(L, m, tail), flat, cyc)):
            out[x].append(v)
    shape = {"rows": (len(specs), 2 * L), "want_flat": (len(specs), 2 * L), "want_cyc": (len(specs), 2 * L)}
    return {x: np.array(v, bool if x == "applies" else np.int32).reshape(shape.get(x, (len(specs),)))
            for x, v in out.items()}


def junction_specs(L):
    """(id, k, m, tail) of junction_rows(L): every (k, m) in DEPTHS(L)^2 with max(k, m) >= 15 and every
    tail that fits, the move ids dealt round robin; the first applied combination of every k gets all
    four ids, so that every (id, k) occurs among the applied rows"""
    specs, n, seen = [], 0, set()
    for k in depths(L):
        for m in depths(L):
            if max(k, m) < 15:
                continue
            for tail in TAILS:
                if not fits(L, k, m, tail):
                    continue
                if applies(L, m, tail) and k not in seen:
                    seen.add(k)
                    specs += [(a, k, m, tail) for a in range(4)]
                else:
                    specs.append((n % 4, k, m, tail))
                    n += 1
    return specs


def _frozen(s):
    """the sets are computed once per L and shared: read-only arrays"""
    for v in s.values():
        v.setflags(write=False)
    return s


@functools.lru_cache(maxsize=None)
def junction_rows(L, seed=0):
    return _frozen(_collect(L, junction_specs(L), np.random.default_rng(100 * L + seed)))


def gate_specs(L):
    """{class: [(id, k, m, tail)]} of gate_rows(L).
      len_L / len_L1 / len_L2: the deepest junctions whose product before the peel has exactly L,
        L + 1 and L + 2 letters (the first is applied, the others leave the row as it is);
      cancel_to_fit: |r_i| + |r_j| > L, the product fits only because of the cancellation;
      peel_to_fit: small k, deep m -- the product exceeds L before the peel and not after it: left
        as it is under either flag (the gate comes before the peel, and without the peel the product
        does not fit at all)."""
    g = {"len_L": [], "len_L1": [], "len_L2": [], "cancel_to_fit": [], "peel_to_fit": []}
    n = 0
    for e, name in enumerate(("len_L", "len_L1", "len_L2")):
        for m in (0, 1):
            t = L + e - 2 * m
            tail = ((t + 1) // 2, t // 2)
            kmax = L - m - max(tail)
            for k in sorted({kmax} | {d for d in depths(L) if 15 <= d <= kmax}):
                if k >= 1 and fits(L, k, m, tail):
                    g[name] += [(n % 4, k, m, tail), ((n + 1) % 4, k, m, tail[::-1])]
                    n += 2
    for k in (L - 2, L // 2, L // 2 + 1):
        for m in (0, 1):
            for tail in TAILS[:3]:
                if fits(L, k, m, tail) and 2 * (k + m) + sum(tail) > L and applies(L, m, tail):
                    g["cancel_to_fit"].append((n % 4, k, m, tail))
                    n += 1
    for k in (0, 1, 2):
        for m in sorted({L // 2, (L + 1) // 2, L - 2 - k}):
            for tail in TAILS[:3]:
                if fits(L, k, m, tail) and not applies(L, m, tail) and sum(tail) <= L:
                    g["peel_to_fit"].append((n % 4, k, m, tail))
                    n += 1
    return g


@functools.lru_cache(maxsize=None)
def gate_rows(L, seed=0):
    """{class: set of rows}, see gate_specs"""
    rng = np.random.default_rng(100 * L + 50 + seed)
    return {name: _frozen(_collect(L, specs, rng)) for name, specs in gate_specs(L).items()}


@functools.lru_cache(maxsize=None)
def nested_rows(L, seed=0):
    """Unreduced relators a v v^-1 b with |v| in DEPTHS(L), in r0 and in r1 in turn (the other
    relator is a cyclically reduced random word); every second one carries a cascade a = a' c,
    b = c^-1 b', so that the cancellation goes on past v.  a b (a' b') is cyclically reduced: the row
    reduces to it under either flag.  Returns {rows, want, depth (|v| + |c|), half, cascade}."""
    rng = np.random.default_rng(100 * L + 70 + seed)
    rows, want, depth, half, casc = [], [], [], [], []
    n = [0, 0]  # rows so far without / with a cascade: each kind goes to r0 and r1 in turn
    for v_len in depths(L):
        if v_len < 1:
            continue
        for la, lb in ((1, 1), (0, 2), (3, 0), (2, 3)):
            for cascade in (0, 1):
                room = L - 2 * v_len - la - lb
                if room < 0 or (cascade and room < 2):
                    continue
                lc = 0 if not cascade else 1 + int(rng.integers(min(room // 2, 17)))
                for _ in range(10000):
                    a1 = reduced_word(rng, la)
                    c = reduced_word(rng, lc, a1[-1] if a1 else 0)
                    v = reduced_word(rng, v_len, (a1 + c)[-1] if a1 or c else 0)
                    b1 = reduced_word(rng, lb)
                    if is_cyc_reduced(a1 + b1) and is_reduced(a1 + c + v) and is_reduced(inv(c + v) + b1):
                        break
                else:
                    raise AssertionError(("no nested row", L, v_len, la, lb, cascade))
                word = a1 + c + v + inv(v) + inv(c) + b1
                for _ in range(10000):
                    other = reduced_word(rng, 1 + int(rng.integers(L)))
                    if is_cyc_reduced(other):
                        break
                h = n[cascade] % 2
                n[cascade] += 1
                rows.append(pad_row(*((word, other) if h == 0 else (other, word)), L))
                want.append(pad_row(*((a1 + b1, other) if h == 0 else (other, a1 + b1)), L))
                depth.append(v_len + lc)
                half.append(h)
                casc.append(cascade)
    return _frozen({"rows": np.array(rows, np.int32), "want": np.array(want, np.int32),
                    "depth": np.array(depth, np.int32), "half": np.array(half, np.int32),
                    "cascade": np.array(casc, bool)})


def unclean_twin(planted, L):
    """The rows of a junction / gate set with one cancelling pair x x^-1 inserted in the middle of
    a tail, away from the junction (in A inside r_i, or where A is empty in B inside r_j), where the
    relator has room for two more letters: the row is no longer freely reduced, so a kernel cannot
    take its clean-row move (ac_move_clean), while the raw junction still cancels exactly k letters.
    Returns {rows, ids, k, src (the index of the row it was made from)}."""
    rows, ids, ks, src = [], [], [], []
    for n, row in enumerate(planted["rows"]):
        a, k, m = int(planted["ids"][n]), int(planted["k"][n]), int(planted["m"][n])
        ta, tb = int(planted["ta"][n]), int(planted["tb"][n])
        i, sign = CONCAT[a]
        rel = list(relators(row, L))
        if ta:
            h, at = i, m + ta // 2
        else:  # r_j is u^-1 B p^-1 (sign +1) or its inverse p B^-1 u
            h, at = 1 - i, (k if sign == 1 else m) + tb // 2
        w = rel[h]
        if len(w) + 2 > L:
            continue
        prev, nxt = (w[at - 1] if at else 0), (w[at] if at < len(w) else 0)
        x = next(c for c in LETTERS if c != -prev and c != nxt)
        rel[h] = w[:at] + [x, -x] + w[at:]
        rows.append(pad_row(rel[0], rel[1], L))
        ids.append(a)
        ks.append(k)
        src.append(n)
    return {"rows": np.array(rows, np.int32).reshape(len(rows), 2 * L), "ids": np.array(ids, np.int32),
            "k": np.array(ks, np.int32), "src": np.array(src, np.int32)}


def concat_sets(sets):
    """one set out of several: the keys they all have, concatenated"""
    keys = set.intersection(*(set(s) for s in sets))
    return {x: np.concatenate([s[x] for s in sets]) for x in keys}
