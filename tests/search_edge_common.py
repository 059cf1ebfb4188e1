"""What tests/test_search_edge_cpu.py and tests/test_gpu_search_edge.py share: the relator lengths at
which a search engine's key-word instantiation or its key layout changes, the starts whose searches
turn on the top key word of a relator's tile, and the yardsticks' runs of them.

EDGE_L.  bfs::nw_for (csrc/acx_bfs_common.h) picks the instantiation NW = 1, 2, 3, 4 for L up to 16,
32, 48, 64 and 8 above; a key has key_words(L) = ceil((4 L + 16) / 64) uint64 words
(csrc/acx_expand_kernels.h), which is NW + 1 from L = 16 NW - 3 on (at 16 NW - 3 .. 16 NW - 1 the two
length bytes straddle a word, at the full tile 16 NW they open a word of their own) and steps every
16 letters inside NW = 8.  TILE_L holds both sides of every nw_for edge, every full tile, a
straddling length of every class, one key-word step inside NW = 8 (76 | 77), and ACX_MAX_L with its
neighbour; KW_STEP_L adds both sides of every other step of key_words up to ACX_MAX_L.

The starts, four per L, both relators zero-padded to L (x = 1, y = 2):
    P1 = ([x], y^(L-1))    P0 = (y^(L-1), [x])       the power starts
    N1 = ([x], v)          N0 = (v, [x])             the near-full starts; v a seeded, freely
                                                     reduced word of L - 1 letters, y first and last
The root's children by the two concatenations with [x]^+-1 (ids 0 and 2 on P1 / N1, 1 and 3 on
P0 / N0) are the long relator with x or x^-1 appended: L letters, a full tile.  The twins differ in
one 2-bit field, the last letter of that relator: bit 2 (2L - 1) of the key on P1 / N1, bit
2 (L - 1) on P0 / N0, the top of the relator's tile.  A visited-set compare, a hash, a queue copy or
a priority compare that drops or mis-shifts that word merges or mis-orders the twins.  On the power
starts the twins are the two least frontier entries after the root, equal in total (L + 1) and
depth (1): greedy's second pop is decided at the last tuple position a comparison can reach.

At L = 16 NW - 3 the last key word holds nothing but the high half of the second length byte, and no
pair of the four starts' nodes differs there alone.  From L = 29 on those lengths get a fifth start,
    T1 = (x^16, y^(L-17))
whose first child (id 0) appends x^16 to the second relator: x has letter code 0, as padding has, so
the child's key differs from the root's in that half byte only.  (At L = 13 it is always zero.)

Budgets per start, from the yardstick's own run at the mid budget (40 on the power starts, 300 on
the near-full ones): nodes_after[1] (the search ends right after its second parent or pop; under
greedy the returned path then begins with the id of the twin that was popped), the mid budget, 1."""
import functools

import numpy as np

import bfs_yardstick as YB
import greedy_yardstick as YG

TILE_L = [15, 16, 17, 31, 32, 33, 47, 48, 49, 63, 64, 65, 76, 77, 127, 128]
KW_STEP_L = [12, 13, 28, 29, 44, 45, 60, 61, 92, 93, 108, 109, 124, 125]
EDGE_L = sorted(TILE_L + KW_STEP_L)
X, Y = 1, 2
MID = {"P1": 40, "P0": 40, "N1": 300, "N0": 300, "T1": 40}
# start: (the half that holds the long relator, the two twin ids, x first then x^-1)
TWINS = {"P1": (1, (0, 2)), "N1": (1, (0, 2)), "P0": (0, (3, 1)), "N0": (0, (3, 1))}
CASES = [(L, cyc) for L in EDGE_L for cyc in (False, True)]


def twin_bit(name, L):
    """the key bit at which the twins' one differing field begins"""
    return 2 * (TWINS[name][0] * L + L - 1)


def near_full_word(L):
    """a freely reduced word of L - 1 letters that begins and ends with y, seeded by L"""
    rng = np.random.default_rng(7000 + L)
    while True:
        v = [Y]
        while len(v) < L - 2:
            c = int(rng.choice([1, -1, 2, -2]))
            if c != -v[-1]:
                v.append(c)
        if v[-1] != -Y:
            return v + [Y]


def starts(L):
    """{name: (2L,) int32}"""
    out = {}
    for name, long in (("P1", [Y] * (L - 1)), ("P0", [Y] * (L - 1)), ("N1", near_full_word(L)), ("N0", near_full_word(L))):
        s = np.zeros(2 * L, np.int32)
        half = TWINS[name][0]
        s[half * L:half * L + L - 1] = long
        s[(1 - half) * L] = X
        s.setflags(write=False)
        out[name] = s
    if L % 16 == 13 and L >= 29:
        s = np.zeros(2 * L, np.int32)
        s[:16], s[L:2 * L - 17] = X, Y
        s.setflags(write=False)
        out["T1"] = s
    return out


def _runs(search, start, mid, cyc, **kw):
    """[(budget, the yardstick's run)] at nodes_after[1] of the mid run, the mid budget and 1"""
    big = search(start, mid, cyc, **kw)
    assert len(big["nodes_after"]) >= 2, "the search has no second parent"
    return [(b, big if b == mid else search(start, b, cyc, **kw)) for b in (big["nodes_after"][1], mid, 1)]


@functools.lru_cache(maxsize=None)
def cases(L, cyc):
    """{name: dict(start, mid, bfs=[(budget, run)], greedy=[(budget, run)])}: the runs carry the
    stored states (bfs: states; greedy: stored, runner_up)"""
    out = {}
    for name, s in starts(L).items():
        out[name] = dict(start=s, mid=MID[name], bfs=_runs(YB.bfs, s, MID[name], cyc, states=True),
                         greedy=_runs(YG.greedy, s, MID[name], cyc, shape=True))
    return out


def mid_run(case, engine):
    return next(y for b, y in case[engine] if b == case["mid"])


def want_result(y):
    """what a search function returns for the yardstick's run y ("raises": it raises)"""
    if y["raises"]:
        return "raises"
    return (y["ok"], None if y["path"] is None else [tuple(x) for x in y["path"]])
