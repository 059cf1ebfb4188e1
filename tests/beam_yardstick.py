"""The reference's beam_search (value_search/value_guided_search.py:417-561, solution_cache=None,
time_limit=None) restated over the CPU oracle's 12-way expansion (oracle.expand12), with Python's
own stable sort on the scores: the yardstick of the batched beam tests.  tests/test_beam_cpu.py
checks it against the reference's own recorded runs (tests/golden/beam_search.json).

The scorers are functions of the 14 raw features whose float32 values are exact (small integers
and quarters), so they give the same scores here, in the reference on the CPU and on the GPU; each
is stated once for numpy and once for torch.  Below them are the real-valued ones: scorers on
normalised features (negative and non-integer scores), a token scorer, and a table of floats over
the whole float line."""
import numpy as np

from oracle import oracle as O

EXHAUSTED, FOUND, BUDGET, MOVE_ERROR = 0, 1, 2, 3  # ACX_BFS_* of include/acx.h


def features_np(states, L):
    """compute_features (feature_extraction.py:11-91) of (k, 2L) rows in the packed domain -> (k, 14)
    float32, vectorised (oracle.features.compute_features row by row is the same, and slow)"""
    s = np.asarray(states, np.int64).reshape(-1, 2 * L)
    h = [s[:, :L], s[:, L:]]
    n = [(x != 0).sum(1) for x in h]
    c = [[(x == v).sum(1) for v in (1, -1, 2, -2)] for x in h]
    tot = n[0] + n[1]
    ex = (c[0][0] - c[0][1]) + (c[1][0] - c[1][1])
    mn, mx = np.minimum(n[0], n[1]), np.maximum(n[0], n[1])
    ratio = np.where(tot > 0, n[0] / np.maximum(tot, 1), 0.5)
    mmr = np.where(mn > 0, mx / np.maximum(mn, 1), mx)
    return np.stack([tot, n[0], n[1], *c[0], *c[1], ex, ratio, mmr], 1).astype(np.float32)


# name -> (numpy form, torch form) on the (k, 14) features: 0 total, 2 len_r2, 3 count_x_r1,
# 10 count_yinv_r2
def _s4_np(f):
    return np.where(f[:, 0] % 2 == 0, np.float32(-0.0), np.float32(0.0)).astype(np.float32)


def _s4_t(f):
    import torch
    return torch.where(f[:, 0] % 2 == 0, torch.full_like(f[:, 0], -0.0), torch.zeros_like(f[:, 0]))


SCORERS = {
    "S0": (lambda f: f[:, 0], lambda f: f[:, 0]),  # total length: heavy ties
    "S1": (lambda f: f[:, 2] + np.abs(f[:, 3] - f[:, 10]), lambda f: f[:, 2] + (f[:, 3] - f[:, 10]).abs()),
    "S1q": (lambda f: np.float32(0.25) * (f[:, 2] + np.abs(f[:, 3] - f[:, 10])),
            lambda f: 0.25 * (f[:, 2] + (f[:, 3] - f[:, 10]).abs())),  # S1 scaled for L = 128 (expm1 finite)
    "S2": (lambda f: f[:, 0] * np.float32(0), lambda f: f[:, 0] * 0),  # every score ties: generation order
    "S3": (lambda f: np.float32(-0.25) * f[:, 0], lambda f: -0.25 * f[:, 0]),
    "S4": (_s4_np, _s4_t),  # -0.0 for an even total, +0.0 for an odd one: all tie
}


# ---------------------------------------------------------------------------------------------
# real-valued scores: scorers on NORMALISED features, a token scorer, a table over the float line
# ---------------------------------------------------------------------------------------------
# The normalisation the scored fixture (tests/golden/beam_search_scored.json) and its tests pass:
# (f - mean) / std is one IEEE float32 subtract and one divide, the same in numpy, in the reference
# (value_guided_search.py:59) and in acx_features.  The integer columns 0 .. 11 have an integer
# mean and a power-of-two std, so their normalised values are small dyadic rationals and sums of
# them are exact in any order; the ratio columns 12 and 13 are only selected, negated or compared.
NORM_MEAN = np.float32([12, 4, 5, 9, 2, 8, -5, 6, -2, 7, 3, -4, -1, 1])
NORM_STD = np.float32([-4, 2, -2, 8, -8, 16, -16, 32, -0.25, 0.125, 4, -32, 0.5, 1])


def normalise_np(f, mean, std):
    """oracle.features.normalise: float32 (f - mean) / std"""
    return (np.asarray(f, np.float32) - np.asarray(mean, np.float32)) / np.asarray(std, np.float32)


def _torch():
    import torch
    return torch


NORM_SCORERS = {
    # 2 len_r1 / total + 2 under NORM_MEAN / NORM_STD: non-integers in [2, 4]
    "N12": (lambda f: f[:, 12], lambda f: f[:, 12]),
    # max / min of the lengths, minus 1
    "N13": (lambda f: f[:, 13], lambda f: f[:, 13]),
    # the length ratio against (len_r1 - 4) / 2: both columns' mean and std decide which one wins
    "NMAX": (lambda f: np.maximum(f[:, 12], f[:, 1]), lambda f: _torch().maximum(f[:, 12], f[:, 1])),
    # S1 on normalised columns; column 2's std is negative, so a longer r2 scores LOWER here and the
    # order is not the raw features' (a single column with a positive std orders as without
    # normalisation, and a search on it alone would not notice a skipped normalisation)
    "NNEG": (lambda f: f[:, 2] + np.abs(f[:, 3] - f[:, 10]), lambda f: f[:, 2] + (f[:, 3] - f[:, 10]).abs()),
}
SCORERS.update(NORM_SCORERS)


def _tok_np(t):
    t = np.asarray(t, np.int64)
    return ((t != 2).sum(1) + (t * np.arange(1, t.shape[1] + 1)).sum(1) % 7).astype(np.float32)


def _tok_t(t):
    torch = _torch()
    w = torch.arange(1, t.shape[1] + 1, dtype=torch.int64, device=t.device)
    return ((t != 2).sum(1) + (t * w).sum(1) % 7).to(torch.float32)


# the float line: +-inf, +-0.0, +-the smallest denormal, +-FLT_MAX, 1.0 and -1.0 each with both
# neighbours, and ordinary values with planted duplicates (as bits, so that both forms hold the
# same floats)
TABLE_BITS = np.array([0x7f800000, 0xff800000, 0x00000000, 0x80000000, 0x00000001, 0x80000001, 0x7f7fffff, 0xff7fffff,
                       0x3f800000, 0x3f7fffff, 0x3f800001, 0xbf800000, 0xbf7fffff, 0xbf800001,
                       0x3f000000, 0x3f000000, 0x40500000, 0x40500000, 0xc0f00000, 0xc0f00000, 0x42c80000, 0xc2c80000,
                       0x3a83126f, 0xba83126f, 0x40000000, 0x40000000, 0x00800000, 0x80800000, 0x007fffff, 0x807fffff,
                       0x3eaaaaab], np.uint32)
TABLE = TABLE_BITS.view(np.float32)


def _table_hash(t, w):
    """an int64 hash of the token rows t, w = 1 .. 2L, as an index into the table"""
    return ((t * w).sum(1) + 3 * (t[:, 0] + t[:, t.shape[1] // 2])) % len(TABLE_BITS)


def _table_np(t):
    t = np.asarray(t, np.int64)
    return TABLE[_table_hash(t, np.arange(1, t.shape[1] + 1))]


_TABLE_ON = {}


def _table_t(t):
    torch = _torch()
    if t.device not in _TABLE_ON:  # a device tensor made from the same bits
        _TABLE_ON[t.device] = torch.from_numpy(TABLE_BITS.view(np.int32).copy()).to(t.device).view(torch.float32)
    w = torch.arange(1, t.shape[1] + 1, dtype=torch.int64, device=t.device)
    return _TABLE_ON[t.device].index_select(0, _table_hash(t, w))


# name -> (numpy form, torch form) on the candidates' (k, 2L) int64 token ids (letter + 2)
TOKEN_SCORERS = {
    "TOK": (_tok_np, _tok_t),  # the letters' count plus a hash of the row in 0 .. 6: integers <= 2L + 6
    "TABLE": (_table_np, _table_t),  # yardstick only: expm1 of these is not strictly increasing
}


def table_cases():
    """the TABLE searches of test_beam_cpu.py (their shape) and test_gpu_beam_many.py (their results):
    (presentation, W, budget, cyclical), one width per LDS class of the select kernel"""
    ak3 = np.zeros(36, np.int32)
    ak3[:7], ak3[18:24] = [1, 1, 1, -2, -2, -2, -2], [1, 2, 1, -2, -1, -2]
    ms = np.zeros(72, np.int32)
    ms[:9], ms[36:44] = [-1, 2, 2, 2, 1, -2, -2, -2, -2], [-1, -2, 1, -2, -2, -2, -1, -2]
    return [(ak3, 50, 3000, False), (ms, 86, 3000, True), (ak3, 342, 7000, True)]


def beam(presentation, scorer, width, max_nodes, cyclical=False, on_states=False, mean=None, std=None):
    """scorer: a name of SCORERS or TOKEN_SCORERS, or a function of the candidates' (k, 14) features
    -- with on_states=True of their (k, 2L) states -- that returns k float32 scores.  With mean and
    std the features are normalised in float32 before the scorer, as the reference does.
    The report also holds score_bits (the bit patterns of every score returned) and zero_steps (the
    steps whose scores held both +0.0 and -0.0).
    dict: status, ok, path ([] unless found), raises, nodes (total_nodes at the ending event),
    steps (steps begun), states (the nodes in node_id order), and the search's shape per step: cands[i] = candidates of step i + 1,
    nodes_after[i] = total_nodes after its expansion, and the steps (1-based) at which dup_steps: a
    child equalled an earlier new child of the same step, cut_mid: the budget cut fell before the
    last child of the step, cut_at: (step, action of the cut child, children of the step not looked
    at), tie_steps: the scores of the last selected and the first rejected candidate tied."""
    on_tokens = isinstance(scorer, str) and scorer in TOKEN_SCORERS
    score = (TOKEN_SCORERS if on_tokens else SCORERS)[scorer][0] if isinstance(scorer, str) else scorer
    assert (mean is None) == (std is None) and (mean is None or not (on_tokens or on_states))
    start = np.asarray(presentation, np.int32)
    L = len(start) // 2
    root = tuple(int(x) for x in start)
    visited = {root}
    parent = {0: (None, int(np.count_nonzero(start)), None)}
    beam_ = [(start, 0)]
    total_nodes, step = 1, 0
    out = dict(status=None, ok=False, path=[], raises=False, states=[start], cands=[], nodes_after=[], dup_steps=[],
               cut_mid=[], cut_at=[], tie_steps=[], score_bits=set(), zero_steps=[])

    def path_to(nid):
        p = []
        while parent[nid][2] is not None:
            a, t, nid2 = parent[nid]
            p.append([a, t])
            nid = nid2
        return p[::-1]

    while beam_ and total_nodes < max_nodes and out["status"] is None:
        step += 1
        ch, lens, err = O.expand12(np.stack([b[0] for b in beam_]).astype(np.int32), L, cyclical)
        new, new_set, cut = [], set(), False
        for r, (_, pid) in enumerate(beam_):
            for a in range(12):
                if err[r, a]:  # ACMove raises (utils.py:264-266)
                    out.update(status=MOVE_ERROR, raises=True)
                    break
                t = int(lens[r, a].sum())
                if t == 2:
                    out.update(status=FOUND, ok=True, path=path_to(pid) + [[a, t]])
                    break
                key = tuple(int(x) for x in ch[r, a])
                if key in new_set and out["dup_steps"][-1:] != [step]:
                    out["dup_steps"].append(step)
                if key not in visited:
                    visited.add(key)
                    new_set.add(key)
                    total_nodes += 1
                    parent[total_nodes - 1] = (a, t, pid)
                    new.append((ch[r, a].astype(np.int32), total_nodes - 1))
                    out["states"].append(new[-1][0])
                    if total_nodes >= max_nodes:
                        cut = True
                        left = 12 * len(beam_) - (12 * r + a + 1)
                        out["cut_at"].append((step, a, left))
                        if left:
                            out["cut_mid"].append(step)
                        break
            if cut or out["status"] is not None:
                break
        if out["status"] is not None:
            break
        out["cands"].append(len(new))
        out["nodes_after"].append(total_nodes)
        if not new:  # the beam died
            out["status"] = EXHAUSTED
            break
        cs = np.stack([c[0] for c in new])
        if on_tokens:
            x = cs.astype(np.int64) + 2
        elif on_states:
            x = cs
        else:
            x = features_np(cs, L)
            if mean is not None:
                x = normalise_np(x, mean, std)
        s = np.asarray(score(x), np.float32)
        assert s.shape == (len(new),) and not np.isnan(s).any()
        bits = s.view(np.uint32)
        out["score_bits"].update(np.unique(bits).tolist())
        if (bits == 0).any() and (bits == 0x80000000).any():
            out["zero_steps"].append(step)
        order = sorted(range(len(new)), key=lambda i: float(s[i]))
        if len(new) > width and float(s[order[width - 1]]) == float(s[order[width]]):
            out["tie_steps"].append(step)
        beam_ = [new[i] for i in order[:width]]
    if out["status"] is None:  # the loop condition: total_nodes >= max_nodes (a budget <= 1 runs no step)
        out["status"] = BUDGET
    out.update(nodes=total_nodes, steps=step)
    return out
