"""The reference's mcts_search (value_search/mcts.py:177-314, solution_cache=None, time_limit=None)
restated literally over the CPU oracle's 12-way expansion (oracle.expand12), with Python's own
floats for the statistics and math.log / math.sqrt for the UCB1 score: the yardstick of the batched
MCTS tests.  tests/test_mcts_cpu.py checks it against the reference's own recorded runs
(tests/golden/mcts_search.json).

Literal means: the loop test len(visited) < budget and iterations < 50 * budget before every
iteration; the descent by the least prior among unvisited children (Python's min: the first on
ties) and otherwise by the greatest -(vsum / visit) + c * sqrt(log(N) / visit) with a strict >; all
12 children made before any is judged, so a raising move ends the search even behind a trivial
child; every new state entering the visited set in action order (a twin of an earlier child of the
same expansion is then known, and dropped); prior + 50.0 backed up from a leaf without a new child;
priors max(v, 0) as Python floats and the least of them backed up otherwise.  The root is not scored
here either: its value is only ever added to its own value_sum, which nothing reads.

The values.  The reference's value of a child is float32 expm1 of its model's output, and MCTS
sums the values, so their order alone does not fix a run.  The fixture's model outputs are exact
functions of the features or the token ids (MODELS: small dyadic rationals), and the fixture
stores, per scorer, a table from every output's bits to the bits of the reference's expm1 of it.
value_fn(name, table) looks the values up there -- a miss is an error -- so the yardstick and the
GPU tests see the reference's values bit for bit on any machine.  A scorer may also be a function
that returns the values themselves."""
import math

import numpy as np

from beam_yardstick import (BUDGET, EXHAUSTED, FOUND, MOVE_ERROR, NORM_MEAN, NORM_SCORERS, NORM_STD,  # noqa: F401
                            TOKEN_SCORERS, features_np, normalise_np)
from oracle import oracle as O

# name -> (numpy form, torch form) of a model's output on the (k, 14) features (0 total, 2 len_r2,
# 3 count_x_r1, 10 count_yinv_r2): small, so that expm1 stays small and the sums stay well inside
# the doubles
MODELS = {
    "M0": (lambda f: f[:, 0] / np.float32(16), lambda f: f[:, 0] / 16),
    "M1": (lambda f: (f[:, 2] + np.abs(f[:, 3] - f[:, 10])) / np.float32(8),
           lambda f: (f[:, 2] + (f[:, 3] - f[:, 10]).abs()) / 8),
    "MZ": (lambda f: f[:, 0] * np.float32(0), lambda f: f[:, 0] * 0),  # all-zero: every prior ties
    "MN": (lambda f: np.float32(-0.25) * f[:, 0], lambda f: -0.25 * f[:, 0]),  # negative: clamped to MZ's zeros
}
MODELS.update(NORM_SCORERS)
TOKEN_MODELS = {"TOK": TOKEN_SCORERS["TOK"]}


def model_np(name):
    return (TOKEN_MODELS if name in TOKEN_MODELS else MODELS)[name][0]


def model_t(name):
    return (TOKEN_MODELS if name in TOKEN_MODELS else MODELS)[name][1]


def value_fn(name, table):
    """the numpy scorer of a fixture record: the model's output, then the reference's expm1 of it
    from `table` ({output bits: expm1 bits}, keys as in the JSON: decimal strings)"""
    f = model_np(name)

    def values(x):
        m = np.asarray(f(x), np.float32)
        bits = m.view(np.uint32)
        out = np.array([table[str(int(b))] for b in bits], np.uint32)  # a miss is a KeyError
        return out.view(np.float32)
    return values


def value_fn_t(name, table, device):
    """the same scorer for the GPU tests: a torch function on `device`; a miss raises KeyError"""
    import torch
    f = model_t(name)
    keys = np.array(sorted(int(k) for k in table), np.int64)
    vals = np.array([table[str(int(k))] for k in keys], np.uint32).view(np.int32)
    keys_d = torch.from_numpy(keys).to(device)
    vals_d = torch.from_numpy(vals.copy()).to(device)

    def values(x):
        m = f(x).to(torch.float32).contiguous()
        bits = m.view(torch.int32).to(torch.int64) & 0xffffffff
        i = torch.searchsorted(keys_d, bits).clamp_(max=len(keys_d) - 1)
        if not bool((keys_d[i] == bits).all()):
            raise KeyError("a model output that the fixture's expm1 table does not hold")
        return vals_d[i].view(torch.float32)
    return values


def mcts(presentation, scorer, max_nodes, c_explore=1.41, cyclical=False, on_states=False, on_tokens=False, mean=None,
         std=None):
    """scorer: a function of the new children's (k, 14) features -- with on_states=True of their
    (k, 2L) states, with on_tokens=True of their (k, 2L) int64 token ids -- that returns k float32
    values (the reference's expm1 of its model's output; the clamp at 0 happens here).  With mean
    and std the features are normalised in float32 before the scorer, as the reference does.
    dict: status, ok, path ([] unless found), raises, nodes (len(visited) at the end), iterations,
    and the run's shape: dead_iters (iterations whose leaf had no new child), scored_iters, ucb_sel
    and unvisited_sel (selections of either kind), deepest (the deepest descent), ties (UCB
    selections whose best score another child had too), mingap (the smallest nonzero best-minus-
    second UCB score, relative to max(1, |best|); inf without one), twin_expansions (expansions that
    dropped a twin of an earlier child of their own), overshoot (nodes - budget on a budget ending),
    max_visit (the root's visit count at the end), max_log_n (the largest N whose log a UCB
    selection read; 0 without one), states (the nodes in id order), cands[i] (new
    nodes of scored iteration i) and cand_ids[i] (the first of them)."""
    assert (mean is None) == (std is None) and (mean is None or not (on_tokens or on_states))
    start = np.asarray(presentation, np.int32)
    L = len(start) // 2
    total = [int(np.count_nonzero(start))]
    parent, action, children = [None], [None], [[]]
    visit, vsum, prior = [1], [0.0], [0.0]  # (mcts.py:234; the root's own value is never read)
    states = [start]
    visited = {tuple(int(x) for x in start)}
    out = dict(status=None, ok=False, path=[], raises=False, dead_iters=0, scored_iters=0, ucb_sel=0, unvisited_sel=0,
               deepest=0, ties=0, mingap=math.inf, twin_expansions=0, overshoot=0, max_log_n=0, cands=[], cand_ids=[])
    iterations = 0

    def path_to(nid):
        p = []
        while parent[nid] is not None:
            p.append([action[nid], total[nid]])
            nid = parent[nid]
        return p[::-1]

    def backpropagate(nid, value):
        while nid is not None:
            visit[nid] += 1
            vsum[nid] += value
            nid = parent[nid]

    while len(visited) < max_nodes and iterations < 50 * max_nodes:
        iterations += 1
        # select
        node, depth = 0, 0
        while children[node] and total[node] != 2:
            unvisited = [c for c in children[node] if visit[c] == 0]
            if unvisited:
                node = min(unvisited, key=lambda c: prior[c])
                out["unvisited_sel"] += 1
            else:
                best_score, best_child, scores = -math.inf, None, []
                out["max_log_n"] = max(out["max_log_n"], visit[node])
                for c in children[node]:
                    exploitation = -(vsum[c] / visit[c])
                    exploration = c_explore * math.sqrt(math.log(visit[node]) / visit[c])
                    score = exploitation + exploration
                    scores.append(score)
                    if score > best_score:
                        best_score, best_child = score, c
                assert best_child is not None  # (the reference would crash on None)
                if len(scores) > 1:
                    second = sorted(scores)[-2]
                    if second == best_score:
                        out["ties"] += 1
                    else:
                        out["mingap"] = min(out["mingap"], (best_score - second) / max(1.0, abs(best_score)))
                node = best_child
                out["ucb_sel"] += 1
            depth += 1
        out["deepest"] = max(out["deepest"], depth)
        leaf = node
        if total[leaf] == 2:
            out.update(status=FOUND, ok=True, path=path_to(leaf))
            break
        # expand: all 12 moves are made before any child is judged
        ch, lens, err = O.expand12(states[leaf][None], L, cyclical)
        if err[0].any():  # ACMove raises (utils.py:264-266)
            out.update(status=MOVE_ERROR, raises=True)
            break
        new, twin = [], False
        for a in range(12):
            key = tuple(int(x) for x in ch[0, a])
            if key in visited:
                twin = twin or any(key == tuple(int(x) for x in states[n]) for n in new)
                continue
            visited.add(key)
            nid = len(states)
            states.append(ch[0, a].astype(np.int32))
            total.append(int(lens[0, a].sum()))
            parent.append(leaf)
            action.append(a)
            children.append([])
            visit.append(0)
            vsum.append(0.0)
            prior.append(math.inf)
            children[leaf].append(nid)
            new.append(nid)
        out["twin_expansions"] += twin
        if not new:
            out["dead_iters"] += 1
            backpropagate(leaf, prior[leaf] + 50)
            continue
        terminal = [n for n in new if total[n] == 2]
        if terminal:
            out.update(status=FOUND, ok=True, path=path_to(terminal[0]))
            break
        # evaluate
        cs = np.stack([states[n] for n in new])
        if on_tokens:
            x = cs.astype(np.int64) + 2
        elif on_states:
            x = cs
        else:
            x = features_np(cs, L)
            if mean is not None:
                x = normalise_np(x, mean, std)
        v = np.asarray(scorer(x), np.float32)
        assert v.shape == (len(new),) and not np.isnan(v).any() and not (v == np.inf).any()
        for n, vn in zip(new, v):
            prior[n] = float(max(vn, 0))
        out["scored_iters"] += 1
        out["cands"].append(len(new))
        out["cand_ids"].append(new[0])
        best = min(new, key=lambda n: prior[n])
        backpropagate(leaf, prior[best])
    if out["status"] is None:
        out["status"] = BUDGET if len(visited) >= max_nodes else EXHAUSTED
    if out["status"] == BUDGET:
        out["overshoot"] = len(visited) - max(int(max_nodes), 1)
    out.update(nodes=len(visited), iterations=iterations, states=states, max_visit=visit[0])
    return out


def result(y):
    """what a fixture record holds"""
    if y["raises"]:
        return (True, False, [], None, None)
    return (False, y["ok"], y["path"], y["nodes"], y["iterations"])
