"""The reference's value_guided_greedy_search (value_search/value_guided_search.py:294-414,
solution_cache=None, time_limit=None) restated literally over the CPU oracle's 12-way expansion
(oracle.expand12), with Python's own heapq on (score, path_length, node_id): the yardstick of the
batched value-guided greedy tests.  tests/test_vgreedy_cpu.py checks it against the reference's own
recorded runs (tests/golden/vgreedy_search.json).

Literal means twins included: two actions of one pop that yield the same new state are both given a
node id and both pushed, because the reference tests the children against state_to_id as it stood
before the pop.  drop_twins=True is the engine's variant (csrc/acx_vgreedy.hip): the first is kept,
the later ones are dropped; test_vgreedy_cpu.py asserts that both give the same (solved, path,
nodes, min_length).  The root is not scored here either: it is the only heap entry when it is
popped, so its priority decides nothing.

The scorers are beam_yardstick's: exact functions of the features (SCORERS, the normalised ones
among them) and of the token ids (TOKEN_SCORERS)."""
import heapq

import numpy as np

from beam_yardstick import (BUDGET, EXHAUSTED, FOUND, MOVE_ERROR, NORM_MEAN, NORM_SCORERS, NORM_STD,  # noqa: F401
                            SCORERS, TOKEN_SCORERS, features_np, normalise_np)
from oracle import oracle as O


def heap_level(n):
    """the level (0 .. 3) of entry n - 1 of the engine's implicit heap of fan-out 64: levels hold 1,
    64, 4,096 and 262,144 entries"""
    return 0 if n <= 1 else 1 if n <= 65 else 2 if n <= 4161 else 3


def _xy_power(k, L):
    """r1 = (xy)^k, r2 = x: x^-1 r1 x = y r1 y^-1, so two actions of the root's pop give one state"""
    s = np.zeros(2 * L, np.int32)
    s[:2 * k], s[L] = [1, 2] * k, 1
    return s


def twin_cases():
    """(presentation, scorer, budget, cyclical) whose searches hold a pop with two equal new children"""
    return [(_xy_power(k, L), s, b, cyc) for k, L in ((2, 6), (3, 9), (4, 18)) for s in ("S0", "S2", "S3", "TOK")
            for b, cyc in ((60, False), (500, True))]


def vgreedy(presentation, scorer, max_nodes, cyclical=False, on_states=False, mean=None, std=None, drop_twins=False):
    """scorer: a name of SCORERS or TOKEN_SCORERS, or a function of the candidates' (k, 14) features
    -- with on_states=True of their (k, 2L) states -- that returns k float32 scores.  With mean and
    std the features are normalised in float32 before the scorer, as the reference does.
    dict: status, ok, path ([] unless found), raises, nodes (len(state_to_id) at the ending event),
    min_length, steps (pops), parents = steps, states (the nodes in node_id order, twins included
    unless dropped), and the search's shape: cands[i] = candidates of pop i + 1 and nodes_after[i] =
    node ids handed out after it, twin_pops (pops, 1-based, in which two actions gave the same new
    state), empty_pops (pops without a new child after which the search went on: M == 0 and live),
    id_ties (pops whose entry tied with the heap's next on score and depth: the id decided), peak
    (the most heap entries -- the push of a pop that ends on its budget included, which the engine
    never carries out: it applies the verdict first), and what the engine's heap really holds:
    max_popped (the largest heap a pop took its entry from), level_pops[k] (pops from a heap whose
    last entry lay in level k of the fan-out-64 heap: 1, 2 .. 65, 66 .. 4,161, more entries) and
    level_pushes[k] (pushes after which the search went on, by the level of the last new leaf),
    overshoot (nodes - budget on a budget ending), min_dup (the final
    min_length was also the total of a child that failed the visited test -- see make_golden_vgreedy.py)
    and score_bits (the bit patterns of every score returned)."""
    on_tokens = isinstance(scorer, str) and scorer in TOKEN_SCORERS
    score = (TOKEN_SCORERS if on_tokens else SCORERS)[scorer][0] if isinstance(scorer, str) else scorer
    assert (mean is None) == (std is None) and (mean is None or not (on_tokens or on_states))
    start = np.asarray(presentation, np.int32)
    L = len(start) // 2
    root = tuple(int(x) for x in start)
    total0 = int(np.count_nonzero(start))
    parent = {0: (None, total0, None)}
    state_to_id = {root: 0}
    next_id = 1
    heap = [(0.0, 0, 0, root)]
    min_length, dup_totals = total0, set()
    out = dict(status=None, ok=False, path=[], raises=False, states=[start], cands=[], nodes_after=[], twin_pops=[],
               empty_pops=[], id_ties=0, peak=1, max_popped=0, level_pops=[0, 0, 0, 0], level_pushes=[0, 0, 0, 0],
               overshoot=0, score_bits=set())
    pops = 0

    def path_to(nid):
        p = []
        while parent[nid][2] is not None:
            a, t, nid2 = parent[nid]
            p.append([a, t])
            nid = nid2
        return p[::-1]

    while heap and out["status"] is None:
        out["max_popped"] = max(out["max_popped"], len(heap))
        out["level_pops"][heap_level(len(heap))] += 1
        s0, plen, cur, st = heapq.heappop(heap)
        pops += 1
        if heap and (heap[0][0], heap[0][1]) == (s0, plen):
            out["id_ties"] += 1
        ch, lens, err = O.expand12(np.array(st, np.int32)[None], L, cyclical)
        children, in_pop = [], set()
        for a in range(12):
            if err[0, a]:  # ACMove raises (utils.py:264-266)
                out.update(status=MOVE_ERROR, raises=True)
                break
            t = int(lens[0, a].sum())
            key = tuple(int(x) for x in ch[0, a])
            min_length = min(min_length, t)
            if t == 2:
                out.update(status=FOUND, ok=True, path=path_to(cur) + [[a, t]])
                break
            if key in state_to_id:
                dup_totals.add(t)
                continue
            if key in in_pop:
                if out["twin_pops"][-1:] != [pops]:
                    out["twin_pops"].append(pops)
                if drop_twins:
                    continue
            in_pop.add(key)
            children.append((ch[0, a].astype(np.int32), a, t, key))
        if out["status"] is not None:
            break
        out["cands"].append(len(children))
        if children:
            cs = np.stack([c[0] for c in children])
            if on_tokens:
                x = cs.astype(np.int64) + 2
            elif on_states:
                x = cs
            else:
                x = features_np(cs, L)
                if mean is not None:
                    x = normalise_np(x, mean, std)
            s = np.asarray(score(x), np.float32)
            assert s.shape == (len(children),) and not np.isnan(s).any()
            out["score_bits"].update(np.unique(s.view(np.uint32)).tolist())
            for (state, a, t, key), sc in zip(children, s):
                nid = next_id
                next_id += 1
                parent[nid] = (a, t, cur)
                state_to_id[key] = nid
                out["states"].append(state)
                heapq.heappush(heap, (float(sc), plen + 1, nid, key))
        out["nodes_after"].append(next_id)
        out["peak"] = max(out["peak"], len(heap))
        if len(state_to_id) >= max_nodes:
            out.update(status=BUDGET, overshoot=len(state_to_id) - max(int(max_nodes), 1))
            break
        if children:
            out["level_pushes"][heap_level(len(heap))] += 1
        if not children and heap:
            out["empty_pops"].append(pops)
    if out["status"] is None:
        out["status"] = EXHAUSTED
    out.update(nodes=len(state_to_id), min_length=min_length, steps=pops, parents=pops, min_dup=min_length in dup_totals)
    return out


def result(y):
    """what the two variants must agree on, and what a fixture record holds"""
    return (y["raises"], y["ok"], y["path"], None if y["raises"] else y["nodes"], None if y["raises"] else y["min_length"])
