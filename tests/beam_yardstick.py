"""The reference's beam_search (value_search/value_guided_search.py:417-561, solution_cache=None,
time_limit=None) restated over the CPU oracle's 12-way expansion (oracle.expand12), with Python's
own stable sort on the scores: the yardstick of the batched beam tests.  tests/test_beam_cpu.py
checks it against the reference's own recorded runs (tests/golden/beam_search.json).

The scorers are functions of the 14 raw features whose float32 values are exact (small integers
and quarters), so they give the same scores here, in the reference on the CPU and on the GPU; each
is stated once for numpy and once for torch."""
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


def beam(presentation, scorer, width, max_nodes, cyclical=False, on_states=False):
    """scorer: a name of SCORERS, or a function of the candidates' (k, 14) features -- with
    on_states=True of their (k, 2L) states -- that returns k float32 scores.
    dict: status, ok, path ([] unless found), raises, nodes (total_nodes at the ending event),
    steps (steps begun), states (the nodes in node_id order), and the search's shape per step: cands[i] = candidates of step i + 1,
    nodes_after[i] = total_nodes after its expansion, and the steps (1-based) at which dup_steps: a
    child equalled an earlier new child of the same step, cut_mid: the budget cut fell before the
    last child of the step, cut_at: (step, action of the cut child, children of the step not looked
    at), tie_steps: the scores of the last selected and the first rejected candidate tied."""
    score = SCORERS[scorer][0] if isinstance(scorer, str) else scorer
    start = np.asarray(presentation, np.int32)
    L = len(start) // 2
    root = tuple(int(x) for x in start)
    visited = {root}
    parent = {0: (None, int(np.count_nonzero(start)), None)}
    beam_ = [(start, 0)]
    total_nodes, step = 1, 0
    out = dict(status=None, ok=False, path=[], raises=False, states=[start], cands=[], nodes_after=[], dup_steps=[],
               cut_mid=[], cut_at=[], tie_steps=[])

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
        s = np.asarray(score(cs if on_states else features_np(cs, L)), np.float32)
        assert s.shape == (len(new),) and not np.isnan(s).any()
        order = sorted(range(len(new)), key=lambda i: float(s[i]))
        if len(new) > width and float(s[order[width - 1]]) == float(s[order[width]]):
            out["tie_steps"].append(step)
        beam_ = [new[i] for i in order[:width]]
    if out["status"] is None:  # the loop condition: total_nodes >= max_nodes (a budget <= 1 runs no step)
        out["status"] = BUDGET
    out.update(nodes=total_nodes, steps=step)
    return out
