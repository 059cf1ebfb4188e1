"""What the tests of the two batched searches (acx.bfs_many: test_gpu_bfs_many.py,
test_search_many_cpu.py; acx.greedy_search_many: test_gpu_greedy_many.py, test_greedy_many_cpu.py)
share: the fixture reader, the comparison of a call's results with the reference's records and
with another call's, and the rows they search."""
import json
import os

import numpy as np

from conftest import GOLDEN

EXHAUSTED, FOUND, BUDGET = 0, 1, 2  # ACX_BFS_* of include/acx.h, as in both yardsticks
AK2 = [1, 1, -2, -2, -2, 0, 0, 1, 2, 1, -2, -1, -2, 0]


def _load(name):
    with open(os.path.join(GOLDEN, name)) as f:
        return json.load(f)


def _norm(r):
    return None if r is None else [bool(r[0]), None if r[1] is None else [list(x) for x in r[1]]]


def _check_records(recs, res, st, nodes_key="nodes"):
    for i, c in enumerate(recs):
        assert res[i] == [c["ok"], c["path"]], (i, c)
        if c[nodes_key] is not None:
            assert st["status"][i] == BUDGET and st["nodes"][i] == c[nodes_key], (i, c)
        else:
            assert st["status"][i] == (FOUND if c["ok"] else EXHAUSTED), (i, c)


def _same(a, b):
    return a[0] == b[0] and all(np.array_equal(a[1][k], b[1][k]) for k in a[1])


def _dataset_rows():
    import acx
    rows = acx.data.load_initial_states("all")[::5].astype(np.int32)
    assert rows.shape == (238, 36)
    return rows


def _scrambled(L, rng, k):
    """a trivial presentation after k oracle moves (no cyclic reduction), none leading back"""
    from oracle import oracle as O
    s = np.zeros(2 * L, np.int32)
    s[0], s[L] = [(1, 2), (-2, 1), (2, -1), (-1, -2)][int(rng.integers(4))]
    seen = {s.tobytes()}
    for _ in range(k):
        for _ in range(100):
            out, _, err = O.move_batch(s[None], np.array([rng.integers(12)], np.int32), L, False)
            if err[0] == 0 and out[0].tobytes() not in seen:
                s = out[0].astype(np.int32)
                seen.add(s.tobytes())
                break
    return s
