"""CPU side of the batched BFS (acx.bfs_many): its argument checks are made before any GPU call, and
the yardstick its GPU tests rest on (tests/bfs_yardstick.py, the reference's bfs restated over the
oracle's expansion) reproduces the reference's own recorded runs -- tests/golden/search_many.json
(make_search_many_golden.py) and the BFS records of kat_search_extra.json."""
import numpy as np
import pytest
import torch

import bfs_yardstick as Y
from many_common import _load


def _check(c):
    r = Y.bfs(np.array(c["presentation"]), c["budget"], c["cyclical"])
    assert r["raises"] == c["raises"], c
    if c["raises"]:
        return r
    assert r["ok"] == c["ok"], c
    assert (None if r["path"] is None else [list(x) for x in r["path"]]) == c["path"], c
    nodes = c["nodes"] if "nodes" in c else c["budget_nodes"]
    assert (r["nodes"] if r["status"] == Y.BUDGET else None) == nodes, c
    return r


def test_yardstick_reproduces_the_dataset_records():
    many = _load("search_many.json")
    assert many["L"] == 18 and len(many["dataset"]) == 238 and many["dataset"][0]["nodes"] == 3007
    for c in many["dataset"]:
        assert _check(c)["status"] == Y.BUDGET


def test_yardstick_reproduces_the_solvable_records():
    recs = _load("search_many.json")["solvable"]
    got = [_check(c) for c in recs]
    for cyc in (False, True):  # the fixture is not vacuous for either flag
        part = [r for c, r in zip(recs, got) if c["cyclical"] == cyc]
        assert any(r["status"] == Y.FOUND and len(r["path"]) >= 4 for r in part)
        assert any(r["status"] == Y.BUDGET for r in part)
    assert sum(r["status"] == Y.FOUND and len(r["path"]) >= 4 for r in got) >= 20
    assert sum(r["status"] == Y.BUDGET for r in got) >= 10


def test_yardstick_reproduces_the_random_reference_searches():
    cases = [c for c in _load("kat_search_extra.json") if c["search_fn"] == "bfs"]
    assert len(cases) == 120 and sum(c["raises"] for c in cases) == 14
    for c in cases:
        _check(c)


def test_yardstick_rounds():
    assert Y.rounds([13, 20, 30]) == [(0, 1), (1, 2)]
    after = [13] + list(range(25, 25 + 12 * 10, 10)) + [400] * 200
    rs = Y.rounds(after)
    assert rs[:4] == [(0, 1), (1, 12), (13, 64), (77, 64)] and Y.round_of(rs, 76) == 2 and Y.round_of(rs, 77) == 3


GOOD = np.array([[1, 2, 0, -2, 0, 0], [2, 0, 0, 1, 1, 0]])


@pytest.mark.parametrize("bad,msg", [
    ([[1, 0, 2, 0], [1, 2, 0, 2, 0, 0]], "equal length"),                      # ragged rows
    (np.array([1, 0, 2, 0]), "equal length"),                                  # one row, not a batch
    (np.array([[1, 0, 2], [1, 0, 2]]), "even"),                                # odd row length
    (np.array([[1, 0, 2, 0], [0, 1, 2, 0]]), "not a valid presentation"),      # zero before a letter
    (np.array([[1, 0, 2, 0], [1, 1, 0, 0]]), "not a valid presentation"),      # empty relator
    (np.array([[1, 0, 2, 0], [3, 0, 2, 0]]), r"letters \+-1 \(x\) and \+-2 \(y\) only"),
    (np.array([[1.0, 0, 2, 0]]), "integer"),
])
def test_bfs_many_refuses_bad_presentations_without_a_gpu(bad, msg):
    import acx
    with pytest.raises(ValueError, match=msg):
        acx.bfs_many(bad, 10)


def test_bfs_many_refuses_bad_budgets_and_options_without_a_gpu():
    import acx
    from acx.search import bfs_many
    assert bfs_many is acx.bfs_many
    with pytest.raises(ValueError, match="sequence of 2"):
        acx.bfs_many(GOOD, [10, 20, 30])
    with pytest.raises(ValueError, match="sequence of 2"):
        acx.bfs_many(GOOD, [[10, 20]])
    with pytest.raises(ValueError, match="2\\^24"):
        acx.bfs_many(GOOD, [10, (1 << 24) + 1])
    with pytest.raises(ValueError, match="on_error"):
        acx.bfs_many(GOOD, 10, on_error="ignore")
    with pytest.raises(ValueError, match="equal length"):
        acx.bfs_many(torch.zeros(4, dtype=torch.int32), 10)
    with pytest.raises(ValueError, match=f"exceeds {acx._lib.MAX_L}"):
        acx.bfs_many(np.ones((1, 2 * (acx._lib.MAX_L + 1)), np.int64), 10)
    assert acx.bfs_many(np.zeros((0, 8), np.int32), 10) == []  # nothing to search: no GPU call either


def test_mbfs_workspace_formula_and_argument_checks():
    """acx_mbfs_bytes states the bytes per search of include/acx.h and DESIGN.md "Batched BFS";
    create / run / paths refuse bad arguments before any GPU call."""
    from acx import _lib
    lib = _lib.load()
    for L, B in [(1, 1), (12, 50), (18, 3000), (18, 10_000), (64, 777), (65, 777), (128, 3000)]:
        kw = _lib.key_words(L)
        want = 8 * kw * B + 4 * B + 64 * ((B + 779 + 3) // 4) + 32 + (6144 * kw if L > 64 else 0)
        assert lib.acx_mbfs_bytes(L, B) == want, (L, B)
    assert lib.acx_mbfs_bytes(0, 10) < 0 and lib.acx_mbfs_bytes(129, 10) < 0
    assert lib.acx_mbfs_bytes(18, 0) < 0 and lib.acx_mbfs_bytes(18, (1 << 24) + 1) < 0
    for L, n, B in [(0, 1, 10), (129, 1, 10), (18, 0, 10), (18, 1, 0), (18, 1, (1 << 24) + 1), (18, -1, 10)]:
        assert not lib.acx_mbfs_create(L, n, B, 0)
    lib.acx_mbfs_destroy(None)
    assert lib.acx_mbfs_run(None, None, None, 1, None, None, None, None, None, None) == _lib.E_ARG
    assert lib.acx_mbfs_paths(None, 1, None, None, None, 0, None) == _lib.E_ARG
