"""CPU side of the batched greedy search (acx.greedy_search_many): the yardstick its GPU tests rest
on (tests/greedy_yardstick.py, the reference's greedy_search restated over the oracle's expansion)
reproduces the reference's own recorded runs -- tests/golden/greedy_many.json
(make_greedy_many_golden.py), the greedy records of kat_search_extra.json and AK(2) of
kat_search.json; the frontier order the kernel uses (csrc/acx_prio.h) is the host engines'
priority-key order and the definition (tests/prio_check.cpp, built with the host compiler); the
argument checks are made before any GPU call."""
import os
import subprocess

import numpy as np
import pytest
import torch

from conftest import PKG_ROOT, REPO

import greedy_yardstick as Y
import many_common
from many_common import _load

AK2 = np.array(many_common.AK2)


def _check(c):
    r = Y.greedy(np.array(c["presentation"]), c["budget"], c["cyclical"])
    assert r["raises"] == c["raises"], c
    if c["raises"]:
        assert r["status"] == Y.MOVE_ERROR and r["path"] is None
        return r
    assert r["ok"] == c["ok"], c
    assert [list(x) for x in r["path"]] == c["path"], c
    nodes = c["nodes"] if "nodes" in c else c["budget_nodes"]
    assert (r["nodes"] if r["status"] == Y.BUDGET else None) == nodes, c
    return r


def test_yardstick_reproduces_the_dataset_records():
    many = _load("greedy_many.json")
    assert many["L"] == 18 and len(many["dataset"]) == 238
    got = [_check(c) for c in many["dataset"]]
    assert all(c["budget"] == 2000 and not c["cyclical"] for c in many["dataset"])
    assert sum(r["status"] == Y.FOUND and len(r["path"]) >= 4 for r in got) >= 30
    assert sum(r["status"] == Y.BUDGET for r in got) >= 60


def test_yardstick_reproduces_the_solvable_records():
    recs = _load("greedy_many.json")["solvable"]
    got = [_check(c) for c in recs]
    assert {c["budget"] for c in recs} == {50, 1000, 30000}
    for cyc in (False, True):  # the fixture is not vacuous for either flag
        part = [r for c, r in zip(recs, got) if c["cyclical"] == cyc]
        assert any(r["status"] == Y.FOUND for r in part)
        assert any(r["status"] in (Y.BUDGET, Y.EXHAUSTED) for r in part)


def test_yardstick_reproduces_the_random_reference_searches():
    cases = [c for c in _load("kat_search_extra.json") if c["search_fn"] == "greedy_search"]
    assert len(cases) == 120 and sum(c["raises"] for c in cases) == 70
    got = [_check(c) for c in cases]
    assert sum(r["status"] == Y.EXHAUSTED for r in got) == 8


def test_yardstick_reproduces_ak2():
    kat = _load("kat_search.json")
    for key, budget in [("greedy_ak2", 10 ** 6), ("greedy_ak2_budget10", 10)]:
        r = Y.greedy(AK2, budget)
        assert [r["ok"], [list(x) for x in r["path"]]] == kat[key]


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("prio") / "prio_check")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-I", os.path.join(REPO, "include"), "-I",
                           os.path.join(PKG_ROOT, "csrc"), os.path.join(REPO, "tests", "prio_check.cpp"), "-o", exe])
    return exe


@pytest.mark.parametrize("seed", [1, 2])
def test_frontier_order_on_packed_keys(checker, seed):
    """csrc/acx_prio.h against prio_key's word order and the tuple order, random and planted pairs
    at L in {1, 16, 17, 32, 33, 40, 41, 64, 65, 127, 128}"""
    r = subprocess.run([checker, str(seed)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.startswith("ok"), r.stdout[-2000:]


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
def test_greedy_search_many_refuses_bad_presentations_without_a_gpu(bad, msg):
    import acx
    with pytest.raises(ValueError, match=msg):
        acx.greedy_search_many(bad, 10)


def test_greedy_search_many_refuses_bad_budgets_and_options_without_a_gpu():
    import acx
    from acx.search import greedy_search_many
    assert greedy_search_many is acx.greedy_search_many
    assert "greedy_search_many" in acx.__all__ and "greedy_search_many" in acx.search.__all__
    with pytest.raises(ValueError, match="sequence of 2"):
        acx.greedy_search_many(GOOD, [10, 20, 30])
    with pytest.raises(ValueError, match="sequence of 2"):
        acx.greedy_search_many(GOOD, [[10, 20]])
    with pytest.raises(ValueError, match="greedy_search_many supports at most 2\\^24"):
        acx.greedy_search_many(GOOD, [10, (1 << 24) + 1])
    with pytest.raises(ValueError, match="bfs_many supports at most 2\\^24"):  # bfs_many's message is its own
        acx.bfs_many(GOOD, [10, (1 << 24) + 1])
    with pytest.raises(ValueError, match="on_error"):
        acx.greedy_search_many(GOOD, 10, on_error="ignore")
    with pytest.raises(ValueError, match="equal length"):
        acx.greedy_search_many(torch.zeros(4, dtype=torch.int32), 10)
    with pytest.raises(ValueError, match=f"exceeds {acx._lib.MAX_L}"):
        acx.greedy_search_many(np.ones((1, 2 * (acx._lib.MAX_L + 1)), np.int64), 10)
    assert acx.greedy_search_many(np.zeros((0, 8), np.int32), 10) == []  # nothing to search: no GPU call either
    res, stats = acx.greedy_search_many(np.zeros((0, 8), np.int32), 10, return_stats=True)
    assert res == [] and sorted(stats) == ["min_length", "nodes", "parents", "status"]


def test_mgreedy_workspace_formula_and_argument_checks():
    """acx_mgreedy_bytes states the bytes per search of include/acx.h and DESIGN.md "Batched
    greedy"; create / run / paths refuse bad arguments before any GPU call."""
    from acx import _lib
    lib = _lib.load()
    for L, B in [(1, 1), (12, 50), (18, 2000), (18, 10_000), (64, 777), (65, 777), (128, 3000), (18, 1 << 24)]:
        kw = _lib.key_words(L)
        want = (8 * kw + 20) * (B + 11) + 64 * ((B + 23 + 3) // 4) + 32
        assert lib.acx_mgreedy_bytes(L, B) == want, (L, B)
    assert lib.acx_mgreedy_bytes(0, 10) < 0 and lib.acx_mgreedy_bytes(129, 10) < 0
    assert lib.acx_mgreedy_bytes(18, 0) < 0 and lib.acx_mgreedy_bytes(18, (1 << 24) + 1) < 0
    for L, n, B in [(0, 1, 10), (129, 1, 10), (18, 0, 10), (18, 1, 0), (18, 1, (1 << 24) + 1), (18, -1, 10)]:
        assert not lib.acx_mgreedy_create(L, n, B, 0)
    lib.acx_mgreedy_destroy(None)
    assert lib.acx_mgreedy_run(None, None, None, 1, None, None, None, None, None, None) == _lib.E_ARG
    assert lib.acx_mgreedy_paths(None, 1, None, None, None, 0, None) == _lib.E_ARG
