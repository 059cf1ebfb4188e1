"""GPU: the five unscored search engines and the host engine at every relator length where their
key-word instantiation (bfs::by_nw: NW = 1, 2, 3, 4, 8) or the key's layout changes, from starts
whose searches turn on the top key word of a relator's tile (tests/search_edge_common.py: EDGE_L,
the power and near-full starts, their budgets; tests/test_search_edge_cpu.py checks on the CPU that
the starts do what is said of them).  Every expected value is the yardsticks'
(tests/bfs_yardstick.py, tests/greedy_yardstick.py).

One test per engine, parametrised by (L, cyclical): the ids show which engine ran at which length.
The device BFS runs at chunk 0, 3 and 64, the sharded BFS at one rank and chunk 3; the batched
engines take all starts and budgets of one (L, cyclical) in a single call each.  The weak-hash
library and the sharded BFS at two ranks take the near-full starts of L = 49 and 64 in
tests/test_gpu_weak_hash.py::test_edge_lengths and tests/test_gpu_sbfs.py::test_sharded_bfs_multi_rank.

Measured on an MI355X (--durations): the slowest case, test_device_bfs[12-False] with the
process's first workspace, takes 0.26 s, every other one at most 0.10 s (the device BFS at L >= 124
with cyclic reduction); the 360 cases together 10.4 s, the yardsticks' runs included.  No budget or
chunk had to be lowered."""
import contextlib
import io

import numpy as np
import pytest
import torch

import search_edge_common as SE
from bfs_yardstick import BUDGET, FOUND, MOVE_ERROR
from conftest import unpack_keys_np

pytestmark = [pytest.mark.gpu, pytest.mark.filterwarnings("ignore:The given NumPy array is not writable")]

DEV = torch.device("cuda:0")
CHUNKS = (0, 3, 64)


def _call(fn):
    """fn()'s result as search_edge_common.want_result gives it; the lines it prints swallowed"""
    with contextlib.redirect_stdout(io.StringIO()):
        try:
            ok, path = fn()
        except AssertionError:
            return "raises"
    return bool(ok), None if path is None else [tuple(x) for x in path]


def _states(keys, L):
    return unpack_keys_np(keys, L).astype(np.int32)


def _runs(L, cyc, engine):
    for name, case in SE.cases(L, cyc).items():
        for budget, y in case[engine]:
            yield (L, cyc, name, budget), case["start"], budget, y


def _check_bfs(tag, got, st, keys, y, L):
    """a one-search BFS engine's result, its statistics and its stored keys against the yardstick's
    run y: the keys, unpacked, are the yardstick's states node for node, in order"""
    assert got == SE.want_result(y), tag
    assert (st["status"], st["parents"], st["min_length"]) == (y["status"], y["parents"], y["min_length"]), tag
    n = y["nodes"]
    if y["status"] == BUDGET:
        assert st["nodes"] == n, tag
    assert len(keys) >= n and np.array_equal(_states(keys[:n], L), y["states"]), tag


@pytest.mark.parametrize("L,cyc", SE.CASES)
def test_device_bfs(L, cyc):
    from acx.search import _device_bfs as D
    for tag, start, budget, y in _runs(L, cyc, "bfs"):
        for chunk in CHUNKS:
            got = _call(lambda: D.device_bfs(start, budget, cyclically_reduce_after_moves=cyc, device=DEV, chunk=chunk,
                                             keep_node_keys=True))
            _check_bfs(tag + (chunk,), got, D.LAST_STATS, D.LAST_STATS["node_keys"], y, L)
    D.release_workspaces()


@pytest.mark.parametrize("L,cyc", SE.CASES)
def test_sharded_bfs_one_rank(L, cyc):
    from acx.search import _sharded_bfs as S
    for tag, start, budget, y in _runs(L, cyc, "bfs"):
        got = _call(lambda: S.sharded_bfs(start, budget, cyclically_reduce_after_moves=cyc, device=DEV, chunk=3,
                                          keep_node_keys=True))
        st = S.LAST_STATS
        _check_bfs(tag, got, st, st["node_keys"], y, L)
        assert np.array_equal(st["node_ids"][:y["nodes"]], np.arange(y["nodes"])), tag
    S.release_workspaces()


def _engine_status(y):
    """acx_search_status / acx_greedy_status: 1 success, 2 failed, 3 move error"""
    return {FOUND: 1, MOVE_ERROR: 3}.get(y["status"], 2)


def _check_engine(tag, got, st, y):
    assert got == SE.want_result(y), tag
    assert (st["status"], st["min_length"]) == (_engine_status(y), y["min_length"]), tag
    if y["status"] == BUDGET:
        assert st["nodes"] == y["nodes"], tag


def _check_pops(tag, st, y, L):
    """the states of the engine's popped nodes are the yardstick's pops, in order"""
    pops = _states(st["node_keys"][st["popped"]], L)
    assert np.array_equal(pops, np.array(y["pops"], np.int32).reshape(-1, 2 * L)), tag


@pytest.mark.parametrize("L,cyc", SE.CASES)
def test_host_engine(L, cyc):
    """csrc/acx_search.cpp over acx_expand12's keys: BFS stores the yardstick's states in order;
    greedy stores the yardstick's set of states and pops the yardstick's pops"""
    from acx.search import _engine as E
    for tag, start, budget, y in _runs(L, cyc, "bfs"):
        got = _call(lambda: E.run_search(E.BFS, start, budget, False, cyc, device=DEV, batch=256, keep_node_keys=True))
        st = E.LAST_STATS
        if got != "raises" and not got[0]:  # (a failed search: the engine's path is the reader's, the reference returns None)
            got = (False, None)
        _check_engine(tag, got, st, y)
        assert st["nodes"] >= y["nodes"] and np.array_equal(_states(st["node_keys"][:y["nodes"]], L), y["states"]), tag
    for tag, start, budget, y in _runs(L, cyc, "greedy"):
        got = _call(lambda: E.run_search(E.GREEDY, start, budget, False, cyc, device=DEV, keep_node_keys=True,
                                         engine="host"))
        st = E.LAST_STATS
        _check_engine(tag, got, st, y)
        stored = {tuple(r) for r in _states(st["node_keys"], L).tolist()}
        assert len(stored) == len(st["node_keys"]) and stored == set(y["stored"]), tag
        _check_pops(tag, st, y, L)


@pytest.mark.parametrize("L,cyc", SE.CASES)
def test_device_greedy(L, cyc):
    """csrc/acx_greedy.hip: the result, and pop for pop the yardstick's states"""
    from acx.search import _engine as E
    for tag, start, budget, y in _runs(L, cyc, "greedy"):
        got = _call(lambda: E.run_search(E.GREEDY, start, budget, False, cyc, device=DEV, keep_node_keys=True,
                                         engine="device"))
        st = E.LAST_STATS
        _check_engine(tag, got, st, y)
        _check_pops(tag, st, y, L)


def _check_many(fn, L, cyc, engine):
    runs = list(_runs(L, cyc, engine))
    res, st = fn(np.stack([s for _, s, _, _ in runs]), [b for _, _, b, _ in runs], cyclically_reduce_after_moves=cyc,
                 device=DEV, return_stats=True, on_error="return")
    assert len(res) == len(runs) and all(len(v) == len(runs) for v in st.values())
    for i, (tag, _, _, y) in enumerate(runs):
        got = "raises" if res[i] is None else (bool(res[i][0]), None if res[i][1] is None else [tuple(x) for x in res[i][1]])
        assert got == SE.want_result(y), tag
        assert (st["status"][i], st["nodes"][i], st["parents"][i], st["min_length"][i]) == \
            (y["status"], y["nodes"], y["parents"], y["min_length"]), tag


@pytest.mark.parametrize("L,cyc", SE.CASES)
def test_bfs_many(L, cyc):
    import acx
    _check_many(acx.bfs_many, L, cyc, "bfs")


@pytest.mark.parametrize("L,cyc", SE.CASES)
def test_greedy_many(L, cyc):
    import acx
    _check_many(acx.greedy_search_many, L, cyc, "greedy")
