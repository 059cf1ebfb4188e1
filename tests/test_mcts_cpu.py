"""CPU side of the batched MCTS (acx.mcts_search_many, acx.mcts_search): the yardstick its GPU tests
rest on (tests/mcts_yardstick.py, the reference's mcts_search restated literally over the oracle's
expansion, with the reference's own expm1 values looked up in the fixture's tables) reproduces the
reference's own recorded runs -- tests/golden/mcts_search.json (make_golden_mcts.py); the argument
checks are made before any GPU call."""
import math

import numpy as np
import pytest
import torch

import mcts_yardstick as Y
from many_common import _load


def _end(r):
    if r["raises"]:
        return "raises"
    if r["ok"]:
        return "found"
    return "budget" if r["nodes_explored"] >= max(r["budget"], 1) else "exhausted"


def run_record(c, tables, **kw):
    norm = dict(mean=Y.NORM_MEAN, std=Y.NORM_STD) if c["norm"] else {}
    return Y.mcts(np.array(c["presentation"]), Y.value_fn(c["scorer"], tables[c["scorer"]]), c["budget"], c["c"],
                  c["cyclical"], on_tokens=c["arch"] != "mlp", **norm, **kw)


@pytest.fixture(scope="module")
def runs():
    """(record, the yardstick's run) for every record"""
    fx = _load("mcts_search.json")
    return [(c, run_record(c, fx["tables"])) for c in fx["records"]]


def test_yardstick_reproduces_every_reference_record(runs):
    """(solved, path, nodes_explored, iterations), and the ending's status"""
    for c, y in runs:
        assert Y.result(y) == (c["raises"], c["ok"], c["path"] or [], c["nodes_explored"], c["iterations"]), c
        want = {"found": Y.FOUND, "budget": Y.BUDGET, "exhausted": Y.EXHAUSTED, "raises": Y.MOVE_ERROR}[_end(c)]
        assert y["status"] == want, c
        assert c["mingap"] == (None if y["mingap"] == math.inf else y["mingap"]), c


def test_the_fixture_covers_what_it_is_for(runs):
    recs = [c for c, _ in runs]
    by = {}
    for r in recs:
        by.setdefault(r["name"].split("-")[0], []).append(r)
    assert {_end(r) for r in recs} == {"found", "budget", "exhausted", "raises"}
    assert {(r["L"], r["cyclical"], r["budget"]) for r in by["ak"]} == {
        (L, c, b) for L in (7, 18) for c in (False, True) for b in (0, 1, 2, 37, 500, 3000)}
    assert {r["scorer"] for r in by["ak"]} == {"M0", "M1", "MZ", "MN"}
    # a budget of 0 or 1 runs no iteration, even for a trivial root
    for r in recs:
        if r["budget"] <= 1 and not r["raises"]:
            assert (r["ok"], r["path"], r["nodes_explored"], r["iterations"]) == (False, [], 1, 0), r
    trivial = [r for r in by["roots"] if r["name"] == "roots-trivial"]
    assert {(r["budget"] > 1, r["ok"]) for r in trivial} == {(True, True), (False, False)}
    assert all(r["path"] == [] and r["nodes_explored"] == 1 for r in trivial)
    spins = [r for r in by["roots"] if r["name"] == "roots-spins"]
    assert sorted((r["budget"], r["iterations"], r["nodes_explored"]) for r in spins) == [(20, 1000, 1), (32, 1600, 1)]
    assert len(by["ms"]) == 20 and all(r["L"] == 36 for r in by["ms"]) and max(r["budget"] for r in by["ms"]) == 1000
    # (a row on which bfs meets a raising move: MCTS need not reach that move within its budget)
    assert sum(r["raises"] for r in by["raise"]) >= 3 and not any(r["raises"] for r in recs if r not in by["raise"])
    assert {(r["arch"], r["scorer"]) for r in by["norm"]} == {("mlp", s) for s in Y.NORM_SCORERS} | {("seq", "TOK")}
    assert all(r["norm"] == (r["arch"] == "mlp") for r in by["norm"]) and {r["L"] for r in by["norm"]} == {7, 18, 36}
    assert sum(r["L"] == 128 for r in by["long"]) == 2 and {r["cyclical"] for r in recs} == {False, True}
    assert {r["c"] for r in recs} == {0.0, 1.41, 4.0} and max(r["budget"] for r in recs) == 3000
    # what the generator refuses to go without
    ys = [y for _, y in runs]
    assert max(len(r["path"]) for r in recs if r["ok"]) >= 20
    assert max(y["deepest"] for y in ys) >= 30 and max(y["dead_iters"] for y in ys) >= 100
    assert max(y["overshoot"] for y in ys) >= 2


def test_a_skipped_normalisation_changes_the_search(runs):
    differ = 0
    for c, y in runs:
        if c["norm"]:  # (outputs the table does not hold: numpy's expm1)
            plain = Y.mcts(np.array(c["presentation"]),
                           lambda x, f=Y.model_np(c["scorer"]): np.expm1(np.asarray(f(x), np.float32)),
                           c["budget"], c["c"], c["cyclical"])
            differ += Y.result(plain) != Y.result(y)
    assert differ >= 5


def test_the_shape_report(runs):
    """what the GPU tests assert of their inputs is reported here: both kinds of selection, exact
    ties and near-ties of the UCB score, dead ends, twins, overshoots"""
    ys = [y for _, y in runs]
    assert sum(y["ucb_sel"] > 0 for y in ys) >= 50 and sum(y["unvisited_sel"] > 0 for y in ys) >= 50
    assert sum(y["ties"] for y in ys) >= 1000 and min(y["mingap"] for y in ys) < 1e-4
    assert sum(y["twin_expansions"] > 0 for y in ys) >= 1
    for c, y in runs:
        assert y["iterations"] >= y["dead_iters"] + y["scored_iters"] and len(y["cands"]) == y["scored_iters"], c
        if y["status"] in (Y.BUDGET, Y.EXHAUSTED):
            assert sum(y["cands"]) + 1 == y["nodes"] == len(y["states"]), c
            assert y["iterations"] == y["dead_iters"] + y["scored_iters"] and y["max_visit"] == y["iterations"] + 1, c
    # the negative model's values are clamped: the all-zero model's searches
    mz = {(tuple(c["presentation"]), c["budget"], c["cyclical"]): Y.result(y) for c, y in runs if c["scorer"] == "MZ"}
    mn = {(tuple(c["presentation"]), c["budget"], c["cyclical"]): Y.result(y) for c, y in runs if c["scorer"] == "MN"}
    assert len(mn) >= 8 and all(mz[k] == v for k, v in mn.items())


GOOD = np.array([[1, 2, 0, -2, 0, 0], [2, 0, 0, 1, 1, 0]])


def _zero(x):
    return x[:, 0]


def test_refuses_bad_arguments_without_a_gpu():
    import acx
    from acx.search import mcts_search, mcts_search_many
    assert mcts_search_many is acx.mcts_search_many and mcts_search is acx.mcts_search
    assert {"mcts_search", "mcts_search_many"} <= set(acx.__all__) & set(acx.search.__all__)
    many = acx.mcts_search_many
    for bad, msg in [([[1, 0, 2, 0], [1, 2, 0, 2, 0, 0]], "equal length"),
                     (np.array([[1, 0, 2], [1, 0, 2]]), "even"),
                     (np.array([[1, 0, 2, 0], [1, 1, 0, 0]]), "not a valid presentation"),
                     (np.array([[1, 0, 2, 0], [3, 0, 2, 0]]), r"letters \+-1 \(x\) and \+-2 \(y\) only")]:
        with pytest.raises(ValueError, match=msg):
            many(bad, _zero)
    with pytest.raises(ValueError, match="callable"):
        many(GOOD, None)
    with pytest.raises(ValueError, match="sequence of 2"):
        many(GOOD, _zero, max_nodes_to_explore=[10, 20, 30])
    with pytest.raises(ValueError, match="mcts_search_many supports at most 2\\^24"):
        many(GOOD, _zero, max_nodes_to_explore=(1 << 24) + 1)
    with pytest.raises(ValueError, match="scorer_input"):
        many(GOOD, _zero, scorer_input="states")
    with pytest.raises(ValueError, match="both feat_mean and feat_std"):
        many(GOOD, _zero, feat_mean=np.zeros(14))
    with pytest.raises(ValueError, match="14 values"):
        many(GOOD, _zero, feat_mean=np.zeros(13), feat_std=np.ones(13))
    with pytest.raises(ValueError, match="scorer_input='features'"):
        many(GOOD, _zero, scorer_input="tokens", feat_mean=np.zeros(14), feat_std=np.ones(14))
    with pytest.raises(ValueError, match="on_error"):
        many(GOOD, _zero, on_error="ignore")
    with pytest.raises(ValueError, match="c_explore must not be a NaN"):
        many(GOOD, _zero, c_explore=float("nan"))
    with pytest.raises(ValueError, match="c_explore must be a number"):
        many(GOOD, _zero, c_explore="much")
    assert many(np.zeros((0, 8), np.int32), _zero) == []  # nothing to search: no GPU call either
    res, stats = many(np.zeros((0, 8), np.int32), _zero, return_stats=True)
    assert res == [] and sorted(stats) == ["iterations", "nodes", "status"]
    for kw in (dict(solution_cache={}), dict(time_limit=1.0)):
        with pytest.raises(NotImplementedError):
            acx.mcts_search(GOOD[0], None, **kw)
        with pytest.raises(NotImplementedError):
            acx.mcts_search(GOOD[0], torch.nn.Identity(), **kw)
    with pytest.raises(ValueError, match="feat_mean"):
        acx.mcts_search(GOOD[0], torch.nn.Identity())
    with pytest.raises(ValueError, match="a model is needed"):
        acx.mcts_search(GOOD[0], None)
    from acx.search import _batch_bfs, _batch_mcts
    assert callable(_batch_mcts.release_workspaces)
    _batch_bfs.release_workspaces()  # (nothing cached: no GPU call)


def test_workspace_formula_and_argument_checks():
    """acx_mcts_bytes states the bytes per search of include/acx.h and DESIGN.md "Batched MCTS";
    every entry point refuses bad arguments before any GPU call."""
    from acx import _lib
    lib = _lib.load()
    for L, B in [(1, 1), (12, 50), (18, 2000), (18, 10_000), (64, 777), (65, 778), (128, 3000), (18, 1 << 24)]:
        kw = _lib.key_words(L)
        want = (8 * kw + 36) * (B + 11) + 64 * ((B + 23 + 3) // 4) + 140
        assert lib.acx_mcts_bytes(L, B) == want, (L, B)
        assert want == lib.acx_vgreedy_bytes(L, B) + 16 * (B + 11)  # a record and a trail entry for a heap entry
    for L, B in [(0, 10), (129, 10), (18, 0), (18, (1 << 24) + 1)]:
        assert lib.acx_mcts_bytes(L, B) < 0
        assert not lib.acx_mcts_create(L, 1, B, 0)
    assert not lib.acx_mcts_create(18, 0, 10, 0) and not lib.acx_mcts_create(18, -1, 10, 0)
    lib.acx_mcts_destroy(None)
    assert lib.acx_mcts_begin(None, None, None, 1, None) == _lib.E_ARG
    assert lib.acx_mcts_select(None, None, 0, 1.41, None, None) == _lib.E_ARG
    assert lib.acx_mcts_gather(None, None, 1, None) == _lib.E_ARG
    assert lib.acx_mcts_backup(None, None, 1, None) == _lib.E_ARG
    assert lib.acx_mcts_finish(None, None, None, None, None, None, None) == _lib.E_ARG
    assert lib.acx_mcts_paths(None, 1, None, None, None, 0, None) == _lib.E_ARG
    assert lib.acx_internal_ucb(None, None, None, 1.41, None, 1, None) == _lib.E_ARG
    assert _lib.MCTS_SPIN == 64 and _lib.BEAM_NAN == -5  # the status of a NaN score, shared with the beam search
