"""CPU side of the batched value-guided greedy search (acx.value_guided_greedy_search_many,
acx.value_guided_greedy_search): the yardstick its GPU tests rest on (tests/vgreedy_yardstick.py, the
reference's value_guided_greedy_search restated literally over the oracle's expansion) reproduces
the reference's own recorded runs -- tests/golden/vgreedy_search.json (make_golden_vgreedy.py); the
engine's variant of it, which drops the later of two equal new children of one pop, gives the same
results; the argument checks are made before any GPU call."""
import numpy as np
import pytest
import torch

import vgreedy_yardstick as Y
from many_common import _load


def _end(r):
    return "raises" if r["raises"] else "found" if r["ok"] else "budget" if r["nodes_explored"] >= max(
        r["budget"], 1) else "died"


def _run(c, **kw):
    norm = dict(mean=Y.NORM_MEAN, std=Y.NORM_STD) if c["norm"] else {}
    return Y.vgreedy(np.array(c["presentation"]), c["scorer"], c["budget"], c["cyclical"], **norm, **kw)


@pytest.fixture(scope="module")
def runs():
    """(record, the literal yardstick's run, the dropping variant's run) for every record"""
    return [(c, _run(c), _run(c, drop_twins=True)) for c in _load("vgreedy_search.json")]


def test_the_fixture_covers_what_it_is_for(runs):
    recs = [c for c, _, _ in runs]
    by = {}
    for r in recs:
        by.setdefault(r["name"].split("-")[0], []).append(r)
    assert {_end(r) for r in recs} == {"found", "budget", "died", "raises"}
    assert {(r["L"], r["cyclical"], r["budget"]) for r in by["ak"]} == {(L, c, b) for L in (7, 18) for c in (False, True)
                                                                        for b in (1, 37, 3000)}
    assert {r["scorer"] for r in by["ak"]} == {"S0", "S1", "S2", "S3", "S4"}
    assert len(by["ms"]) == 30 and all(r["L"] == 36 for r in by["ms"]) and {"found", "budget"} <= {_end(r) for r in by["ms"]}
    assert len(by["len"]) >= 10 and all(r["length_priority"] and r["scorer"] == "S0" for r in by["len"])
    assert {r["L"] for r in by["len"]} == {7, 18, 36} and not any(r["length_priority"] for r in recs if r not in by["len"])
    assert len(by["raise"]) >= 3 and all(r["raises"] for r in by["raise"])
    assert {(r["arch"], r["scorer"]) for r in by["norm"]} == {("mlp", s) for s in Y.NORM_SCORERS} | {("seq", "TOK")}
    assert all(r["norm"] == (r["arch"] == "mlp") for r in by["norm"]) and {r["L"] for r in by["norm"]} == {7, 18, 36}
    assert any(r["L"] == 128 for r in by["long"]) and {r["cyclical"] for r in recs} == {False, True}
    assert 1 <= min(r["budget"] for r in by["ak"]) and max(r["budget"] for r in recs) == 3000
    named = {r["name"]: r for r in recs}
    assert _end(named["roots-dies"]) == "died" and named["roots-dies"]["nodes_explored"] == 1
    assert named["roots-trivial"]["ok"] and named["roots-trivial"]["nodes_explored"] == 1
    # a budget of 1 (or 0) still runs one pop: AK(2)'s root has 6 new children
    assert (named["roots-budget1"]["nodes_explored"], named["roots-budget0"]["nodes_explored"]) == (7, 7)
    # what the generator refuses to go without
    assert max(r["nodes_explored"] - r["budget"] for r in recs if _end(r) == "budget" and r["budget"] >= 1) >= 2
    assert any(y["min_dup"] and y["min_length"] < int(np.count_nonzero(c["presentation"])) for c, y, _ in runs)


def test_yardstick_reproduces_every_reference_record(runs):
    """literally, twins included: (solved, path, nodes_explored, min_length)"""
    for c, y, _ in runs:
        assert Y.result(y) == (c["raises"], c["ok"], c["path"] or [], c["nodes_explored"], c["min_length"]), c
        want = {"found": Y.FOUND, "budget": Y.BUDGET, "died": Y.EXHAUSTED, "raises": Y.MOVE_ERROR}[_end(c)]
        assert y["status"] == want, c


def test_a_skipped_normalisation_changes_the_search(runs):
    differ = [c for c, y, _ in runs if c["norm"] and Y.result(Y.vgreedy(np.array(c["presentation"]), c["scorer"],
                                                                         c["budget"], c["cyclical"])) != Y.result(y)]
    assert len(differ) >= 5 and any(c["scorer"] == "NNEG" for c in differ)


def test_dropping_the_later_twin_changes_nothing_observable(runs):
    """the derivation in csrc/acx_vgreedy.hip: the later of two equal new children of a pop has the
    same score and depth and a larger id, and its pop finds every child visited"""
    twins = 0
    for c, y, d in runs:
        assert Y.result(d) == Y.result(y) and d["status"] == y["status"], c
        twins += bool(y["twin_pops"])
        if y["twin_pops"] and y["status"] != Y.FOUND:
            assert len(d["states"]) < len(y["states"])  # the literal run gave the twin a node id
    assert twins >= 10
    extra = 0
    for p, s, b, cyc in Y.twin_cases():
        y, d = Y.vgreedy(p, s, b, cyc), Y.vgreedy(p, s, b, cyc, drop_twins=True)
        assert Y.result(d) == Y.result(y) and d["status"] == y["status"], (p, s, b, cyc)
        assert y["twin_pops"] and d["twin_pops"], (p, s, b, cyc)
        extra += y["twin_pops"][0] == 1
    assert extra >= 6  # the root's own pop


def test_the_shape_report(runs):
    """pops with no new child while the heap is not empty, ties decided by the node id, frontier
    peaks, budget overshoots: what the GPU tests assert of their inputs is reported here"""
    ys = [d for _, _, d in runs]
    assert sum(bool(y["empty_pops"]) for y in ys) >= 10 and sum(y["id_ties"] > 0 for y in ys) >= 50
    assert max(y["peak"] for y in ys) > 2000 and {y["peak"] for y in ys} >= {1}
    for y in ys:  # the heap that is popped from is never larger than the one pushed to
        assert y["max_popped"] <= y["peak"] and sum(y["level_pops"]) == y["steps"] and y["level_pops"][0] >= 1
    assert sum(y["level_pops"][2] > 0 for y in ys) >= 50 and [Y.heap_level(n) for n in (1, 2, 65, 66, 4161, 4162)] == [
        0, 1, 1, 2, 2, 3]
    assert max(y["overshoot"] for y in ys) >= 5
    for c, _, d in runs:
        if d["status"] in (Y.BUDGET, Y.EXHAUSTED):
            assert len(d["cands"]) == d["steps"] and sum(d["cands"]) + 1 == d["nodes"] == d["nodes_after"][-1], c
    # S2 and S4 tie every score: the same searches, -0.0 equal to +0.0
    s2 = {(tuple(c["presentation"]), c["budget"], c["cyclical"]): Y.result(d) for c, _, d in runs if c["scorer"] == "S2"}
    s4 = {(tuple(c["presentation"]), c["budget"], c["cyclical"]): Y.result(d) for c, _, d in runs if c["scorer"] == "S4"}
    assert s2 == s4 and len(s2) >= 12


GOOD = np.array([[1, 2, 0, -2, 0, 0], [2, 0, 0, 1, 1, 0]])


def _zero(x):
    return x[:, 0]


def test_refuses_bad_arguments_without_a_gpu():
    import acx
    from acx.search import value_guided_greedy_search, value_guided_greedy_search_many
    assert value_guided_greedy_search_many is acx.value_guided_greedy_search_many
    assert value_guided_greedy_search is acx.value_guided_greedy_search
    assert {"value_guided_greedy_search", "value_guided_greedy_search_many"} <= set(acx.__all__) & set(acx.search.__all__)
    many = acx.value_guided_greedy_search_many
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
    with pytest.raises(ValueError, match="value_guided_greedy_search_many supports at most 2\\^24"):
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
    assert many(np.zeros((0, 8), np.int32), _zero) == []  # nothing to search: no GPU call either
    res, stats = many(np.zeros((0, 8), np.int32), _zero, return_stats=True)
    assert res == [] and sorted(stats) == ["min_length", "nodes", "status", "steps"]
    for kw in (dict(solution_cache={}), dict(time_limit=1.0)):
        with pytest.raises(NotImplementedError):
            acx.value_guided_greedy_search(GOOD[0], None, **kw)
        with pytest.raises(NotImplementedError):
            acx.value_guided_greedy_search(GOOD[0], None, use_length_priority=True, **kw)
    with pytest.raises(ValueError, match="feat_mean"):
        acx.value_guided_greedy_search(GOOD[0], torch.nn.Identity())
    with pytest.raises(ValueError, match="a model is needed"):
        acx.value_guided_greedy_search(GOOD[0])
    from acx.search import _batch_bfs, _batch_vgreedy
    assert callable(_batch_vgreedy.release_workspaces)
    _batch_bfs.release_workspaces()  # (nothing cached: no GPU call)


def test_workspace_formula_and_argument_checks():
    """acx_vgreedy_bytes states the bytes per search of include/acx.h and DESIGN.md "Batched
    value-guided greedy"; every entry point refuses bad arguments before any GPU call."""
    from acx import _lib
    lib = _lib.load()
    for L, B in [(1, 1), (12, 50), (18, 2000), (18, 10_000), (64, 777), (65, 778), (128, 3000), (18, 1 << 24)]:
        kw = _lib.key_words(L)
        want = (8 * kw + 20) * (B + 11) + 64 * ((B + 23 + 3) // 4) + 140
        assert lib.acx_vgreedy_bytes(L, B) == want, (L, B)
        assert want == lib.acx_mgreedy_bytes(L, B) + 108  # the greedy engine's slices and the step's state
    for L, B in [(0, 10), (129, 10), (18, 0), (18, (1 << 24) + 1)]:
        assert lib.acx_vgreedy_bytes(L, B) < 0
        assert not lib.acx_vgreedy_create(L, 1, B, 0)
    assert not lib.acx_vgreedy_create(18, 0, 10, 0) and not lib.acx_vgreedy_create(18, -1, 10, 0)
    lib.acx_vgreedy_destroy(None)
    assert lib.acx_vgreedy_begin(None, None, None, 1, None) == _lib.E_ARG
    assert lib.acx_vgreedy_pop(None, None, None) == _lib.E_ARG
    assert lib.acx_vgreedy_gather(None, None, 1, None) == _lib.E_ARG
    assert lib.acx_vgreedy_push(None, None, 1, None) == _lib.E_ARG
    assert lib.acx_vgreedy_finish(None, None, None, None, None, None, None) == _lib.E_ARG
    assert lib.acx_vgreedy_paths(None, 1, None, None, None, 0, None) == _lib.E_ARG
    assert _lib.BEAM_NAN == -5  # the status of a NaN score, shared with the beam search
