"""GPU parity of the batched greedy search (acx.greedy_search_many, csrc/acx_mgreedy.hip: one wave
per search, the frontier a heap on the device): every search of a batch gives the reference's
greedy_search result (greedy.py:15-121) -- against the reference's recorded runs
(tests/golden/greedy_many.json, kat_search*.json, search_scale.json), against the yardstick
tests/greedy_yardstick.py (checked on the CPU by test_greedy_many_cpu.py) and against the
one-search device engine acx.greedy_search(engine="device")."""
import contextlib
import functools
import io
import re

import numpy as np
import pytest
import torch

import greedy_yardstick as Y
from many_common import AK2, _check_records, _dataset_rows, _load, _norm, _same, _scrambled

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")


def _many(pres, budgets, cyc=False, **kw):
    import acx
    res, st = acx.greedy_search_many(pres, budgets, cyclically_reduce_after_moves=cyc, device=DEV, return_stats=True,
                                     **kw)
    assert len(res) == len(pres) and all(len(v) == len(pres) for v in st.values())
    return [_norm(r) for r in res], st


def _device_engine(pres, budget, cyc=False):
    """acx.greedy_search(engine="device") and its LAST_STATS (the budget line it prints is swallowed)"""
    import acx
    from acx.search import _engine as E
    with contextlib.redirect_stdout(io.StringIO()):
        try:
            res = _norm(acx.greedy_search(np.asarray(pres), int(budget), cyclically_reduce_after_moves=cyc,
                                          device=DEV, engine="device"))
        except AssertionError:
            res = None
    return res, dict(E.LAST_STATS)


def _check_yardstick(res, st, i, y, tag):
    assert res[i] == (None if y["raises"] else [y["ok"], [list(x) for x in y["path"]]]), tag
    assert (st["status"][i], st["nodes"][i], st["parents"][i], st["min_length"][i]) == \
        (y["status"], y["nodes"], y["parents"], y["min_length"]), tag


def test_dataset_part_in_one_call(capsys):
    recs = _load("greedy_many.json")["dataset"]
    assert len(recs) == 238 and {c["budget"] for c in recs} == {2000}
    res, st = _many(np.array([c["presentation"] for c in recs]), 2000)
    _check_records(recs, res, st)
    assert sum(c["ok"] for c in recs) >= 30 and sum(not c["ok"] for c in recs) >= 60
    assert capsys.readouterr().out == ""  # greedy_search_many prints nothing


@pytest.mark.parametrize("cyc", [False, True])
def test_solvable_part_one_call_per_flag_with_per_search_budgets(cyc):
    recs = [c for c in _load("greedy_many.json")["solvable"] if c["cyclical"] == cyc]
    assert len(recs) >= 50 and len({c["budget"] for c in recs}) == 3
    assert any(c["ok"] for c in recs) and any(not c["ok"] for c in recs) and not any(c["raises"] for c in recs)
    res, st = _many(np.array([c["presentation"] for c in recs]), [c["budget"] for c in recs], cyc)
    _check_records(recs, res, st)


def test_random_reference_searches_grouped_by_length_and_flag():
    import acx
    cases = [c for c in _load("kat_search_extra.json") if c["search_fn"] == "greedy_search"]
    assert len(cases) == 120 and sum(c["raises"] for c in cases) == 70
    groups = {}
    for c in cases:
        groups.setdefault((len(c["presentation"]), c["cyclical"]), []).append(c)
    assert {k[0] // 2 for k in groups} == {2, 3, 4, 5, 6}
    exhausted = 0
    for (_, cyc), recs in sorted(groups.items()):
        pres = [c["presentation"] for c in recs]  # a list of rows
        budgets = [c["budget"] for c in recs]
        res, st = _many(pres, budgets, cyc, on_error="return")
        raising = [i for i, c in enumerate(recs) if c["raises"]]
        assert [i for i, r in enumerate(res) if r is None] == raising
        assert np.nonzero(st["status"] == Y.MOVE_ERROR)[0].tolist() == raising
        keep = [i for i in range(len(recs)) if i not in raising]
        _check_records([recs[i] for i in keep], [res[i] for i in keep], {k: v[keep] for k, v in st.items()},
                       "budget_nodes")
        exhausted += int((st["status"] == Y.EXHAUSTED).sum())
        if raising:
            with pytest.raises(AssertionError) as e:
                acx.greedy_search_many(pres, budgets, cyclically_reduce_after_moves=cyc, device=DEV)
            assert str(raising) in str(e.value) and "greedy_search_many" in str(e.value)
        else:
            assert [_norm(r) for r in acx.greedy_search_many(pres, budgets, cyclically_reduce_after_moves=cyc,
                                                             device=DEV)] == res
    assert exhausted == 8  # the frontier ran dry: (False, the last popped node's path + its last child)


def test_kat_ak2_and_miller_schupp():
    kat = _load("kat_search.json")
    res, st = _many(np.array([AK2, AK2]), [10 ** 6, 10])
    assert res == [kat["greedy_ak2"], kat["greedy_ak2_budget10"]] and kat["greedy_ak2"][0]
    assert st["status"].tolist() == [Y.FOUND, Y.BUDGET]
    case = next(c for c in kat["miller_schupp"] if c["search_fn"] == "greedy_search" and c["budget"] == 10 ** 4)
    pres = case["presentations"]
    assert len(pres) == 16
    got = {}
    for W in sorted({len(p) for p in pres}):  # one call per max_relator_length
        idx = [i for i, p in enumerate(pres) if len(p) == W]
        res, _ = _many([pres[i] for i in idx], case["budget"])
        got.update(zip(idx, res))
    n = len(pres)
    assert [pres[i] for i in range(n) if got[i][0]] == case["solved"]
    assert [pres[i] for i in range(n) if not got[i][0]] == case["unsolved"]
    assert [got[i][1] for i in range(n) if got[i][0]] == case["paths"]


def test_scale_records_at_L128_as_one_batch():
    recs = [c for c in _load("search_scale.json") if c["search_fn"] == "greedy_search" and c["L"] == 128]
    assert len(recs) == 3 and all(c["budget"] == 3000 for c in recs) and {c["cyclical"] for c in recs} == {False, True}
    for cyc in (False, True):  # one batch of all three per flag; the records of that flag are checked
        res, st = _many(np.array([c["presentation"] for c in recs]), 3000, cyc)
        for i, c in enumerate(recs):
            if c["cyclical"] != cyc:
                continue
            assert res[i] == [c["ok"], c["path"]]
            assert st["parents"][i] == c["parents"]
            m = re.search(r"number of explored nodes = (\d+)", c["stdout"][-1])
            assert st["nodes"][i] == int(m.group(1)) and st["status"][i] == Y.BUDGET


# ---------------------------------------------------------------------------------------------
# boundaries: searches shaped so that the kernel's pops and its heap meet every case
# ---------------------------------------------------------------------------------------------
BIG = 3000
LEVEL_SIZES = (1, 1 + Y.FAN, 1 + Y.FAN + Y.FAN ** 2)  # entries of the heap with 1, 2, 3 full levels
FLAGS = ("budget_exact", "success_beats_cut", "same_child_in_pop", "k0_tie", "frontier_crosses_fanout", "budget_1")
# Near-full relators: most moves would pass max_relator_length and change nothing, so the search
# ends on an empty frontier -- after the frontier has held more than 1 + 64 + 64^2 entries (found
# by trying random reduced words of length L - 2 .. L with the yardstick).
DRAINING = {  # L: r0 then r1, each zero-padded to L
    12: [-2, -1, -1, 2, 1, -2, 1, 2, 2, 2, 2, 0,
         -2, 1, 1, 1, 1, -2, -2, -1, -2, -1, 0, 0],
    13: [2, 2, 1, -2, -1, -2, -1, 2, 1, 1, 1, 0, 0,
         1, 2, 2, -1, -1, -1, -1, -1, -1, -2, -1, -1, 0],
    16: [-2, -1, -2, 1, -2, -2, -2, -2, -2, 1, 2, 2, 2, 2, 0, 0,
         1, -2, -2, 1, -2, -2, 1, 2, -1, -2, -1, 2, -1, 2, -1, 2],
    17: [1, 2, 2, 2, 1, 2, 1, -2, -1, -2, -2, 1, 2, -1, -2, 0, 0,
         -1, -2, -2, -2, -2, -2, -1, -2, -1, 2, -1, 2, 2, 1, 2, 0, 0],
    36: [2, -1, 2, 1, 2, 1, 2, -1, -2, -1, 2, 1, 2, 1, -2, -2, -1, -1, -2, -1, -1, -2, 1, -2, 1, -2, -2, 1,
         -2, -1, -2, -2, 1, 1, -2, 0,
         -2, -1, -1, 2, 1, 1, -2, 1, 2, -1, -1, -1, -1, -2, -1, -1, -1, 2, 2, 2, 2, 1, 1, 1, 2, 1, -2, 1, -2,
         -2, 1, -2, 1, 2, 1, -2],
}


def _crosses(frontier, size):
    """the frontier grows past `size` entries and later shrinks back below it"""
    up = [i for i, f in enumerate(frontier) if f > size]
    return bool(up) and any(f < size for f in frontier[up[0]:])


@functools.lru_cache(maxsize=None)
def boundary_cases(L):
    """[(presentation, budget, cyclical, yardstick result)] and the flags they raise, from the
    yardstick alone"""
    rng = np.random.default_rng(2000 + L)
    cases, flags = [], set()

    def add(s, budget, cyc, shape=True):
        r = Y.greedy(s, budget, cyc, shape=shape)
        cases.append((s, budget, cyc, r))
        return r

    # the heap gains its second and third level and loses them again (appended last: the
    # one-search engine is run on the first cases only)
    drain = Y.greedy(np.array(DRAINING[L], np.int32), 10 ** 6)
    if drain["status"] == Y.EXHAUSTED and all(_crosses([1] + drain["frontier_after"], size) for size in LEVEL_SIZES):
        flags.add("frontier_crosses_fanout")
    for n in range(10):
        cyc = bool(n % 2)
        s = _scrambled(L, rng, 4 + n)
        big = add(s, BIG, cyc)
        after = big["nodes_after"]
        if big["same_child"]:
            flags.add("same_child_in_pop")
        if big["k0_ties"]:
            flags.add("k0_tie")
        if add(s, 1, cyc)["parents"] == 1:
            flags.add("budget_1")
        if len(after) >= 4:  # the budget met exactly after pop i, and one node later
            i = len(after) // 2
            r0, r1 = add(s, after[i], cyc), add(s, after[i] + 1, cyc)
            if (r0["status"], r0["parents"], r0["nodes"]) == (Y.BUDGET, i + 1, after[i]) and r1["parents"] > i + 1:
                flags.add("budget_exact")
        if big["status"] == Y.FOUND and big["parents"] >= 2 and big["nodes"] > after[-1]:
            # the budget is met by the success pop's children before the success child: without
            # the success the cut would come after this very pop
            r = add(s, big["nodes"], cyc)
            assert r["status"] == Y.FOUND and r["path"] == big["path"] and r["success_beats_cut"]
            flags.add("success_beats_cut")
    cases.append((np.array(DRAINING[L], np.int32), 10 ** 6, False, drain))
    return cases, flags


@pytest.mark.parametrize("L", [12, 13, 16, 17, 36])
def test_boundaries_against_yardstick_and_device_engine(L):
    cases, flags = boundary_cases(L)
    assert flags == set(FLAGS), (L, set(FLAGS) - flags)  # every case occurs: the test is not vacuous
    for cyc in (False, True):
        part = [c for c in cases if c[2] == cyc]
        res, st = _many(np.stack([c[0] for c in part]), [c[1] for c in part], cyc, on_error="return")
        for i, (s, budget, _, y) in enumerate(part):
            _check_yardstick(res, st, i, y, (L, cyc, i, budget))
        for i, (s, budget, _, y) in enumerate(part[:20]):  # at most 40 cases through the one-search engine
            dres, d = _device_engine(s, budget, cyc)
            assert dres == res[i], (L, cyc, i)
            assert d["min_length"] == y["min_length"], (L, cyc, i)
            if y["status"] == Y.BUDGET:
                assert d["nodes"] == st["nodes"][i], (L, cyc, i)


# ---------------------------------------------------------------------------------------------
# batch shapes, splitting, workspace reuse
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [1, 3])
def test_small_batches(N):
    rows = _dataset_rows()[:N]
    budgets = [150, 40, 700][:N]
    res, st = _many(rows, budgets)
    for i in range(N):
        _check_yardstick(res, st, i, Y.greedy(rows[i], budgets[i]), (N, i))


def test_more_searches_than_resident_workgroups():
    rows = _dataset_rows()
    N = 4096
    res, st = _many(rows[np.arange(N) % len(rows)], 200)
    for i in range(len(rows), N):  # identical rows, identical results
        j = i % len(rows)
        assert res[i] == res[j] and all(st[k][i] == st[k][j] for k in st), i
    for j in range(len(rows)):
        _check_yardstick(res, st, j, Y.greedy(rows[j], 200), j)


def test_split_call_equals_unsplit_call():
    from acx import _lib
    from acx.search import _batch_greedy as G
    recs = _load("greedy_many.json")["solvable"]
    recs = [c for c in recs if not c["cyclical"] and c["budget"] <= 1000][:40]
    pres = np.array([c["presentation"] for c in recs])
    budgets = [c["budget"] for c in recs]
    whole = _many(pres, budgets)
    G.release_workspaces()
    per = _lib.load().acx_mgreedy_bytes(18, max(budgets))
    split = _many(pres, budgets, workspace_bytes=7 * per + per // 2)  # groups of 7: 5 full, one of 5
    assert G._HANDLES[(0, 18, False)][1] == 7
    assert _same(split, whole)
    assert _same(_many(pres, budgets, workspace_bytes=1), whole)  # never less than one search per launch
    assert any(r[0] for r in whole[0]) and not all(r[0] for r in whole[0])


def test_cached_handle_gives_what_a_fresh_one_gives():
    from acx.search import _batch_bfs as B
    from acx.search import _batch_greedy as G
    from acx.search import _device_bfs as D
    recs = [c for c in _load("greedy_many.json")["solvable"] if not c["cyclical"] and c["budget"] <= 1000]
    first, second = recs[:24], recs[24:48][::-1]
    G.release_workspaces()
    args = [(np.array([c["presentation"] for c in part]), [c["budget"] for c in part]) for part in (first, second)]
    _many(*args[0])
    h = dict(G._HANDLES)
    assert len(h) == 1
    again = _many(*args[1])
    assert G._HANDLES == h  # the same workspace
    D.release_workspaces()  # frees the batch workspaces too
    assert not G._HANDLES
    fresh = _many(*args[1])
    assert _same(again, fresh)
    _check_records(second, fresh[0], fresh[1])
    B.release_workspaces()  # so does the batched BFS's
    assert not G._HANDLES
    for _ in range(70):  # past the wrap of the table's 6-bit epoch
        _many(*args[0])
    assert _same(_many(*args[1]), fresh)
    G.release_workspaces()
    assert not G._HANDLES
