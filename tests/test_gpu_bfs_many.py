"""GPU parity of the batched BFS (acx.bfs_many, csrc/acx_mbfs.hip: one workgroup per search): every
search of a batch gives the reference's bfs result (breadth_first.py:15-97) -- against the
reference's recorded runs (tests/golden/search_many.json, kat_search*.json, search_scale.json),
against the yardstick tests/bfs_yardstick.py (checked on the CPU by test_search_many_cpu.py) and
against the one-search device engine acx.bfs(engine="device")."""
import contextlib
import functools
import io
import re

import numpy as np
import pytest
import torch

import bfs_yardstick as Y
from many_common import AK2, _check_records, _dataset_rows, _load, _norm, _same, _scrambled

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")


def _many(pres, budgets, cyc=False, **kw):
    import acx
    res, st = acx.bfs_many(pres, budgets, cyclically_reduce_after_moves=cyc, device=DEV, return_stats=True, **kw)
    assert len(res) == len(pres) and all(len(v) == len(pres) for v in st.values())
    return [_norm(r) for r in res], st


def _device_engine(pres, budget, cyc=False):
    """acx.bfs(engine="device") and its LAST_STATS (the budget line it prints is swallowed)"""
    import acx
    from acx.search import _device_bfs as D
    with contextlib.redirect_stdout(io.StringIO()):
        try:
            res = _norm(acx.bfs(np.asarray(pres), int(budget), cyclically_reduce_after_moves=cyc, device=DEV,
                                engine="device"))
        except AssertionError:
            res = None
    return res, dict(D.LAST_STATS)


def test_dataset_part_in_one_call(capsys):
    recs = _load("search_many.json")["dataset"]
    assert len(recs) == 238 and len({c["budget"] for c in recs}) == 1
    res, st = _many(np.array([c["presentation"] for c in recs]), recs[0]["budget"])
    _check_records(recs, res, st)
    assert capsys.readouterr().out == ""  # bfs_many prints nothing


@pytest.mark.parametrize("cyc", [False, True])
def test_solvable_part_one_call_per_flag_with_per_search_budgets(cyc):
    recs = [c for c in _load("search_many.json")["solvable"] if c["cyclical"] == cyc]
    assert len(recs) >= 50 and len({c["budget"] for c in recs}) == 3 and not any(c["raises"] for c in recs)
    res, st = _many(np.array([c["presentation"] for c in recs]), [c["budget"] for c in recs], cyc)
    _check_records(recs, res, st)


def test_random_reference_searches_grouped_by_length_and_flag():
    import acx
    cases = [c for c in _load("kat_search_extra.json") if c["search_fn"] == "bfs"]
    assert len(cases) == 120 and sum(c["raises"] for c in cases) == 14
    groups = {}
    for c in cases:
        groups.setdefault((len(c["presentation"]), c["cyclical"]), []).append(c)
    assert {k[0] // 2 for k in groups} == {2, 3, 4, 5, 6}
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
        if raising:
            with pytest.raises(AssertionError) as e:
                acx.bfs_many(pres, budgets, cyclically_reduce_after_moves=cyc, device=DEV)
            assert str(raising) in str(e.value)
        else:
            assert [_norm(r) for r in acx.bfs_many(pres, budgets, cyclically_reduce_after_moves=cyc,
                                                   device=DEV)] == res


def test_kat_ak2_and_miller_schupp():
    kat = _load("kat_search.json")
    res, st = _many(np.array([AK2, AK2]), [10 ** 6, 10])
    assert res == [kat["bfs_ak2"], [False, None]] and kat["bfs_ak2"][0]
    assert st["status"].tolist() == [Y.FOUND, Y.BUDGET]
    case = next(c for c in kat["miller_schupp"] if c["search_fn"] == "bfs")
    pres = case["presentations"]
    assert sorted({len(p) // 2 for p in pres}) == [12, 16] and len(pres) == 8
    got = {}
    for W in (24, 32):  # one call per max_relator_length
        idx = [i for i, p in enumerate(pres) if len(p) == W]
        res, _ = _many([pres[i] for i in idx], case["budget"])
        got.update(zip(idx, res))
    assert [pres[i] for i in range(8) if got[i][0]] == case["solved"]
    assert [pres[i] for i in range(8) if not got[i][0]] == case["unsolved"]
    assert [got[i][1] for i in range(8) if got[i][0]] == case["paths"]


def test_scale_records_at_L128_as_one_batch():
    recs = [c for c in _load("search_scale.json") if c["search_fn"] == "bfs" and c["L"] == 128]
    assert len(recs) == 2 and all(c["budget"] == 3000 for c in recs)
    for cyc in (False, True):  # (the two records differ in the flag: one batch of two per flag)
        res, st = _many(np.array([c["presentation"] for c in recs]), 3000, cyc)
        for i, c in enumerate(recs):
            if c["cyclical"] != cyc:
                continue
            assert res[i] == [c["ok"], c["path"]]
            assert st["parents"][i] == c["parents"]
            m = re.search(r"number of explored nodes = (\d+)", c["stdout"][-1])
            assert st["nodes"][i] == int(m.group(1)) and st["status"][i] == Y.BUDGET


# ---------------------------------------------------------------------------------------------
# round boundaries: searches shaped so that the 64-parent rounds of the kernel meet every case
# ---------------------------------------------------------------------------------------------
BIG = 3000
FLAGS = ("crosses_64", "mid_round_cut", "success_beats_cut", "cut_beats_success", "same_child_in_round")


@functools.lru_cache(maxsize=None)
def boundary_cases(L):
    """[(presentation, budget, yardstick result)] and the flags they raise, from the yardstick alone"""
    rng = np.random.default_rng(1000 + L)
    cases, flags = [], set()

    def add(s, budget):
        r = Y.bfs(s, budget)
        cases.append((s, budget, r))
        return r

    for n in range(8):
        s = _scrambled(L, rng, 3 + n % 4)
        big = add(s, BIG)
        after, parent = big["nodes_after"], big["node_parent"]
        rs = Y.rounds(after)
        depth = [0] * len(parent)
        for j in range(1, len(parent)):
            depth[j] = depth[parent[j]] + 1
        for (h, P), (h2, _) in zip(rs, rs[1:]):  # a level longer than the round that starts in it
            if P == Y.ROUND and depth[h2 - 1] == depth[h2]:
                flags.add("crosses_64")
        if any(parent[j] != at and Y.round_of(rs, parent[j]) == Y.round_of(rs, at) for at, j in big["dups"]
               if parent[j] >= 0 and at < len(after)):
            flags.add("same_child_in_round")
        full = [(h, P) for h, P in rs if P == Y.ROUND]
        if full:  # the budget reached at the 32nd parent of a full round
            h, P = full[-1]
            r = add(s, after[h + 31])
            cut = r["parents"] - 1
            if r["status"] == Y.BUDGET and h < cut < h + P - 1:
                flags.add("mid_round_cut")
        if big["status"] == Y.FOUND:
            ps = big["parents"] - 1  # the parent of the success child
            rs_to = Y.rounds(after + after[-1:])  # the rounds up to the one that takes parent ps
            h = rs_to[Y.round_of(rs_to, ps)][0] if ps >= 1 else 0
            if ps >= 1 and big["nodes"] > after[ps - 1]:
                # the budget is met by the success parent's children before the success child:
                # without the success the cut would come after this very parent
                r = add(s, big["nodes"])
                assert r["status"] == Y.FOUND and r["path"] == big["path"]
                flags.add("success_beats_cut")
            if ps - 1 >= h and ps >= 1:  # the cut one parent before the success, in its round
                r = add(s, after[ps - 1])
                cut = r["parents"] - 1
                if r["status"] == Y.BUDGET and h <= cut < ps:
                    flags.add("cut_beats_success")
    return cases, flags


@pytest.mark.parametrize("L", [12, 13, 16, 17, 36])
def test_round_boundaries_against_yardstick_and_device_engine(L):
    cases, flags = boundary_cases(L)
    assert flags == set(FLAGS), (L, set(FLAGS) - flags)  # every case occurs: the test is not vacuous
    pres = np.stack([c[0] for c in cases])
    budgets = [c[1] for c in cases]
    res, st = _many(pres, budgets)
    for i, (s, budget, y) in enumerate(cases):
        assert res[i] == [y["ok"], None if y["path"] is None else [list(x) for x in y["path"]]], (L, i)
        assert (st["status"][i], st["nodes"][i], st["parents"][i], st["min_length"][i]) == \
            (y["status"], y["nodes"], y["parents"], y["min_length"]), (L, i, budget)
        dres, d = _device_engine(s, budget)
        assert dres == res[i], (L, i)
        assert (d["status"], d["parents"], d["min_length"]) == (y["status"], y["parents"], y["min_length"]), (L, i)
        if d["status"] == Y.BUDGET:  # (on other exits the device engine counts whole chunks)
            assert d["nodes"] == st["nodes"][i], (L, i)


# ---------------------------------------------------------------------------------------------
# batch shapes, splitting, workspace reuse
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [1, 3])
def test_small_batches(N):
    rows = _dataset_rows()[:N]
    budgets = [150, 40, 700][:N]
    res, st = _many(rows, budgets)
    for i in range(N):
        y = Y.bfs(rows[i], budgets[i])
        assert res[i] == [y["ok"], y["path"]] and y["status"] == Y.BUDGET
        assert (st["status"][i], st["nodes"][i], st["parents"][i], st["min_length"][i]) == \
            (y["status"], y["nodes"], y["parents"], y["min_length"])


def test_more_searches_than_resident_workgroups():
    rows = _dataset_rows()
    N = 4096
    res, st = _many(rows[np.arange(N) % len(rows)], 200)
    for i in range(len(rows), N):  # identical rows, identical results
        j = i % len(rows)
        assert res[i] == res[j] and all(st[k][i] == st[k][j] for k in st), i
    for j in range(len(rows)):
        dres, d = _device_engine(rows[j], 200)
        assert dres == res[j], j
        assert (d["status"], d["nodes"], d["parents"], d["min_length"]) == \
            (st["status"][j], st["nodes"][j], st["parents"][j], st["min_length"][j]) and d["status"] == Y.BUDGET, j


def test_split_call_equals_unsplit_call():
    from acx import _lib
    from acx.search import _batch_bfs as B
    recs = _load("search_many.json")["solvable"]
    recs = [c for c in recs if not c["cyclical"] and c["budget"] <= 1000][:40]
    pres = np.array([c["presentation"] for c in recs])
    budgets = [c["budget"] for c in recs]
    whole = _many(pres, budgets)
    B.release_workspaces()
    per = _lib.load().acx_mbfs_bytes(18, max(budgets))
    split = _many(pres, budgets, workspace_bytes=7 * per + per // 2)  # groups of 7: 5 full, one of 5
    assert B._HANDLES[(0, 18, False)][1] == 7
    assert _same(split, whole)
    assert _same(_many(pres, budgets, workspace_bytes=1), whole)  # never less than one search per launch
    assert any(r[0] for r in whole[0]) and not all(r[0] for r in whole[0])


def test_cached_handle_gives_what_a_fresh_one_gives():
    from acx.search import _batch_bfs as B
    from acx.search import _device_bfs as D
    recs = [c for c in _load("search_many.json")["solvable"] if not c["cyclical"] and c["budget"] <= 1000]
    first, second = recs[:24], recs[24:48][::-1]
    B.release_workspaces()
    args = [(np.array([c["presentation"] for c in part]), [c["budget"] for c in part]) for part in (first, second)]
    _many(*args[0])
    h = dict(B._HANDLES)
    assert len(h) == 1
    again = _many(*args[1])
    assert B._HANDLES == h  # the same workspace
    D.release_workspaces()  # frees the batch workspaces too
    assert not B._HANDLES
    fresh = _many(*args[1])
    assert _same(again, fresh)
    _check_records(second, fresh[0], fresh[1])
    for _ in range(70):  # past the wrap of the table's 6-bit epoch
        _many(*args[0])
    assert _same(_many(*args[1]), fresh)
    B.release_workspaces()
