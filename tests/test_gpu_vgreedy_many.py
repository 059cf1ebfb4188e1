"""GPU parity of the batched value-guided greedy search (acx.value_guided_greedy_search_many /
acx.value_guided_greedy_search, csrc/acx_vgreedy.hip: one wave per search, a step = pop, gather, the
caller's scorer, push): with scorers whose float32 values are exact, every search gives the
reference's value_guided_greedy_search result (value_search/value_guided_search.py:253-414) --
against the reference's recorded runs (tests/golden/vgreedy_search.json) and against the yardstick
tests/vgreedy_yardstick.py (checked on the CPU by test_vgreedy_cpu.py; here its drop_twins variant,
which is the engine's and which that file proves equal to the literal one).  A call has one scorer,
so the fixture's records are grouped by (L, flag, scorer, normalisation)."""
import functools

import numpy as np
import pytest
import torch

import beam_yardstick as BY
import vgreedy_yardstick as Y
from many_common import AK2, _dataset_rows, _load, _norm, _same, _scrambled
from scored_common import AK3, Engine, _FnModel, _key, _pad, _refused, _solvable, _thirteen, drive
from test_gpu_batch_refusals import _check_search as _refusals_check_search
from test_gpu_batch_refusals import _rows

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
def _fn(scorer):
    if not isinstance(scorer, str):
        return scorer, {}
    if scorer in Y.TOKEN_SCORERS:
        return Y.TOKEN_SCORERS[scorer][1], dict(scorer_input="tokens")
    return Y.SCORERS[scorer][1], {}


def _many(pres, scorer, budgets, cyc=False, **kw):
    import acx
    fn, skw = _fn(scorer)
    res, st = acx.value_guided_greedy_search_many(pres, fn, max_nodes_to_explore=budgets,
                                                  cyclically_reduce_after_moves=cyc, device=DEV, return_stats=True,
                                                  **skw, **kw)
    assert len(res) == len(pres) and all(len(v) == len(pres) for v in st.values())
    return [_norm(r) for r in res], st


def _check_yardstick(res, st, i, y, tag):
    assert res[i] == (None if y["raises"] else [y["ok"], y["path"]]), tag
    got = (st["status"][i], st["nodes"][i], st["steps"][i], st["min_length"][i])
    assert got == (y["status"], y["nodes"], y["steps"], y["min_length"]), (tag, got)


def _check_record(res, st, i, c):
    if c["raises"]:
        assert res[i] is None and st["status"][i] == Y.MOVE_ERROR, c
        return
    assert res[i] == [c["ok"], c["path"]], c
    assert (st["nodes"][i], st["min_length"][i]) == (c["nodes_explored"], c["min_length"]), c
    died = not c["ok"] and c["nodes_explored"] < max(c["budget"], 1)
    assert st["status"][i] == (Y.FOUND if c["ok"] else Y.EXHAUSTED if died else Y.BUDGET), c


def _record_kw(c):
    return dict(feat_mean=Y.NORM_MEAN, feat_std=Y.NORM_STD) if c["norm"] else {}


def test_every_fixture_record_grouped_into_single_calls(capsys):
    groups = {}
    for c in _load("vgreedy_search.json"):
        groups.setdefault((c["L"], c["cyclical"], c["scorer"], c["norm"]), []).append(c)
    assert sum(len(g) for g in groups.values()) >= 130 and {k[0] for k in groups} >= {2, 7, 18, 36, 128}
    for (L, cyc, scorer, norm), recs in sorted(groups.items()):
        res, st = _many(np.array([c["presentation"] for c in recs]), scorer, [c["budget"] for c in recs], cyc,
                        on_error="return", **_record_kw(recs[0]))
        for i, c in enumerate(recs):
            _check_record(res, st, i, c)
    assert capsys.readouterr().out == ""  # value_guided_greedy_search_many prints nothing


@pytest.mark.parametrize("group", ["ak", "len", "roots raise", "ms", "norm", "long"])
def test_fixture_records_through_value_guided_greedy_search(group):
    """the reference's signature, the model's output through expm1 on the GPU: expm1 is strictly
    increasing over every value these scorers returned in the reference's runs
    (make_golden_vgreedy.py asserts it), distinct values lie a relative 1e-4 or more apart, and equal
    inputs give equal outputs, so the heap orders as the reference's did.  use_length_priority=True
    runs without a model."""
    import acx
    recs = [c for c in _load("vgreedy_search.json") if c["name"].split("-")[0] in group.split()]
    assert len(recs) >= 2
    zero, one = np.zeros(14, np.float32), np.ones(14, np.float32)
    for c in recs:
        fn = (Y.SCORERS if c["arch"] == "mlp" else Y.TOKEN_SCORERS)[c["scorer"]][1]
        mean, std = (Y.NORM_MEAN, Y.NORM_STD) if c["norm"] else (zero, one) if c["arch"] == "mlp" else (None, None)
        args = dict(max_nodes_to_explore=c["budget"], device=DEV, cyclically_reduce_after_moves=c["cyclical"],
                    use_length_priority=c["length_priority"])
        model = None if c["length_priority"] else _FnModel(fn).to(DEV)
        p = np.array(c["presentation"], np.int8)
        if c["raises"]:
            with pytest.raises(AssertionError, match="invalid presentation"):
                acx.value_guided_greedy_search(p, model, c["arch"], mean, std, **args)
            continue
        ok, path, stats = acx.value_guided_greedy_search(p, model, c["arch"], mean, std, **args)
        assert (ok, [list(x) for x in path], stats) == (c["ok"], c["path"], dict(nodes_explored=c["nodes_explored"],
                                                                                 min_length=c["min_length"])), c


# ---------------------------------------------------------------------------------------------
# against the yardstick; its shape report asserts that the inputs are not vacuous
# ---------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _yard(key, scorer, budget, cyc=False):
    return Y.vgreedy(np.frombuffer(key, np.int32), scorer, budget, cyc, drop_twins=True)


def _against_yardstick(pres, scorer, budgets, cyc=False, **kw):
    res, st = _many(pres, scorer, budgets, cyc, on_error="return", **kw)
    ys = [_yard(_key(p), scorer, int(b), cyc) for p, b in zip(pres, budgets)]
    for i, y in enumerate(ys):
        _check_yardstick(res, st, i, y, (scorer, i, budgets[i], cyc))
    return ys, st


@pytest.mark.parametrize("L", [16, 17, 32, 33, 48, 49, 64, 65])
def test_key_word_counts_against_yardstick(L):
    """one L on each side of every key-word count that by_nw distinguishes; S2 and S4 tie every score,
    so depth and node id alone order the heap; S3 prefers longer words, so its pops run into the
    length gate (children of refused moves are duplicates of their parent)"""
    rng = np.random.default_rng(500 + L)
    pres = np.stack([_pad(AK3, L), _scrambled(L, rng, 6), _scrambled(L, rng, 9), _pad(AK3[::-1], L, 6)])
    budgets = [300, 400, 1, 257]
    ys = []
    for scorer, cyc in (("S0", False), ("S1", True), ("S2", False), ("S4", True), ("S3", False)):
        y, _ = _against_yardstick(pres, scorer, budgets, cyc)
        ys += [(scorer, v) for v in y]
    assert any(v["id_ties"] >= 10 for s, v in ys if s in ("S2", "S4"))
    assert any(v["empty_pops"] for s, v in ys if s == "S3") and any(v["overshoot"] >= 2 for _, v in ys)
    assert {v["status"] for _, v in ys} >= {Y.FOUND, Y.BUDGET}


def test_all_tie_scorers_give_one_search():
    """-0.0 ties with +0.0: S4's searches are S2's"""
    pres = np.stack([_pad(AK3, 18)] + list(_dataset_rows()[::60]))
    budgets = [500 + 7 * i for i in range(len(pres))]
    assert _same(_many(pres, "S2", budgets), _many(pres, "S4", budgets))


# The heap's levels hold 1, 64 and 4,096 entries, so 65 | 66 and 4,161 | 4,162 entries are the
# boundaries at which the take's sift-down and the push's sift-up gain a level.  What counts is the
# heap the engine holds: the one a pop takes its entry from, and the one a push leaves when the
# search goes on (the push of a pop that ends on its budget is never carried out).  Budgets found
# with the yardstick: (scorer, budget, the largest heap popped from, pops from a heap above the
# boundary at least)
LEVEL_CASES = [("S1", 74, 65, 2, 0), ("S0", 74, 66, 2, 1), ("S0", 300, None, 2, 20),
               ("S1", 4906, 4160, 3, 0), ("S1", 4950, 4193, 3, 11), ("S1", 6000, 5057, 3, 194)]


def test_heaps_on_both_sides_of_the_heap_levels():
    p = _pad(AK3, 18)
    for scorer, budget, largest, level, above in LEVEL_CASES:
        (y,), _ = _against_yardstick(p[None], scorer, [budget])
        assert largest is None or y["max_popped"] == largest, (scorer, budget, y["max_popped"])
        assert y["level_pops"][level] >= above and (above > 0 or y["level_pops"][level:] == [0] * (4 - level)), (
            scorer, budget, y["level_pops"])
        assert above == 0 or y["level_pushes"][level] >= above - 1, (scorer, budget, y["level_pushes"])
    (y,), _ = _against_yardstick(np.array([[1, 1, 2, 2]], np.int32), "S0", [100])  # the root alone, then nothing
    assert y["level_pops"] == [1, 0, 0, 0] and y["status"] == Y.EXHAUSTED


def test_same_child_twice_in_one_pop():
    groups = {}
    for p, s, b, cyc in Y.twin_cases():
        groups.setdefault((len(p), s, cyc), []).append((p, b))
    for (_, s, cyc), rows in groups.items():
        ys, _ = _against_yardstick(np.stack([r[0] for r in rows]), s, [r[1] for r in rows], cyc)
        assert all(y["twin_pops"] for y in ys), (s, cyc)


def test_a_step_without_candidates_while_searches_are_live():
    """three copies of a search whose pops find no new child (S3), next to one that ends at once: at
    such a pop M == 0 with three searches live, no scorer call is made and the loop goes on"""
    calls = []

    def s3(f):
        calls.append(len(f))
        return Y.SCORERS["S3"][1](f)

    p = _pad(AK3, 18)
    pres = np.stack([p, p, p, _pad([1, 2], 18, 1)])  # (the last: a trivial child of the root)
    res, st = _many(pres, s3, [400, 400, 400, 400])
    y = _yard(_key(p), "S3", 400)
    for i in range(3):
        _check_yardstick(res, st, i, y, i)
    assert res[3][0] and st["steps"][3] == 1
    mid = [k for k in y["empty_pops"] if k < y["steps"]]
    assert len(mid) >= 10 and calls == [3 * c for c in y["cands"] if c]  # the empty pops made no call


def test_per_row_budgets_and_raising_rows():
    import acx
    """the fixture's raising rows of L = 6 next to rows that search on, each with its own budget"""
    recs = [c for c in _load("vgreedy_search.json") if c["name"] == "raise" and c["L"] == 6 and not c["cyclical"]]
    assert recs
    rng = np.random.default_rng(9)
    rows = [np.array(c["presentation"], np.int32) for c in recs] + [_scrambled(6, rng, 5 + i) for i in range(6)]
    budgets = [500] * len(recs) + [1, 2, 13, 50, 200, 1]
    ys, st = _against_yardstick(np.stack(rows), "S0", budgets)
    assert any(y["raises"] for y in ys) and any(y["status"] == Y.BUDGET and b == 1 for y, b in zip(ys, budgets))
    assert len({y["status"] for y in ys}) >= 3
    with pytest.raises(AssertionError, match=r"invalid presentation .* in searches \["):
        acx.value_guided_greedy_search_many(np.stack(rows), Y.SCORERS["S0"][1], max_nodes_to_explore=budgets, device=DEV)


def test_more_searches_than_resident_workgroups():
    rows = _dataset_rows()
    N = 4096
    res, st = _many(rows[np.arange(N) % len(rows)], "S0", 100)
    for i in range(len(rows), N):  # identical rows, identical results
        j = i % len(rows)
        assert res[i] == res[j] and all(st[k][i] == st[k][j] for k in st), i
    for j in range(len(rows)):
        _check_yardstick(res, st, j, _yard(_key(rows[j]), "S0", 100), j)


def test_split_call_equals_unsplit_call():
    from acx import _lib
    from acx.search import _batch_vgreedy as V
    pres, budgets = _solvable()
    whole = _many(pres, "S1", budgets)
    V.release_workspaces()
    per = _lib.load().acx_vgreedy_bytes(18, max(budgets))
    split = _many(pres, "S1", budgets, workspace_bytes=7 * per + per // 2)  # groups of 7: 5 full, one of 5
    assert V._HANDLES[(0, 18, False)][1] == 7
    assert _same(split, whole)
    assert _same(_many(pres, "S1", budgets, workspace_bytes=1), whole)  # never less than one search per call
    assert any(r[0] for r in whole[0]) and not all(r[0] for r in whole[0])


def test_cached_handle_gives_what_a_fresh_one_gives():
    from acx.search import _batch_bfs
    from acx.search import _batch_vgreedy as V
    pres, budgets = _solvable()
    first, second = (pres[:20], budgets[:20]), (pres[20:][::-1].copy(), budgets[20:][::-1])
    V.release_workspaces()
    _many(first[0], "S0", first[1])
    h = dict(V._HANDLES)
    assert len(h) == 1
    again = _many(second[0], "S0", second[1])
    assert V._HANDLES == h  # the same workspace
    _batch_bfs.release_workspaces()  # frees these workspaces too
    assert not V._HANDLES
    fresh = _many(second[0], "S0", second[1])
    assert _same(again, fresh)
    for i in range(len(second[0])):
        _check_yardstick(fresh[0], fresh[1], i, _yard(_key(second[0][i]), "S0", second[1][i]), i)
    for _ in range(70):  # past the wrap of the table's 6-bit epoch
        _many(first[0][:4], "S0", 60)
    assert _same(_many(second[0], "S0", second[1]), fresh)
    V.release_workspaces()


def test_tokens_scorer():
    """scorer_input="tokens": int64 (M, 2L) ids, letter + 2; their sum is exact in float32"""
    seen = []

    def on_tokens(t):
        seen.append((t.dtype, t.shape[1], int(t.min()), int(t.max())))
        return t.sum(1).to(torch.float32)

    def on_states(s):
        return (np.asarray(s, np.int64) + 2).sum(1).astype(np.float32)

    pres = _dataset_rows()[::20]
    budgets = [150 + 10 * i for i in range(len(pres))]
    res, st = _many(pres, on_tokens, budgets, scorer_input="tokens")
    assert seen and all(s[:2] == (torch.int64, 36) and 0 <= s[2] and s[3] <= 4 for s in seen)
    for i in range(len(pres)):
        _check_yardstick(res, st, i, Y.vgreedy(pres[i], on_states, budgets[i], on_states=True, drop_twins=True), i)
    assert st["steps"].min() >= 3
    ys, _ = _against_yardstick(pres, "TOK", budgets, True)
    assert any(y["id_ties"] for y in ys)


def test_nan_scorer_raises_and_leaves_the_handle_usable():
    import acx
    from acx.search import _batch_vgreedy as V
    pres = np.array([[1, 0, 0, 0, 0, 0, 0, 2, 0, 0, 0, 0, 0, 0], AK2, AK2])  # row 0 is found before any scoring
    V.release_workspaces()
    want = _many(pres, "S1", 3000)
    h = dict(V._HANDLES)
    calls = []

    def nan(f):
        calls.append(len(f))
        return f[:, 0] * float("nan")

    with pytest.raises(ValueError, match=r"NaN in searches \[1, 2\]"):
        acx.value_guided_greedy_search_many(pres, nan, max_nodes_to_explore=3000, device=DEV)
    assert calls == [12] and V._HANDLES == h  # the NaN is sticky: one scorer call, both searches ended
    res, st = acx.value_guided_greedy_search_many(pres[:1], nan, device=DEV, return_stats=True)  # (never scored)
    assert res[0][0] and st["status"][0] == Y.FOUND
    assert _same(_many(pres, "S1", 3000), want) and want[0][0][0]


def test_scorer_contract_on_a_cached_handle():
    """wrong shapes and a CPU tensor raise ValueError, an exception of the scorer's own reaches the
    caller as it is, (M, 1) float64 is taken as float32; the handle gives a fresh one's results after"""
    import acx
    from acx.search import _batch_vgreedy as V
    pres, budgets = _solvable()
    s1 = Y.SCORERS["S1"][1]
    V.release_workspaces()
    want = _many(pres[:12], "S1", budgets[:12])
    h = dict(V._HANDLES)
    for form in (lambda f: f[:, :2], lambda f: s1(f)[:-1], lambda f: s1(f).cpu(), lambda f: None):
        with pytest.raises(ValueError, match="the scorer must return"):
            acx.value_guided_greedy_search_many(pres[:12], form, max_nodes_to_explore=budgets[:12], device=DEV)
    calls = []

    def broken(f):
        calls.append(len(f))
        if len(calls) == 3:
            raise RuntimeError("the model broke")
        return s1(f)

    with pytest.raises(RuntimeError, match="the model broke"):
        acx.value_guided_greedy_search_many(pres[:12], broken, max_nodes_to_explore=budgets[:12], device=DEV)
    assert len(calls) == 3 and V._HANDLES == h
    assert _same(_many(pres[:12], lambda f: s1(f).to(torch.float64)[:, None], budgets[:12]), want)
    assert _same(_many(pres[:12], "S1", budgets[:12]), want) and V._HANDLES == h
    V.release_workspaces()


@pytest.mark.parametrize("case", range(3))
def test_table_scorer_over_the_float_line_against_yardstick(case):
    """heap words from +-inf, +-0.0, +-the smallest denormal, +-FLT_MAX, 1.0 and -1.0 with both their
    neighbours and planted duplicates.  These searches find nothing, and their endings say little
    about the order of the scores; the candidates of a pop do: they are the children of the node the
    heap gave, so every scorer input equals the yardstick's new nodes of that pop exactly when every
    pop took the least (score, depth, id)."""
    p, _, _, cyc = BY.table_cases()[case]
    budget = 2000
    seen = []

    def table(t):
        seen.append(t.cpu().numpy())
        return Y.TOKEN_SCORERS["TABLE"][1](t)

    res, st = _many(p[None], table, budget, cyc, scorer_input="tokens")
    y = Y.vgreedy(p, "TABLE", budget, cyc, drop_twins=True)
    _check_yardstick(res, st, 0, y, (case, budget))
    assert y["score_bits"] == set(BY.TABLE_BITS.tolist()) and y["id_ties"] >= 50 and y["steps"] >= 300
    nodes = np.stack(y["states"]).astype(np.int64) + 2
    bounds = [1] + y["nodes_after"]
    scored = [i for i, c in enumerate(y["cands"]) if c]
    assert len(seen) == len(scored)  # (a pop without candidates is not scored)
    for t, i in zip(seen, scored):
        assert np.array_equal(t, nodes[bounds[i]:bounds[i + 1]]), (case, "pop", i + 1)


# ---------------------------------------------------------------------------------------------
# the C-ABI: refusal statuses, and the calls of a step one by one
# ---------------------------------------------------------------------------------------------
VGREEDY = Engine("acx_vgreedy", "pop", "push", lambda cap: cap + 13)


def _drive(lib, h, states, budgets, L, scorer="S0", short_push_at=None):
    """short_push_at: the step (0-based) whose push is told M - 1 instead of M"""
    return drive(lib, h, VGREEDY, states, budgets, L, Y.SCORERS[scorer][1], short_take_at=short_push_at)


def _check_search(out, i, y):
    _refusals_check_search(out, i, y, ("status", "nodes", "steps", "min_length"))


@pytest.mark.parametrize("L", [13, 36])
def test_refused_searches_through_the_c_abi(L):
    """ACX_MBFS_DOMAIN for a row outside the packed domain, ACX_MBFS_OVERFLOW for a budget above the
    handle's: all-zero outputs, no path, the other searches undisturbed, nothing left behind for the
    handle's next run"""
    from acx import _lib
    lib = _lib.load()
    CAP = 64
    batch, valid = _rows(L)  # rows 1 .. 4 outside the domain, rows 0, 5, 6 the same valid row
    budgets = [40, 40, 40, 40, 40, 65, 40]
    with torch.cuda.device(DEV):
        h = lib.acx_vgreedy_create(L, 7, CAP, 0)
    assert h
    try:
        out = _drive(lib, h, batch, budgets, L)
        want = [0, _lib.MBFS_DOMAIN, _lib.MBFS_DOMAIN, _lib.MBFS_DOMAIN, _lib.MBFS_DOMAIN, _lib.MBFS_OVERFLOW, 0]
        for i, w in enumerate(want):
            if w < 0:
                _refused(out, i, w)
            else:
                _check_search(out, i, Y.vgreedy(batch[i], "S0", budgets[i], drop_twins=True))
        # the epoch: the same handle, seven valid rows -- a refused search left nothing behind
        out = _drive(lib, h, valid, [50] * 7, L)
        ys = [Y.vgreedy(valid[i], "S0", 50, drop_twins=True) for i in range(7)]
        for i, y in enumerate(ys):
            _check_search(out, i, y)
        assert any(y["ok"] and len(y["path"]) >= 2 for y in ys)  # paths are written and walked
    finally:
        lib.acx_vgreedy_destroy(h)


def test_a_push_with_the_wrong_m_ends_the_search_it_cannot_serve():
    """acx_vgreedy_push told M - 1 at the first step: the last search with candidates does not fit,
    and ends with ACX_MBFS_OVERFLOW and all-zero outputs instead of going on without its children;
    the others are undisturbed, and the handle's next run is a fresh one's"""
    from acx import _lib
    lib = _lib.load()
    L = 13
    rows = _thirteen()
    ys = [Y.vgreedy(r, "S0", 50, drop_twins=True) for r in rows]
    last = max(i for i, y in enumerate(ys) if y["cands"] and y["cands"][0] > 0)
    assert last >= 7 and sum(bool(y["cands"]) for y in ys) >= 4
    with torch.cuda.device(DEV):
        h = lib.acx_vgreedy_create(L, len(rows), 64, 0)
    assert h
    try:
        out = _drive(lib, h, rows, [50] * len(rows), L, short_push_at=0)
        for i, y in enumerate(ys):
            if i == last:
                _refused(out, i, _lib.MBFS_OVERFLOW)
            else:
                _check_search(out, i, y)
        out = _drive(lib, h, rows, [50] * len(rows), L)
        for i, y in enumerate(ys):
            _check_search(out, i, y)
    finally:
        lib.acx_vgreedy_destroy(h)
