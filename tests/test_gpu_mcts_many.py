"""GPU parity of the batched MCTS (acx.mcts_search_many / acx.mcts_search, csrc/acx_mcts.hip: one
wave per search, a step = select, gather, the caller's scorer, backup): given the reference's
values, every search gives the reference's mcts_search result (value_search/mcts.py:177-314) --
against the reference's recorded runs (tests/golden/mcts_search.json, with the reference's own
expm1 values looked up in its tables) and against the yardstick tests/mcts_yardstick.py (checked on
the CPU by test_mcts_cpu.py).  A call has one scorer and one c_explore, so the fixture's records
are grouped by (L, flag, scorer, normalisation, c)."""
import functools
import math

import numpy as np
import pytest
import torch

import mcts_yardstick as Y
import vgreedy_yardstick as YV
from many_common import AK2, _dataset_rows, _load, _norm, _same, _scrambled
from scored_common import AK3, Engine, _FnModel, _key, _pad, _refused, _solvable, _thirteen, drive
from test_gpu_batch_refusals import _check_search as _refusals_check_search
from test_gpu_batch_refusals import _rows

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
def _fn(scorer):
    """a name of Y.MODELS / Y.TOKEN_MODELS: the model's output taken as the value itself (exact in
    float32 on both sides, no expm1), or a function"""
    if not isinstance(scorer, str):
        return scorer, {}
    if scorer in Y.TOKEN_MODELS:
        return Y.model_t(scorer), dict(scorer_input="tokens")
    return Y.model_t(scorer), {}


def _many(pres, scorer, budgets, cyc=False, c=1.41, **kw):
    import acx
    fn, skw = _fn(scorer)
    res, st = acx.mcts_search_many(pres, fn, max_nodes_to_explore=budgets, c_explore=c,
                                   cyclically_reduce_after_moves=cyc, device=DEV, return_stats=True, **skw, **kw)
    assert len(res) == len(pres) and all(len(v) == len(pres) for v in st.values())
    assert sorted(st) == ["iterations", "nodes", "status"]
    return [_norm(r) for r in res], st


def _check_yardstick(res, st, i, y, tag):
    assert res[i] == (None if y["raises"] else [y["ok"], y["path"]]), tag
    if y["raises"]:
        assert st["status"][i] == Y.MOVE_ERROR, tag
        return
    got = (st["status"][i], st["nodes"][i], st["iterations"][i])
    assert got == (y["status"], y["nodes"], y["iterations"]), (tag, got)


def _check_record(res, st, i, c):
    if c["raises"]:
        assert res[i] is None and st["status"][i] == Y.MOVE_ERROR, c
        return
    assert res[i] == [c["ok"], c["path"]], c
    assert (st["nodes"][i], st["iterations"][i]) == (c["nodes_explored"], c["iterations"]), c
    spun = not c["ok"] and c["nodes_explored"] < max(c["budget"], 1)
    assert st["status"][i] == (Y.FOUND if c["ok"] else Y.EXHAUSTED if spun else Y.BUDGET), c


def _record_kw(c):
    return dict(feat_mean=Y.NORM_MEAN, feat_std=Y.NORM_STD) if c["norm"] else {}


@pytest.mark.parametrize("Ls", [(2, 3, 4, 5, 6, 7), (18,), (36, 128)])
def test_every_fixture_record_grouped_into_single_calls(Ls, capsys):
    fx = _load("mcts_search.json")
    assert {c["L"] for c in fx["records"]} <= {2, 3, 4, 5, 6, 7, 18, 36, 128} and len(fx["records"]) >= 100
    groups = {}
    for c in fx["records"]:
        if c["L"] in Ls:
            groups.setdefault((c["L"], c["cyclical"], c["scorer"], c["norm"], c["c"]), []).append(c)
    assert sum(len(g) for g in groups.values()) >= 20
    for (L, cyc, scorer, norm, cx), recs in sorted(groups.items()):
        values = Y.value_fn_t(scorer, fx["tables"][scorer], DEV)
        kw = dict(scorer_input="tokens") if scorer in Y.TOKEN_MODELS else _record_kw(recs[0])
        res, st = _many(np.array([c["presentation"] for c in recs]), values, [c["budget"] for c in recs], cyc, cx,
                        on_error="return", **kw)
        for i, c in enumerate(recs):
            _check_record(res, st, i, c)
    assert capsys.readouterr().out == ""  # mcts_search_many prints nothing


@pytest.mark.parametrize("group", ["ak", "c roots raise long", "ms", "norm"])
def test_fixture_records_through_mcts_search(group):
    """the reference's signature, the model's output through expm1 on the GPU.  Float32 expm1 there
    differs from the reference's by about 1e-7 relative, so only records whose smallest nonzero UCB
    gap is at least 1e-4 relative (or that never compared two UCB scores) are run: a margin of 100 or
    more; equal inputs give equal outputs, so the ties stay ties.  The all-zero and the negative
    model give exact values (0, and anything below 0 clamped to it) and run whatever their gaps."""
    import acx
    recs = [c for c in _load("mcts_search.json")["records"]
            if c["scorer"] in ("MZ", "MN") or c["mingap"] is None or c["mingap"] >= 1e-4]
    assert len(recs) >= 30 and {c["scorer"] for c in recs} >= {"M0", "M1", "MZ", "MN"}
    assert any(c["raises"] for c in recs) and any(c["ok"] and c["path"] for c in recs) and any(c["norm"] for c in recs)
    recs = [c for c in recs if c["name"].split("-")[0] in group.split()]
    assert len(recs) >= 5
    zero, one = np.zeros(14, np.float32), np.ones(14, np.float32)
    for c in recs:
        mean, std = (Y.NORM_MEAN, Y.NORM_STD) if c["norm"] else (zero, one) if c["arch"] == "mlp" else (None, None)
        args = dict(max_nodes_to_explore=c["budget"], c_explore=c["c"], device=DEV,
                    cyclically_reduce_after_moves=c["cyclical"])
        model = _FnModel(Y.model_t(c["scorer"])).to(DEV)
        p = np.array(c["presentation"], np.int8)
        if c["raises"]:
            with pytest.raises(AssertionError, match="invalid presentation"):
                acx.mcts_search(p, model, c["arch"], mean, std, **args)
            continue
        ok, path, stats = acx.mcts_search(p, model, c["arch"], mean, std, **args)
        assert (ok, [list(x) for x in path], stats) == (c["ok"], c["path"], dict(nodes_explored=c["nodes_explored"],
                                                                                 iterations=c["iterations"])), c


# ---------------------------------------------------------------------------------------------
# against the yardstick; its shape report asserts that the inputs are not vacuous
# ---------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _yard(key, scorer, budget, cyc=False, c=1.41):
    return Y.mcts(np.frombuffer(key, np.int32), Y.model_np(scorer), budget, c, cyc, on_tokens=scorer in Y.TOKEN_MODELS)


def _against_yardstick(pres, scorer, budgets, cyc=False, c=1.41, **kw):
    res, st = _many(pres, scorer, budgets, cyc, c, on_error="return", **kw)
    ys = [_yard(_key(p), scorer, int(b), cyc, c) for p, b in zip(pres, budgets)]
    for i, y in enumerate(ys):
        _check_yardstick(res, st, i, y, (scorer, i, budgets[i], cyc, c))
    return ys, st


@pytest.mark.parametrize("L", [16, 17, 32, 33, 48, 49, 64, 65])
def test_key_word_counts_against_yardstick(L):
    """one L on each side of every key-word count that by_nw distinguishes; MZ ties every prior and,
    at c = 0, every UCB score, so action order alone decides"""
    rng = np.random.default_rng(500 + L)
    pres = np.stack([_pad(AK3, L), _scrambled(L, rng, 6), _scrambled(L, rng, 9), _pad(AK3[::-1], L, 6)])
    budgets = [300, 400, 1, 257]
    ys = []
    for scorer, cyc, c in (("M0", False, 1.41), ("M1", True, 1.41), ("MZ", False, 0.0), ("M0", True, 4.0)):
        y, _ = _against_yardstick(pres, scorer, budgets, cyc, c)
        ys += y
    assert sum(y["ucb_sel"] >= 10 for y in ys) >= 8 and any(y["ties"] >= 10 for y in ys)  # the UCB phase
    assert any(y["dead_iters"] for y in ys) and any(y["overshoot"] >= 2 for y in ys)
    assert {y["status"] for y in ys} >= {Y.BUDGET} and any(y["iterations"] == 0 for y in ys)


def test_negative_scorer_gives_the_all_zero_scorers_searches():
    """the clamp max(v, 0): every negative value is the prior 0"""
    pres = np.stack([_pad(AK3, 18)] + list(_dataset_rows()[::60]))
    budgets = [300 + 7 * i for i in range(len(pres))]
    zero = _many(pres, "MZ", budgets)
    assert _same(_many(pres, "MN", budgets), zero)
    assert _same(_many(pres, lambda f: f[:, 0] * 0 - float("inf"), budgets), zero)
    for i in (0, 1):
        _check_yardstick(zero[0], zero[1], i, _yard(_key(pres[i]), "MZ", budgets[i]), i)


def test_a_spinning_search_next_to_live_ones():
    """[1,1,2,2] has no new child: its search backs up dead ends until iterations == 50 * budget --
    1000 is not a multiple of the 64 iterations a launch runs, 1600 is -- with M == 0 from it at
    every step while the other rows search on; dead-end launches make no scorer call"""
    calls = []

    def m0(f):
        calls.append(len(f))
        return Y.model_t("M0")(f)

    pres = np.array([[1, 1, 2, 2], [1, 2, 2, 2], [1, 1, 2, 2], [1, -2, 2, 1], [1, 2, -1, 2]], np.int32)
    budgets = [20, 32, 32, 32, 25]
    res, st = _many(pres, m0, budgets)
    ys = [_yard(_key(p), "M0", b) for p, b in zip(pres, budgets)]
    for i, y in enumerate(ys):
        _check_yardstick(res, st, i, y, i)
    spun = [(y["status"], y["nodes"], y["iterations"]) for y in ys[0:3:2]]
    assert spun == [(Y.EXHAUSTED, 1, 1000), (Y.EXHAUSTED, 1, 1600)]
    assert all(y["scored_iters"] >= 10 and y["dead_iters"] >= 1 for y in ys[1::2] + ys[4:])
    assert sum(calls) == sum(sum(y["cands"]) for y in ys) and len(calls) == max(y["scored_iters"] for y in ys)


def test_a_success_with_a_raising_sibling_is_a_move_error():
    import acx
    pres = np.array([[1, 2, -1, 0, 1, 2, -1, 0], [1, 2, 0, 0, 1, 1, 0, 0]], np.int32)
    ys, st = _against_yardstick(pres, "M0", [100, 100], True)
    assert ys[0]["raises"] and st["status"][0] == Y.MOVE_ERROR and not ys[1]["raises"]
    with pytest.raises(AssertionError, match=r"invalid presentation .* in searches \[0\]"):
        acx.mcts_search_many(pres, Y.model_t("M0"), max_nodes_to_explore=100, cyclically_reduce_after_moves=True,
                             device=DEV)


def test_new_siblings_after_the_success_are_counted():
    """the root's child 2 is trivial and later children are new: nodes_explored counts them all"""
    pres = np.array([[1, 0, 0, 0, 1, 1, 0, 0], [1, 0, 0, 0, -1, -1, 0, 0]], np.int32)
    for cyc, nodes in ((False, [9, 9]), (True, [5, 5])):
        ys, st = _against_yardstick(pres, "M0", [100, 100], cyc)
        assert all(y["ok"] and y["iterations"] == 1 and len(y["path"]) == 1 for y in ys)
        assert st["nodes"].tolist() == nodes
    assert ys[0]["path"][0][0] == 2 and ys[1]["path"][0][0] == 0


def test_same_child_twice_in_one_expansion():
    groups = {}
    for p, s, b, cyc in YV.twin_cases():
        groups.setdefault((len(p), cyc), []).append((p, b))
    for (_, cyc), rows in groups.items():
        for scorer in ("M0", "MZ"):
            ys, _ = _against_yardstick(np.stack([r[0] for r in rows]), scorer, [r[1] for r in rows], cyc)
            assert all(y["twin_expansions"] for y in ys), (scorer, cyc)


@pytest.mark.parametrize("case", range(3))
def test_every_scored_iterations_inputs_against_yardstick(case):
    """the endings say little about a run's selections; the candidates of an iteration do: they are
    the new children of the leaf the descent reached, so every scorer input equals the yardstick's
    new nodes of that iteration exactly when every selection -- least prior, UCB1, the ties -- was
    the reference's"""
    p, scorer, budget, cyc, c = [(_pad(AK3, 18), "M0", 1500, False, 1.41),
                                 (_dataset_rows()[214], "M1", 800, True, 1.41),
                                 (_pad(AK3, 18), "TOK", 1000, True, 4.0)][case]
    seen = []
    fn, skw = _fn(scorer)

    def spy(x):
        seen.append(x.cpu().numpy())
        return fn(x)

    res, st = _many(p[None], spy, budget, cyc, c, scorer_input="tokens" if skw else "features")
    y = _yard(_key(p), scorer, budget, cyc, c)
    _check_yardstick(res, st, 0, y, (case, budget))
    assert y["ucb_sel"] >= 200 and y["ties"] >= 10 and y["mingap"] < 1e-3 and y["deepest"] >= 3
    assert case != 1 or (y["deepest"] >= 30 and y["dead_iters"] >= 100 and y["ucb_sel"] >= 5000)
    assert len(seen) == y["scored_iters"] >= 100
    nodes = np.stack(y["states"])
    for i, x in enumerate(seen):
        rows = nodes[y["cand_ids"][i]:y["cand_ids"][i] + y["cands"][i]]
        want = rows.astype(np.int64) + 2 if skw else Y.features_np(rows, 18)
        assert np.array_equal(x, want), (case, "iteration", i)


def test_the_kernels_ucb_score_bit_for_bit():
    """acx_internal_ucb runs the select kernel's own score routine over arrays: the same bits as
    Python's -(vsum / visit) + c * sqrt(log(N) / visit), for sums that are zero, tiny and huge,
    visit = 1, N = 1 (log 0.0) and large N, at c = 0.0, 1.41 and 4.0"""
    from acx import _lib
    lib = _lib.load()
    rng = np.random.default_rng(7)
    n = 120_000
    visit = rng.integers(1, 5000, n).astype(np.uint32)
    N = np.maximum(visit.astype(np.int64), rng.integers(1, 2_000_000, n))
    vsum = rng.random(n) * visit * rng.choice([0.0, 1e-300, 1e-3, 1.0, 57.25, 1e6, 1e300], n)
    vsum[:1000] = rng.integers(0, 400, 1000) / 16.0  # the fixture's dyadic values
    visit[1000:2000], N[2000:3000], vsum[3000:3500] = 1, 1, 0.0
    N[2000:3000] = np.maximum(N[2000:3000], 1)
    visit[2000:3000] = 1
    logN = np.array([math.log(int(k)) for k in N])
    stream = torch.cuda.current_stream(DEV).cuda_stream
    with torch.cuda.device(DEV):
        s_d, v_d, l_d = (torch.from_numpy(x).to(DEV) for x in (vsum, visit.view(np.int32), logN))
        out = torch.empty(n, dtype=torch.float64, device=DEV)
        for c in (0.0, 1.41, 4.0):
            assert lib.acx_internal_ucb(s_d.data_ptr(), v_d.data_ptr(), l_d.data_ptr(), c, out.data_ptr(), n,
                                        stream) == 0
            got = out.cpu().numpy()
            want = np.array([-(float(s) / int(v)) + c * math.sqrt(float(lg) / int(v))
                             for s, v, lg in zip(vsum.tolist(), visit.tolist(), logN.tolist())])
            assert np.array_equal(got.view(np.uint64), want.view(np.uint64)), (
                c, int((got.view(np.uint64) != want.view(np.uint64)).sum()))
        assert lib.acx_internal_ucb(s_d.data_ptr(), v_d.data_ptr(), l_d.data_ptr(), 1.0, out.data_ptr(), 0, stream) == 0


def test_per_row_budgets_and_raising_rows():
    recs = [c for c in _load("mcts_search.json")["records"]
            if c["name"] == "raise" and c["L"] == 6 and not c["cyclical"]]
    assert recs
    rng = np.random.default_rng(9)
    rows = [np.array(c["presentation"], np.int32) for c in recs] + [_scrambled(6, rng, 5 + i) for i in range(6)]
    budgets = [500] * len(recs) + [1, 2, 13, 50, 200, 0]
    ys, st = _against_yardstick(np.stack(rows), "M0", budgets)
    assert any(y["raises"] for y in ys) and len({y["status"] for y in ys}) >= 3
    assert [y["iterations"] for y in ys[-1:]] == [0]


def test_more_searches_than_resident_workgroups():
    rows = _dataset_rows()
    N = 4096
    res, st = _many(rows[np.arange(N) % len(rows)], "M0", 60)
    for i in range(len(rows), N):  # identical rows, identical results
        j = i % len(rows)
        assert res[i] == res[j] and all(st[k][i] == st[k][j] for k in st), i
    for j in range(0, len(rows), 4):
        _check_yardstick(res, st, j, _yard(_key(rows[j]), "M0", 60), j)


def test_split_call_equals_unsplit_call():
    from acx import _lib
    from acx.search import _batch_mcts as V
    pres, budgets = _solvable()
    whole = _many(pres, "M1", budgets)
    V.release_workspaces()
    per = _lib.load().acx_mcts_bytes(18, max(budgets))
    split = _many(pres, "M1", budgets, workspace_bytes=7 * per + per // 2)  # groups of 7: 5 full, one of 5
    assert V._HANDLES[(0, 18, False)][1] == 7
    assert _same(split, whole)
    assert _same(_many(pres, "M1", budgets, workspace_bytes=1), whole)  # never less than one search per call
    assert any(r[0] for r in whole[0]) and not all(r[0] for r in whole[0])


def test_cached_handle_gives_what_a_fresh_one_gives():
    from acx.search import _batch_bfs
    from acx.search import _batch_mcts as V
    pres, budgets = _solvable()
    first, second = (pres[:20], budgets[:20]), (pres[20:][::-1].copy(), budgets[20:][::-1])
    V.release_workspaces()
    _many(first[0], "M0", first[1])
    h = dict(V._HANDLES)
    assert len(h) == 1
    again = _many(second[0], "M0", second[1])
    assert V._HANDLES == h  # the same workspace
    _batch_bfs.release_workspaces()  # frees these workspaces too
    assert not V._HANDLES and not V._LOG_TABLES
    fresh = _many(second[0], "M0", second[1])
    assert _same(again, fresh)
    for i in range(0, len(second[0]), 3):
        _check_yardstick(fresh[0], fresh[1], i, _yard(_key(second[0][i]), "M0", second[1][i]), i)
    for _ in range(70):  # past the wrap of the table's 6-bit epoch
        _many(first[0][:4], "M0", 40)
    assert _same(_many(second[0], "M0", second[1]), fresh)
    V.release_workspaces()


def test_tokens_scorer():
    """scorer_input="tokens": int64 (M, 2L) ids, letter + 2; an eighth of their sum is exact in float32"""
    seen = []

    def on_tokens(t):
        seen.append((t.dtype, t.shape[1], int(t.min()), int(t.max())))
        return t.sum(1).to(torch.float32) / 8

    def on_np(t):
        return (np.asarray(t, np.int64).sum(1) / 8).astype(np.float32)

    pres = _dataset_rows()[::20]
    budgets = [150 + 10 * i for i in range(len(pres))]
    res, st = _many(pres, on_tokens, budgets, scorer_input="tokens")
    assert seen and all(s[:2] == (torch.int64, 36) and 0 <= s[2] and s[3] <= 4 for s in seen)
    for i in range(len(pres)):
        _check_yardstick(res, st, i, Y.mcts(pres[i], on_np, budgets[i], on_tokens=True), i)
    assert st["iterations"].min() >= 3
    _against_yardstick(pres, "TOK", budgets, True)


def test_nan_and_inf_scores_raise_and_leave_the_handle_usable():
    import acx
    from acx.search import _batch_mcts as V
    pres = np.array([[1, 0, 0, 0, 0, 0, 0, 2, 0, 0, 0, 0, 0, 0], AK2, AK2])  # row 0: a trivial root, found unscored
    V.release_workspaces()
    want = _many(pres, "M1", 3000)
    h = dict(V._HANDLES)
    for bad in (float("nan"), float("inf")):
        calls = []

        def refused(f):
            calls.append(len(f))
            return f[:, 0] * 0 + bad

        with pytest.raises(ValueError, match=r"NaN in searches \[1, 2\]"):
            acx.mcts_search_many(pres, refused, max_nodes_to_explore=3000, device=DEV)
        assert calls == [12] and V._HANDLES == h  # sticky: one scorer call, both searches ended
        res, st = acx.mcts_search_many(pres[:1], refused, device=DEV, return_stats=True)  # (never scored)
        assert res[0] == (True, []) and st["status"][0] == Y.FOUND and st["iterations"][0] == 1
    assert _same(_many(pres, "M1", 3000), want) and want[0][0] == [True, []]


def test_scorer_contract_on_a_cached_handle():
    """wrong shapes and a CPU tensor raise ValueError, an exception of the scorer's own reaches the
    caller as it is, (M, 1) float64 is taken as float32; the handle gives a fresh one's results after"""
    import acx
    from acx.search import _batch_mcts as V
    pres, budgets = _solvable()
    m1 = Y.model_t("M1")
    V.release_workspaces()
    want = _many(pres[:12], "M1", budgets[:12])
    h = dict(V._HANDLES)
    for form in (lambda f: f[:, :2], lambda f: m1(f)[:-1], lambda f: m1(f).cpu(), lambda f: None):
        with pytest.raises(ValueError, match="the scorer must return"):
            acx.mcts_search_many(pres[:12], form, max_nodes_to_explore=budgets[:12], device=DEV)
    calls = []

    def broken(f):
        calls.append(len(f))
        if len(calls) == 3:
            raise RuntimeError("the model broke")
        return m1(f)

    with pytest.raises(RuntimeError, match="the model broke"):
        acx.mcts_search_many(pres[:12], broken, max_nodes_to_explore=budgets[:12], device=DEV)
    assert len(calls) == 3 and V._HANDLES == h
    assert _same(_many(pres[:12], lambda f: m1(f).to(torch.float64)[:, None], budgets[:12]), want)
    assert _same(_many(pres[:12], "M1", budgets[:12]), want) and V._HANDLES == h
    V.release_workspaces()


# ---------------------------------------------------------------------------------------------
# the C-ABI: refusal statuses, and the calls of a step one by one
# ---------------------------------------------------------------------------------------------
MCTS = Engine("acx_mcts", "select", "backup", lambda cap: cap + 50 * cap // 64 + 3, steps="iterations")


def _drive(lib, h, states, budgets, L, scorer="M0", short_backup_at=None, n_log=None, c=1.41):
    """short_backup_at: the step (0-based) whose backup is told M - 1 instead of M; n_log: the
    entries of the log table the select calls are told of (default: all it can need)"""
    logs = torch.tensor([-math.inf] + [math.log(k) for k in range(1, 64 * (MCTS.bound(max(budgets)) + 1) + 2)],
                        dtype=torch.float64, device=DEV)
    return drive(lib, h, MCTS, states, budgets, L, Y.model_t(scorer),
                 make=(logs.data_ptr(), n_log or logs.numel(), c), short_take_at=short_backup_at)


def _check_search(out, i, y):
    _refusals_check_search(out, i, y, ("status", "nodes", "iterations"))


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
        h = lib.acx_mcts_create(L, 7, CAP, 0)
    assert h
    try:
        out = _drive(lib, h, batch, budgets, L)
        want = [0, _lib.MBFS_DOMAIN, _lib.MBFS_DOMAIN, _lib.MBFS_DOMAIN, _lib.MBFS_DOMAIN, _lib.MBFS_OVERFLOW, 0]
        for i, w in enumerate(want):
            if w < 0:
                _refused(out, i, w)
            else:
                _check_search(out, i, Y.mcts(batch[i], Y.model_np("M0"), budgets[i]))
        # the epoch: the same handle, seven valid rows -- a refused search left nothing behind
        out = _drive(lib, h, valid, [50] * 7, L)
        ys = [Y.mcts(valid[i], Y.model_np("M0"), 50) for i in range(7)]
        for i, y in enumerate(ys):
            _check_search(out, i, y)
        assert any(y["ok"] and len(y["path"]) >= 2 for y in ys)  # paths are written and walked
        stream = torch.cuda.current_stream(DEV).cuda_stream
        pair = torch.zeros(2, dtype=torch.int64, device=DEV)
        logs = torch.zeros(8, dtype=torch.float64, device=DEV)
        assert lib.acx_mcts_select(h, logs.data_ptr(), 8, float("nan"), pair.data_ptr(), stream) == _lib.E_ARG
        assert lib.acx_mcts_select(h, None, 8, 1.41, pair.data_ptr(), stream) == _lib.E_ARG
        assert lib.acx_mcts_select(h, logs.data_ptr(), 1, 1.41, pair.data_ptr(), stream) == _lib.E_ARG
    finally:
        lib.acx_mcts_destroy(h)


def test_a_backup_with_the_wrong_m_ends_the_search_it_cannot_serve():
    """acx_mcts_backup told M - 1 at the first step: the last search with candidates does not fit,
    and ends with ACX_MBFS_OVERFLOW and all-zero outputs instead of going on without its priors;
    the others are undisturbed, and the handle's next run is a fresh one's"""
    from acx import _lib
    lib = _lib.load()
    rows = _thirteen()
    ys = [Y.mcts(r, Y.model_np("M0"), 50) for r in rows]
    last = max(i for i, y in enumerate(ys) if y["cands"])
    assert last >= 7 and sum(bool(y["cands"]) for y in ys) >= 4
    with torch.cuda.device(DEV):
        h = lib.acx_mcts_create(13, len(rows), 64, 0)
    assert h
    try:
        out = _drive(lib, h, rows, [50] * len(rows), 13, short_backup_at=0)
        for i, y in enumerate(ys):
            if i == last:
                _refused(out, i, _lib.MBFS_OVERFLOW)
            else:
                _check_search(out, i, y)
        out = _drive(lib, h, rows, [50] * len(rows), 13)
        for i, y in enumerate(ys):
            _check_search(out, i, y)
    finally:
        lib.acx_mcts_destroy(h)


def test_a_log_table_one_entry_too_short_for_one_search():
    """the search that reads the log of the largest visit count N needs log_table[N]; told of a
    table that ends just before it, it ends with ACX_MBFS_OVERFLOW and the others are undisturbed"""
    from acx import _lib
    lib = _lib.load()
    rows = _thirteen()
    budgets = [50] * len(rows)
    budgets[7] = 64
    ys = [Y.mcts(r, Y.model_np("M0"), b) for r, b in zip(rows, budgets)]
    need = [y["max_log_n"] for y in ys]
    top = int(np.argmax(need))
    assert sorted(need)[-1] > sorted(need)[-2] >= 2 and ys[top]["ucb_sel"] >= 5
    with torch.cuda.device(DEV):
        h = lib.acx_mcts_create(13, len(rows), 64, 0)
    assert h
    try:
        out = _drive(lib, h, rows, budgets, 13, n_log=need[top] + 1)  # entries 0 .. need[top]: enough
        for i, y in enumerate(ys):
            _check_search(out, i, y)
        out = _drive(lib, h, rows, budgets, 13, n_log=need[top])
        for i, y in enumerate(ys):
            if i == top:
                assert out["status"][i] == _lib.MBFS_OVERFLOW and out["path_len"][i] == 0
            else:
                _check_search(out, i, y)
    finally:
        lib.acx_mcts_destroy(h)
