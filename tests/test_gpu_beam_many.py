"""GPU parity of the batched beam search (acx.beam_search_many / acx.beam_search, csrc/acx_beam.hip:
one workgroup per search, a step = expand, gather, the caller's scorer, select): with scorers whose
float32 values are exact, every search gives the reference's beam_search result
(value_search/value_guided_search.py:417-561) -- against the reference's recorded runs
(tests/golden/beam_search.json) and against the yardstick tests/beam_yardstick.py (checked on the
CPU by test_beam_cpu.py).  A call has one scorer, so the fixture's records are grouped by
(L, flag, scorer).  The scoring path itself -- normalised features, token ids, scores over the
whole float line, what a scorer may return -- is tested with real-valued scorers against
tests/golden/beam_search_scored.json and the yardstick."""
import functools

import numpy as np
import pytest
import torch

import beam_yardstick as Y
from many_common import AK2, _dataset_rows, _load, _norm, _same, _scrambled
from scored_common import AK3, Engine, _FnModel, _pad, _refused, _solvable, drive
from test_gpu_batch_refusals import _check_search as _refusals_check_search
from test_gpu_batch_refusals import _rows

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
def _many(pres, scorer, W, budgets, cyc=False, **kw):
    import acx
    fn = Y.SCORERS[scorer][1] if isinstance(scorer, str) else scorer
    res, st = acx.beam_search_many(pres, fn, beam_width=W, max_nodes_to_explore=budgets,
                                   cyclically_reduce_after_moves=cyc, device=DEV, return_stats=True, **kw)
    assert len(res) == len(pres) and all(len(v) == len(pres) for v in st.values())
    return [_norm(r) for r in res], st


def _check_yardstick(res, st, i, y, tag):
    assert res[i] == (None if y["raises"] else [y["ok"], y["path"]]), tag
    assert (st["status"][i], st["nodes"][i], st["steps"][i]) == (y["status"], y["nodes"], y["steps"]), tag


def _check_record(res, st, i, c):
    if c["raises"]:
        assert res[i] is None and st["status"][i] == Y.MOVE_ERROR, c
        return
    assert res[i] == [c["ok"], c["path"]], c
    assert (st["nodes"][i], st["steps"][i]) == (c["nodes_explored"], c["steps"]), c
    died = not c["ok"] and c["nodes_explored"] < max(c["budget"], 1)
    assert st["status"][i] == (Y.FOUND if c["ok"] else Y.EXHAUSTED if died else Y.BUDGET), c


@functools.lru_cache(maxsize=None)
def _groups():
    groups = {}
    for c in _load("beam_search.json"):
        groups.setdefault((c["L"], c["cyclical"], c["scorer"]), []).append(c)
    return groups


def test_every_fixture_record_grouped_into_single_calls(capsys):
    groups = _groups()
    assert sum(len(g) for g in groups.values()) >= 120 and {k[0] for k in groups} >= {2, 7, 18, 36, 128}
    for (L, cyc, scorer), recs in sorted(groups.items()):
        res, st = _many(np.array([c["presentation"] for c in recs]), scorer, [c["W"] for c in recs],
                        [c["budget"] for c in recs], cyc, on_error="return")
        for i, c in enumerate(recs):
            _check_record(res, st, i, c)
    assert capsys.readouterr().out == ""  # beam_search_many prints nothing


class _Model(torch.nn.Module):
    def __init__(self, scorer):
        super().__init__()
        self.fn = Y.SCORERS[scorer][1]

    def forward(self, f):
        return self.fn(f)[:, None]


@pytest.mark.parametrize("scorer", ["S0", "S1", "S2"])
def test_fixture_records_through_beam_search(scorer):
    """the reference's signature, the model's output through expm1 on the GPU: these modules' scores
    are integers in [0, 80], which expm1 keeps apart and in order in float32 wherever it is computed"""
    import acx
    recs = [c for c in _load("beam_search.json") if c["scorer"] == scorer and c["L"] <= 36]
    assert len(recs) >= 12 and any(c["raises"] for c in recs) == (scorer != "S2")
    model = _Model(scorer).to(DEV)
    mean, std = np.zeros(14, np.float32), np.ones(14, np.float32)
    for c in recs:
        args = dict(beam_width=c["W"], max_nodes_to_explore=c["budget"], device=DEV,
                    cyclically_reduce_after_moves=c["cyclical"])
        if c["raises"]:
            with pytest.raises(AssertionError, match="invalid presentation"):
                acx.beam_search(np.array(c["presentation"], np.int8), model, "mlp", mean, std, **args)
            continue
        ok, path, stats = acx.beam_search(np.array(c["presentation"], np.int8), model, "mlp", mean, std, **args)
        assert (ok, [list(x) for x in path], stats) == (c["ok"], c["path"], dict(nodes_explored=c["nodes_explored"],
                                                                                 steps=c["steps"])), c


# ---------------------------------------------------------------------------------------------
# widths, key-word counts, per-row widths and budgets: against the yardstick
# ---------------------------------------------------------------------------------------------
# 6 / 22 / 65 entries: 72 children cross a wave, 264 the workgroup, 780 the pass; 85 | 86 and
# 341 | 342 are the select kernel's LDS classes (12 W <= 1024, <= 4096, above)
WIDTH_CALLS = ([1, 5, 6, 21, 22, 64, 65, 85], [86, 341, 7], [342, 1024, 50])


@functools.lru_cache(maxsize=None)
def _width_case(call, scorer):
    """(presentations, budgets, the yardstick's results) of a call: AK(3) and Miller-Schupp rows"""
    widths = WIDTH_CALLS[call]
    rows = _dataset_rows()
    pres = np.stack([rows[(37 * i) % len(rows)] if i % 2 else _pad(AK3, 18) for i in range(len(widths))])
    budgets = [min(20000, 40 + 19 * w + 3 * i) for i, w in enumerate(widths)]
    return pres, budgets, [Y.beam(pres[i], scorer, w, budgets[i]) for i, w in enumerate(widths)]


@pytest.mark.parametrize("scorer", ["S0", "S1"])
@pytest.mark.parametrize("call", range(len(WIDTH_CALLS)))
def test_widths_and_budgets_per_row_against_yardstick(call, scorer):
    widths = WIDTH_CALLS[call]
    pres, budgets, ys = _width_case(call, scorer)
    res, st = _many(pres, scorer, widths, budgets)
    for i, w in enumerate(widths):
        _check_yardstick(res, st, i, ys[i], (scorer, w, budgets[i]))


def test_the_width_cases_are_not_vacuous():
    """by the yardstick's shape report: duplicate children inside one step, a budget cut in the
    middle of a parent, score ties across the W boundary, and at every width a step that selected
    from more candidates than the width"""
    ys = [(w, y) for call in range(len(WIDTH_CALLS)) for scorer in ("S0", "S1")
          for w, y in zip(WIDTH_CALLS[call], _width_case(call, scorer)[2])]
    assert any(y["dup_steps"] for _, y in ys) and any(y["cut_mid"] for _, y in ys) and any(y["tie_steps"] for _, y in ys)
    assert {w for w, y in ys if max(y["cands"], default=0) > w} == {w for c in WIDTH_CALLS for w in c}


@pytest.mark.parametrize("L", [16, 17, 32, 33, 48, 49, 64, 65])
def test_key_word_counts_against_yardstick(L):
    """one L on each side of every key-word count that by_nw distinguishes"""
    rng = np.random.default_rng(500 + L)
    pres = np.stack([_pad(AK3, L), _scrambled(L, rng, 6), _scrambled(L, rng, 9), _pad(AK3[::-1], L, 6)])
    for scorer, cyc in (("S0", False), ("S1", True)):
        budgets = [300, 400, 500, 257]
        res, st = _many(pres, scorer, [22, 5, 65, 3], budgets, cyc)
        for i in range(len(pres)):
            _check_yardstick(res, st, i, Y.beam(pres[i], scorer, [22, 5, 65, 3][i], budgets[i], cyc), (L, scorer, i))


def test_more_searches_than_resident_workgroups():
    rows = _dataset_rows()
    N = 4096
    res, st = _many(rows[np.arange(N) % len(rows)], "S0", 5, 100)
    for i in range(len(rows), N):  # identical rows, identical results
        j = i % len(rows)
        assert res[i] == res[j] and all(st[k][i] == st[k][j] for k in st), i
    for j in range(len(rows)):
        _check_yardstick(res, st, j, Y.beam(rows[j], "S0", 5, 100), j)


def test_split_call_equals_unsplit_call():
    from acx import _lib
    from acx.search import _batch_beam as B
    pres, budgets = _solvable()
    whole = _many(pres, "S1", 7, budgets)
    B.release_workspaces()
    per = _lib.load().acx_beam_bytes(18, max(budgets), 7)
    split = _many(pres, "S1", 7, budgets, workspace_bytes=7 * per + per // 2)  # groups of 7: 5 full, one of 5
    assert B._HANDLES[(0, 18, False)][1] == 7
    assert _same(split, whole)
    assert _same(_many(pres, "S1", 7, budgets, workspace_bytes=1), whole)  # never less than one search per call
    assert any(r[0] for r in whole[0]) and not all(r[0] for r in whole[0])


def test_cached_handle_gives_what_a_fresh_one_gives():
    from acx.search import _batch_beam as B
    from acx.search import _batch_bfs
    pres, budgets = _solvable()
    first, second = (pres[:20], budgets[:20]), (pres[20:][::-1].copy(), budgets[20:][::-1])
    B.release_workspaces()
    _many(first[0], "S0", 7, first[1])
    h = dict(B._HANDLES)
    assert len(h) == 1
    again = _many(second[0], "S0", 7, second[1])
    assert B._HANDLES == h  # the same workspace
    _batch_bfs.release_workspaces()  # frees the beam workspaces too
    assert not B._HANDLES
    fresh = _many(second[0], "S0", 7, second[1])
    assert _same(again, fresh)
    for i in range(len(second[0])):
        _check_yardstick(fresh[0], fresh[1], i, Y.beam(second[0][i], "S0", 7, second[1][i]), i)
    for _ in range(70):  # past the wrap of the table's 6-bit epoch
        _many(first[0][:4], "S0", 7, 60)
    assert _same(_many(second[0], "S0", 7, second[1]), fresh)
    B.release_workspaces()


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
    res, st = _many(pres, on_tokens, 6, budgets, scorer_input="tokens")
    assert seen and all(s[:2] == (torch.int64, 36) and 0 <= s[2] and s[3] <= 4 for s in seen)
    for i in range(len(pres)):
        _check_yardstick(res, st, i, Y.beam(pres[i], on_states, 6, budgets[i], on_states=True), i)
    assert st["steps"].min() >= 3  # the beams were selected by these scores, more than once


def test_nan_scorer_raises_and_leaves_the_handle_usable():
    import acx
    from acx.search import _batch_beam as B
    pres = np.array([[1, 0, 0, 0, 0, 0, 0, 2, 0, 0, 0, 0, 0, 0], AK2, AK2])  # row 0 is found before any scoring
    B.release_workspaces()
    want = _many(pres, "S1", 50, 3000)
    h = dict(B._HANDLES)
    calls = []

    def nan(f):
        calls.append(len(f))
        return f[:, 0] * float("nan")

    with pytest.raises(ValueError, match=r"NaN in searches \[1, 2\]"):
        acx.beam_search_many(pres, nan, beam_width=50, max_nodes_to_explore=3000, device=DEV)
    assert calls and B._HANDLES == h
    assert _same(_many(pres, "S1", 50, 3000), want) and want[0][0][0] and want[0][1][0]


# ---------------------------------------------------------------------------------------------
# real-valued scores: normalised features, token ids, the float line (beam_search_scored.json)
# ---------------------------------------------------------------------------------------------
def _scored_kw(c):
    """how a scored record's scorer reaches beam_search_many: (the torch form, its keyword arguments)"""
    if c["arch"] == "mlp":
        return Y.SCORERS[c["scorer"]][1], dict(feat_mean=Y.NORM_MEAN, feat_std=Y.NORM_STD) if c["norm"] else {}
    return Y.TOKEN_SCORERS[c["scorer"]][1], dict(scorer_input="tokens")


def test_every_scored_record_grouped_into_single_calls():
    """the reference's beam_search with a non-trivial mean / std ('mlp': scores from normalised
    columns, the two ratio columns among them) and on token ids ('seq'), grouped by (L, flag, scorer,
    mean / std): ops.features(keys=, mean=, std=) is the only source of these scores"""
    groups = {}
    for c in _load("beam_search_scored.json"):
        groups.setdefault((c["L"], c["cyclical"], c["arch"], c["scorer"], c["norm"]), []).append(c)
    assert sum(len(g) for g in groups.values()) >= 45 and {k[0] for k in groups} == {7, 18, 36}
    for (L, cyc, arch, scorer, norm), recs in sorted(groups.items()):
        fn, kw = _scored_kw(recs[0])
        res, st = _many(np.array([c["presentation"] for c in recs]), fn, [c["W"] for c in recs],
                        [c["budget"] for c in recs], cyc, **kw)
        for i, c in enumerate(recs):
            _check_record(res, st, i, c)


@pytest.mark.parametrize("arch", ["mlp", "seq"])
def test_scored_records_through_beam_search(arch):
    """the reference's signature: 'mlp' with the real mean / std, and the token branch
    (architecture != 'mlp').  expm1 is strictly increasing over every value these scorers returned
    in the reference's runs (make_golden_beam.py asserts it), and distinct values lie a relative
    1e-4 or more apart (quotients of lengths up to 36, eighths, integers), a thousand float32
    roundings: an expm1 that is a few ulps off orders them the same."""
    import acx
    recs = [c for c in _load("beam_search_scored.json") if c["arch"] == arch]
    assert len(recs) >= 9 and {c["W"] for c in recs} == {3, 50, 86, 342}
    for c in recs:
        fn, _ = _scored_kw(c)
        mean, std = (Y.NORM_MEAN, Y.NORM_STD) if arch == "mlp" else (None, None)
        ok, path, stats = acx.beam_search(np.array(c["presentation"], np.int8), _FnModel(fn).to(DEV), arch, mean, std,
                                          beam_width=c["W"], max_nodes_to_explore=c["budget"], device=DEV,
                                          cyclically_reduce_after_moves=c["cyclical"])
        assert (ok, [list(x) for x in path], stats) == (c["ok"], c["path"], dict(nodes_explored=c["nodes_explored"],
                                                                                 steps=c["steps"])), c


def test_without_its_normalisation_the_negative_std_search_differs():
    """the NNEG records rerun WITHOUT mean / std: the GPU gives the yardstick's un-normalised search,
    which is not the recorded one -- so the records above cannot pass if the normalisation is skipped"""
    recs = [c for c in _load("beam_search_scored.json") if c["scorer"] == "NNEG" and c["L"] == 18 and not c["cyclical"]]
    assert len(recs) >= 2
    res, st = _many(np.array([c["presentation"] for c in recs]), "NNEG", [c["W"] for c in recs],
                    [c["budget"] for c in recs])
    for i, c in enumerate(recs):
        raw = Y.beam(np.array(c["presentation"]), "NNEG", c["W"], c["budget"])
        _check_yardstick(res, st, i, raw, c)
        assert (raw["ok"], raw["path"], raw["nodes"], raw["steps"]) != (c["ok"], c["path"], c["nodes_explored"], c["steps"])


@pytest.mark.parametrize("case", range(3))
def test_table_scorer_over_the_float_line_against_yardstick(case):
    """beam_select_kernel on +-inf, +-0.0, +-the smallest denormal, +-FLT_MAX, 1.0 and -1.0 with both
    their neighbours and planted duplicates, at W = 50, 86 and 342: one per LDS class.  (That every
    entry is returned, that a step holds both zeros and that steps tie across W: test_beam_cpu.py.)"""
    p, W, budget, cyc = Y.table_cases()[case]
    seen = []

    def table(t):
        seen.append(t.cpu().numpy())
        return Y.TOKEN_SCORERS["TABLE"][1](t)

    res, st = _many(p[None], table, W, budget, cyc, scorer_input="tokens")
    y = Y.beam(p, "TABLE", W, budget, cyc)
    _check_yardstick(res, st, 0, y, (W, budget))
    assert y["steps"] >= 5 and max(y["cands"]) > W and y["zero_steps"] and y["tie_steps"]
    # These searches find nothing, and their endings say little about the order of the scores.  The
    # candidates of a step do: they are the children of the beam selected the step before, so every
    # step's scorer input equals the yardstick's new nodes of that step exactly when every
    # selection was the stable sort's.
    nodes = np.stack(y["states"]).astype(np.int64) + 2
    bounds = [1] + y["nodes_after"]
    assert len(seen) == sum(c > 0 for c in y["cands"])  # (a step without candidates is not scored)
    for i, t in enumerate(seen):
        assert np.array_equal(t, nodes[bounds[i]:bounds[i + 1]]), (W, "step", i + 1)


# ---------------------------------------------------------------------------------------------
# the scorer contract (_batch_beam._scores) on a cached handle
# ---------------------------------------------------------------------------------------------
def _contract_batches():
    """(the batch the odd scorers run on, another batch for the handle's next call): same L, the
    second no larger in any dimension, so that the cached handle serves it"""
    pres, budgets = _solvable()
    return (pres[:12], budgets[:12]), (pres[20:30][::-1].copy(), budgets[20:30][::-1])


@pytest.fixture(scope="module")
def contract():
    """the float32 results of both batches, each from a fresh handle"""
    from acx.search import _batch_beam as B
    first, second = _contract_batches()
    B.release_workspaces()
    want = _many(first[0], "S1", 7, first[1])
    B.release_workspaces()
    fresh = _many(second[0], "S1", 7, second[1])
    B.release_workspaces()
    assert any(r[0] for r in want[0]) and any(r[0] for r in fresh[0]) and want[1]["steps"].max() >= 4
    return want, fresh


def _with_cached_handle(run):
    """run(first batch) on a handle a plain call has just cached; then the same handle must give a
    fresh handle's results on the other batch"""
    from acx.search import _batch_beam as B
    first, second = _contract_batches()
    B.release_workspaces()
    _many(first[0], "S1", 7, first[1])
    h = dict(B._HANDLES)
    assert len(h) == 1
    out = run(first)
    assert B._HANDLES == h
    after = _many(second[0], "S1", 7, second[1])
    assert B._HANDLES == h
    B.release_workspaces()
    return out, after


S1_T = Y.SCORERS["S1"][1]  # integers in [0, 80]: exact in float16 too


@pytest.mark.parametrize("form", ["column", "float64", "float16", "float64 column"])
def test_scorer_outputs_taken_as_float32(contract, form):
    """(M, 1), float64 and float16 outputs of an integer-valued scorer give the float32 result"""
    forms = {"column": lambda f: S1_T(f)[:, None], "float64": lambda f: S1_T(f).to(torch.float64),
             "float16": lambda f: S1_T(f).to(torch.float16), "float64 column": lambda f: S1_T(f).to(torch.float64)[:, None]}
    want, fresh = contract
    out, after = _with_cached_handle(lambda b: _many(b[0], forms[form], 7, b[1]))
    assert _same(out, want) and _same(after, fresh)


@pytest.mark.parametrize("form", ["two columns", "one short", "scalar", "cpu", "numpy", "list", "none"])
def test_scorer_outputs_refused(contract, form):
    """a wrong shape, a CPU tensor and a non-tensor each raise ValueError, before anything is
    selected; the handle stays usable"""
    import acx
    forms = {"two columns": lambda f: f[:, :2], "one short": lambda f: S1_T(f)[:-1], "scalar": lambda f: S1_T(f).sum(),
             "cpu": lambda f: S1_T(f).cpu(), "numpy": lambda f: S1_T(f).cpu().numpy(),
             "list": lambda f: S1_T(f).tolist(), "none": lambda f: None}
    calls = []

    def scorer(f):
        calls.append(len(f))
        return forms[form](f)

    def run(b):
        with pytest.raises(ValueError, match="the scorer must return"):
            acx.beam_search_many(b[0], scorer, beam_width=7, max_nodes_to_explore=b[1], device=DEV)

    _, after = _with_cached_handle(run)
    assert len(calls) == 1 and calls[0] > 0 and _same(after, contract[1])


def test_scorer_that_raises_mid_run_propagates(contract):
    """a RuntimeError on the scorer's third call reaches the caller as it is; the searches it
    abandoned between expand and select leave nothing behind for the handle's next run"""
    import acx
    calls = []

    def scorer(f):
        calls.append(len(f))
        if len(calls) == 3:
            raise RuntimeError("the model broke")
        return S1_T(f)

    def run(b):
        with pytest.raises(RuntimeError, match="the model broke"):
            acx.beam_search_many(b[0], scorer, beam_width=7, max_nodes_to_explore=b[1], device=DEV)

    _, after = _with_cached_handle(run)
    assert len(calls) == 3 and _same(after, contract[1])


# ---------------------------------------------------------------------------------------------
# the C-ABI: refusal statuses, and the calls of a step one by one
# ---------------------------------------------------------------------------------------------
BEAM = Engine("acx_beam", "expand", "select", lambda cap: cap + 2, report=lambda M, _: (M, M))


def _drive(lib, h, states, budgets, widths, L, scorer="S0"):
    return drive(lib, h, BEAM, states, budgets, L, Y.SCORERS[scorer][1],
                 begin=(torch.tensor(widths, dtype=torch.int32, device=DEV),))


def _check_search(out, i, y):
    _refusals_check_search(out, i, y, ("status", "nodes", "steps"))


@pytest.mark.parametrize("L", [13, 36])
def test_refused_searches_through_the_c_abi(L):
    """ACX_MBFS_DOMAIN for a row outside the packed domain, ACX_MBFS_OVERFLOW for a budget above the
    handle's and for a width outside [1, max_width]: all-zero outputs, no path, the other searches
    undisturbed, nothing left behind for the handle's next run"""
    from acx import _lib
    lib = _lib.load()
    CAP, WCAP = 64, 8
    batch, valid = _rows(L)  # rows 1 .. 4 outside the domain, rows 0, 5, 6 the same valid row
    batch = np.concatenate([batch, valid[:3]])
    budgets = [40, 40, 40, 40, 40, 65, 40, 40, 40, 40]
    widths = [3, 3, 3, 3, 3, 3, 3, 0, 9, 8]
    with torch.cuda.device(DEV):
        h = lib.acx_beam_create(L, 10, CAP, WCAP, 0)
    assert h
    try:
        out = _drive(lib, h, batch, budgets, widths, L)
        want = [0, _lib.MBFS_DOMAIN, _lib.MBFS_DOMAIN, _lib.MBFS_DOMAIN, _lib.MBFS_DOMAIN, _lib.MBFS_OVERFLOW, 0,
                _lib.MBFS_OVERFLOW, _lib.MBFS_OVERFLOW, 0]
        for i, w in enumerate(want):
            if w < 0:
                _refused(out, i, w)
            else:
                _check_search(out, i, Y.beam(batch[i], "S0", widths[i], budgets[i]))
        # the epoch: the same handle, seven valid rows -- a refused search left nothing behind
        out = _drive(lib, h, valid, [50] * 7, [8, 1, 2, 3, 4, 5, 6], L)
        ys = [Y.beam(valid[i], "S0", [8, 1, 2, 3, 4, 5, 6][i], 50) for i in range(7)]
        for i, y in enumerate(ys):
            _check_search(out, i, y)
        assert any(y["ok"] and len(y["path"]) >= 2 for y in ys)  # paths are written and walked
    finally:
        lib.acx_beam_destroy(h)
