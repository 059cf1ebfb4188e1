"""CPU side of the batched beam search (acx.beam_search_many, acx.beam_search): the yardstick its
GPU tests rest on (tests/beam_yardstick.py, the reference's beam_search restated over the oracle's
expansion) reproduces the reference's own recorded runs -- tests/golden/beam_search.json
(make_golden_beam.py); the score order the select kernel sorts by (csrc/acx_beam_key.h) is the
floats' own order and Python's stable sort (tests/beam_key_check.cpp, built with the host compiler,
once more under the address and undefined-behaviour sanitizers); the argument checks are made before
any GPU call."""
import os
import struct
import subprocess

import numpy as np
import pytest
import torch

from conftest import PKG_ROOT, REPO

import beam_yardstick as Y
from many_common import _load


@pytest.fixture(scope="module")
def records():
    return _load("beam_search.json")


def _end(r):
    return "raises" if r["raises"] else "found" if r["ok"] else "budget" if r["nodes_explored"] >= max(
        r["budget"], 1) else "died"


def test_the_fixture_covers_what_it_is_for(records):
    by = {}
    for r in records:
        by.setdefault(r["name"].split("-")[0], []).append(r)
    assert {_end(r) for r in by["ak"]} == {"found", "budget", "died"}
    assert {(r["L"], r["cyclical"], r["W"]) for r in by["ak"]} == {(L, c, W) for L in (7, 18) for c in (False, True)
                                                                   for W in (1, 3, 50)}
    assert {r["scorer"] for r in by["ak"]} == {"S0", "S1", "S2", "S3", "S4"}
    assert len(by["ms"]) == 40 and all(r["L"] == 36 for r in by["ms"]) and {"found", "budget"} <= {_end(r) for r in by["ms"]}
    assert len(by["raise"]) >= 3 and all(r["raises"] for r in by["raise"])
    assert any(_end(r) == "found" for r in by["scr"]) and any(r["L"] == 128 for r in by["long"])
    named = {r["name"]: r for r in records}
    assert named["roots-dies"]["steps"] == 1 and _end(named["roots-dies"]) == "died"
    assert named["roots-trivial"]["ok"]
    assert (named["roots-budget1"]["nodes_explored"], named["roots-budget1"]["steps"]) == (1, 0)
    assert {"cut-first", "cut-middle", "cut-last", "cut-before-trivial"} <= set(named)
    # the quoted endings of the issue: AK(2), S1, W = 50 found in 21 steps; AK(2) at W = 1 dies at 64 nodes
    assert any(r["name"] == "ak-AK2" and r["scorer"] == "S1" and r["W"] == 50 and r["ok"] and r["steps"] == 21
               for r in records)
    assert any(r["name"] == "ak-AK2" and r["W"] == 1 and _end(r) == "died" and r["nodes_explored"] == 64
               for r in records)


def test_yardstick_reproduces_every_reference_record(records):
    """paths, nodes_explored and steps; and the budgets named cut-* cut where their names say"""
    for c in records:
        y = Y.beam(np.array(c["presentation"]), c["scorer"], c["W"], c["budget"], c["cyclical"])
        assert y["raises"] == c["raises"], c
        if c["raises"]:
            assert y["status"] == Y.MOVE_ERROR
            continue
        assert (y["ok"], y["path"], y["nodes"], y["steps"]) == (c["ok"], c["path"], c["nodes_explored"], c["steps"]), c
        assert y["status"] == {"found": Y.FOUND, "budget": Y.BUDGET, "died": Y.EXHAUSTED}[_end(c)], c
        if c["name"].startswith("cut-"):
            (_, a, left), = y["cut_at"]
            want = {"cut-first": a == 0, "cut-middle": 0 < a < 11, "cut-last": a == 11, "cut-before-trivial": left > 0}
            assert want[c["name"]], (c["name"], a, left)
    full = Y.beam(np.array(records[0]["presentation"]), "S1", 50, 3000)
    cut = next(c for c in records if c["name"] == "cut-before-trivial")
    assert full["ok"] and cut["budget"] == full["nodes"] and cut["steps"] == full["steps"]  # the success step itself


def test_yardstick_features_are_the_oracle_s():
    from oracle import features as F
    rng = np.random.default_rng(3)
    for L in (3, 18, 40):
        st = np.zeros((200, 2 * L), np.int32)
        for r in st:
            for h in range(2):
                n = int(rng.integers(1, L + 1))
                r[h * L:h * L + n] = rng.choice([1, -1, 2, -2], n)
        assert np.array_equal(Y.features_np(st, L), F.compute_features_batch(st, L))


def test_scorers_agree_between_numpy_and_torch():
    f = Y.features_np(np.array([[1, 2, -1, 0, -2, -2, 1, 0], [1, 0, 0, 0, 2, 0, 0, 0], [1, 1, 1, 0, 2, 0, 0, 0]]), 4)
    for name, (fn, ft) in Y.SCORERS.items():
        a, b = np.asarray(fn(f), np.float32), ft(torch.from_numpy(f)).to(torch.float32).numpy()
        assert a.tobytes() == b.tobytes(), name  # bit for bit: S4's zeros keep their signs


# ---------------------------------------------------------------------------------------------
# real-valued, normalised scores: tests/golden/beam_search_scored.json (make_golden_beam.py --scored)
# ---------------------------------------------------------------------------------------------
def _norm_of(c):
    return dict(mean=Y.NORM_MEAN, std=Y.NORM_STD) if c["norm"] else {}


@pytest.fixture(scope="module")
def scored_runs():
    """(record, the yardstick's run of it) for every record of the scored fixture"""
    return [(c, Y.beam(np.array(c["presentation"]), c["scorer"], c["W"], c["budget"], c["cyclical"], **_norm_of(c)))
            for c in _load("beam_search_scored.json")]


@pytest.fixture(scope="module")
def table_runs():
    return [(W, Y.beam(p, "TABLE", W, budget, cyc)) for p, W, budget, cyc in Y.table_cases()]


def test_the_scored_fixture_covers_what_it_is_for(scored_runs):
    recs = [c for c, _ in scored_runs]
    assert {c["L"] for c in recs} == {7, 18, 36} and sum(c["L"] == 36 for c in recs) >= 12
    assert {(c["arch"], c["scorer"]) for c in recs} == {("mlp", s) for s in Y.NORM_SCORERS} | {("seq", "TOK")}
    assert all(c["norm"] == (c["arch"] == "mlp") for c in recs) and not any(c["raises"] for c in recs)
    assert {c["W"] for c in recs} == {3, 50, 86, 342} and {c["cyclical"] for c in recs} == {False, True}
    assert all(c["budget"] <= (7000 if c["W"] == 342 else 3000) for c in recs)
    assert {_end(c) for c in recs} == {"found", "budget", "died"}
    assert len(set(Y.NORM_MEAN.tolist())) == 14 and len(set(Y.NORM_STD.tolist())) == 14 and (Y.NORM_STD < 0).any()
    # the integer columns: an integer mean and a power-of-two std (their normalised values are dyadic)
    assert (Y.NORM_MEAN[:12] == np.round(Y.NORM_MEAN[:12])).all() and (np.frexp(Y.NORM_STD[:12])[0] == np.sign(
        Y.NORM_STD[:12]) * 0.5).all()


def test_yardstick_reproduces_every_scored_reference_record(scored_runs):
    """the reference's beam_search with the non-trivial mean / std ('mlp') and on token ids ('seq')"""
    for c, y in scored_runs:
        assert not y["raises"], c
        assert (y["ok"], y["path"], y["nodes"], y["steps"]) == (c["ok"], c["path"], c["nodes_explored"], c["steps"]), c
        assert y["status"] == {"found": Y.FOUND, "budget": Y.BUDGET, "died": Y.EXHAUSTED}[_end(c)], c


def test_the_scored_searches_are_not_vacuous(scored_runs, table_runs):
    """by the yardstick's report: in every (scorer, W) group a step selected from more candidates than
    W and some step tied across the W boundary; negative and non-integer scores occurred; the table
    scorer returned every entry of its table, and a step held both zeros"""
    groups = {}
    for c, y in scored_runs:
        groups.setdefault((c["scorer"], c["W"]), []).append(y)
    for W, y in table_runs:
        groups.setdefault(("TABLE", W), []).append(y)
    assert set(groups) == {(s, W) for s in list(Y.NORM_SCORERS) + ["TOK"] for W in (3, 50, 86, 342)} | {
        ("TABLE", W) for W in (50, 86, 342)}
    for (s, W), ys in groups.items():
        assert any(max(y["cands"], default=0) > W for y in ys), (s, W)
    assert sum(bool(y["tie_steps"]) for _, y in scored_runs) >= 10
    for s in list(Y.NORM_SCORERS) + ["TOK", "TABLE"]:
        assert any(y["tie_steps"] for (s2, _), ys in groups.items() if s2 == s for y in ys), s
    for s in Y.NORM_SCORERS:
        v = np.array(sorted(set().union(*(y["score_bits"] for (s2, _), ys in groups.items() if s2 == s for y in ys))),
                     np.uint32).view(np.float32)
        assert len(v) >= 20 and (v != np.round(v)).any(), (s, v)
        # N12 lies in [2, 4], so NMAX is >= 2, and N13 is max / min - 1 >= 0: NNEG brings the negatives
        assert (v < 0).any() == (s == "NNEG") and (s != "NNEG" or (v > 0).any()), (s, v)
    for W, y in table_runs:
        assert y["score_bits"] == set(Y.TABLE_BITS.tolist()) and y["zero_steps"] and y["tie_steps"], W
        assert y["steps"] >= 5


def test_a_skipped_normalisation_changes_the_negative_std_search(scored_runs):
    """NNEG's column 2 has a negative std: without mean / std the same scorer orders the candidates
    differently, and the recorded searches end differently -- so a beam search that dropped the
    normalisation cannot reproduce these records"""
    recs = [(c, y) for c, y in scored_runs if c["scorer"] == "NNEG" and c["L"] >= 18]
    assert len(recs) >= 5
    for c, y in recs:
        raw = Y.beam(np.array(c["presentation"]), "NNEG", c["W"], c["budget"], c["cyclical"])
        assert (raw["ok"], raw["path"], raw["nodes"], raw["steps"]) != (y["ok"], y["path"], y["nodes"], y["steps"]), c


def test_real_valued_scorers_agree_between_numpy_and_torch(scored_runs, table_runs):
    """bit for bit, on the states the searches visited: the normalised features' scorers, the token
    scorer and the table (whose zeros, denormals and infinities keep their bits)"""
    for L in (18, 36):
        st = np.concatenate([np.stack(y["states"]) for c, y in scored_runs if c["L"] == L and c["W"] == 50])[:4000]
        f = Y.normalise_np(Y.features_np(st, L), Y.NORM_MEAN, Y.NORM_STD)
        for name, (fn, ft) in Y.NORM_SCORERS.items():
            a, b = np.asarray(fn(f), np.float32), ft(torch.from_numpy(f)).to(torch.float32).numpy()
            assert a.tobytes() == b.tobytes() and len(np.unique(a)) >= 10, name
        t = st.astype(np.int64) + 2
        for name, (fn, ft) in Y.TOKEN_SCORERS.items():
            a, b = np.asarray(fn(t)), ft(torch.from_numpy(t)).numpy()
            assert a.dtype == b.dtype == np.float32 and a.tobytes() == b.tobytes(), name
        assert set(Y._table_np(t).view(np.uint32).tolist()) == set(Y.TABLE_BITS.tolist())
    v = Y.TABLE
    assert np.isinf(v).sum() == 2 and (v == 0).sum() == 2 and np.float32(1).view(np.uint32) + 1 in Y.TABLE_BITS
    assert np.nextafter(np.float32(-1), np.float32(0)) in v and np.nextafter(np.float32(-1), np.float32(-2)) in v
    assert np.finfo(np.float32).max in v and -np.finfo(np.float32).max in v and len(np.unique(v)) < len(v) - 4


def _build(tmp, flags, name):
    exe = str(tmp / name)
    subprocess.check_call(["g++", "-std=c++17", *flags, "-I", os.path.join(REPO, "include"), "-I",
                           os.path.join(PKG_ROOT, "csrc"), os.path.join(REPO, "tests", "beam_key_check.cpp"), "-o", exe])
    return exe


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    return _build(tmp_path_factory.mktemp("beamkey"), ["-O2"], "beam_key_check")


def test_score_key_order(checker):
    """negatives, denormals, +-0, +-inf pairwise; neighbours over the whole float line; the sort by
    (key, index) against std::stable_sort on 8 x 4000 floats with planted ties"""
    r = subprocess.run([checker, "1"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.startswith("ok"), r.stdout[-2000:]


def test_score_key_order_under_sanitizers(tmp_path):
    exe = _build(tmp_path, ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"], "beam_key_san")
    r = subprocess.run([exe, "2"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.startswith("ok") and "runtime error" not in r.stderr, (r.stdout[-2000:],
                                                                                                   r.stderr[-2000:])


def test_sort_by_key_is_python_s_stable_sort(checker, tmp_path):
    rng = np.random.default_rng(11)
    f = rng.standard_normal(6000).astype(np.float32) * np.float32(10.0) ** rng.integers(-44, 38, 6000).astype(np.float32)
    f[::3] = rng.choice(f[1::3], len(f[::3]))                       # planted ties
    f[5::61] = rng.choice(np.array([0.0, -0.0, np.inf, -np.inf, 1e-45, -1e-45], np.float32), len(f[5::61]))
    assert not np.isnan(f).any() and (f == 0).sum() > 10 and len(np.unique(f)) < 0.8 * len(f)
    bits = [struct.unpack("<I", struct.pack("<f", float(x)))[0] for x in f]
    src, dst = tmp_path / "in.txt", tmp_path / "out.txt"
    src.write_text("\n".join(map(str, bits)) + "\n")
    subprocess.check_call([checker, str(src), str(dst)], timeout=60)
    got = [int(x) for x in dst.read_text().split()]
    assert got == sorted(range(len(f)), key=lambda i: float(f[i]))


GOOD = np.array([[1, 2, 0, -2, 0, 0], [2, 0, 0, 1, 1, 0]])


def _zero(x):
    return x[:, 0]


def test_beam_search_many_refuses_bad_arguments_without_a_gpu():
    import acx
    from acx.search import beam_search, beam_search_many
    assert beam_search_many is acx.beam_search_many and beam_search is acx.beam_search
    assert {"beam_search", "beam_search_many"} <= set(acx.__all__) & set(acx.search.__all__)
    for bad, msg in [([[1, 0, 2, 0], [1, 2, 0, 2, 0, 0]], "equal length"),
                     (np.array([[1, 0, 2], [1, 0, 2]]), "even"),
                     (np.array([[1, 0, 2, 0], [1, 1, 0, 0]]), "not a valid presentation"),
                     (np.array([[1, 0, 2, 0], [3, 0, 2, 0]]), r"letters \+-1 \(x\) and \+-2 \(y\) only")]:
        with pytest.raises(ValueError, match=msg):
            acx.beam_search_many(bad, _zero)
    with pytest.raises(ValueError, match="callable"):
        acx.beam_search_many(GOOD, None)
    with pytest.raises(ValueError, match="sequence of 2"):
        acx.beam_search_many(GOOD, _zero, max_nodes_to_explore=[10, 20, 30])
    with pytest.raises(ValueError, match="beam_search_many supports at most 2\\^24"):
        acx.beam_search_many(GOOD, _zero, max_nodes_to_explore=(1 << 24) + 1)
    with pytest.raises(ValueError, match="sequence of 2"):
        acx.beam_search_many(GOOD, _zero, beam_width=[3])
    for w in (0, -1, 1025, [3, 1025], 2.5, True, [1.5, 2.0]):
        with pytest.raises(ValueError, match="beam_width"):
            acx.beam_search_many(GOOD, _zero, beam_width=w)
    with pytest.raises(ValueError, match="scorer_input"):
        acx.beam_search_many(GOOD, _zero, scorer_input="states")
    with pytest.raises(ValueError, match="both feat_mean and feat_std"):
        acx.beam_search_many(GOOD, _zero, feat_mean=np.zeros(14))
    with pytest.raises(ValueError, match="14 values"):
        acx.beam_search_many(GOOD, _zero, feat_mean=np.zeros(13), feat_std=np.ones(13))
    with pytest.raises(ValueError, match="scorer_input='features'"):
        acx.beam_search_many(GOOD, _zero, scorer_input="tokens", feat_mean=np.zeros(14), feat_std=np.ones(14))
    with pytest.raises(ValueError, match="on_error"):
        acx.beam_search_many(GOOD, _zero, on_error="ignore")
    assert acx.beam_search_many(np.zeros((0, 8), np.int32), _zero) == []  # nothing to search: no GPU call either
    res, stats = acx.beam_search_many(np.zeros((0, 8), np.int32), _zero, return_stats=True)
    assert res == [] and sorted(stats) == ["nodes", "status", "steps"]
    for kw in (dict(solution_cache={}), dict(time_limit=1.0)):
        with pytest.raises(NotImplementedError):
            acx.beam_search(GOOD[0], None, **kw)
    with pytest.raises(ValueError, match="feat_mean"):
        acx.beam_search(GOOD[0], torch.nn.Identity())


def test_beam_workspace_formula_and_argument_checks():
    """acx_beam_bytes states the bytes per search of include/acx.h and DESIGN.md "Batched beam
    search"; every entry point refuses bad arguments before any GPU call."""
    from acx import _lib
    lib = _lib.load()
    for L, B, W in [(1, 1, 1), (12, 50, 3), (18, 2000, 50), (18, 10_000, 1024), (64, 777, 85), (65, 777, 86),
                    (128, 3000, 341), (18, 1 << 24, 342)]:
        kw = _lib.key_words(L)
        want = 8 * kw * B + 4 * B + 64 * ((B + 779 + 3) // 4) + 4 * W + 140 + (6144 * kw if L > 64 else 0)
        assert lib.acx_beam_bytes(L, B, W) == want, (L, B, W)
    for L, B, W in [(0, 10, 3), (129, 10, 3), (18, 0, 3), (18, (1 << 24) + 1, 3), (18, 10, 0), (18, 10, 1025)]:
        assert lib.acx_beam_bytes(L, B, W) < 0
        assert not lib.acx_beam_create(L, 1, B, W, 0)
    assert not lib.acx_beam_create(18, 0, 10, 3, 0) and not lib.acx_beam_create(18, -1, 10, 3, 0)
    lib.acx_beam_destroy(None)
    assert lib.acx_beam_begin(None, None, None, None, 1, None) == _lib.E_ARG
    assert lib.acx_beam_expand(None, None, None) == _lib.E_ARG
    assert lib.acx_beam_gather(None, None, 1, None) == _lib.E_ARG
    assert lib.acx_beam_select(None, None, 1, None) == _lib.E_ARG
    assert lib.acx_beam_finish(None, None, None, None, None, None, None) == _lib.E_ARG
    assert lib.acx_beam_paths(None, 1, None, None, None, 0, None) == _lib.E_ARG
