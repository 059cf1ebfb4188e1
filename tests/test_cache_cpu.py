"""CPU side of the solution cache (acx.SolutionCache, the solution_cache= argument of
acx.value_guided_greedy_search[_many], acx.beam_search[_many] and acx.mcts_search[_many]): the yardstick the GPU tests rest on
(tests/cache_yardstick.py, the reference's check / expand / backfill restated over the oracle's move)
reproduces the reference's own recorded dicts, lookups and greedy runs -- tests/golden/cache_dicts.npz
and cache_search.json (make_golden_cache.py); the key algebra the kernels rotate relators with
(csrc/acx_cache.h) agrees with a per-letter restatement (tests/cache_key_check.cpp, built with the
host compiler, once more under the address and undefined-behaviour sanitizers); the bytes formula
holds; the argument checks are made before any GPU call."""
import json
import os
import subprocess

import numpy as np
import pytest

from conftest import PKG_ROOT, REPO

import cache_yardstick as CY

GOLDEN = os.path.join(REPO, "tests", "golden")


def load_dicts():
    return np.load(os.path.join(GOLDEN, "cache_dicts.npz"))


def dict_of(z, name, key="states"):
    """a dict stored as arrays by make_golden_cache.py, in its insertion order"""
    off, act, tot = z[f"{name}_off"], z[f"{name}_act"].tolist(), z[f"{name}_tot"].tolist()
    keys = z[f"{name}_{key}"]
    return {(int(k) if keys.ndim == 1 else tuple(int(x) for x in k)): list(zip(act[off[i]:off[i + 1]], tot[off[i]:off[i + 1]]))
            for i, k in enumerate(keys)}


def inputs_of(z, cyc):
    """(presentations, paths) of the backfills with cyclically_reduce = cyc"""
    return z[f"in_c{int(cyc)}_pres"], list(dict_of(z, f"in_c{int(cyc)}", "pres").values())


def load_records():
    with open(os.path.join(GOLDEN, "cache_search.json")) as f:
        return json.load(f)["records"]


@pytest.fixture(scope="module")
def z():
    return load_dicts()


def test_the_fixture_covers_what_it_is_for(z):
    sizes = {(e, c): len(z[f"bf_e{e}c{c}_states"]) for e in (0, 1) for c in (0, 1)}
    assert sizes[(0, 0)] == 138 and sizes[(1, 0)] == 763 and sizes[(0, 1)] > 100 and sizes[(1, 1)] > sizes[(0, 1)]
    E, rev = dict_of(z, "bf_e1c0"), dict_of(z, "rev_e1c0")
    assert set(E) == set(rev) and sum(E[k] != rev[k] for k in E) >= 3  # the first insertion wins
    recs = load_records()
    for engine in ("vgreedy", "mcts", "beam"):
        mine = [r for r in recs if r["engine"] == engine]
        hits = [r for r in mine if r["cache_hit"]]
        assert {r["depth"] for r in hits} >= {0, 1, 2} and {tuple(r["hit"])[0] for r in hits if r["hit"][1]} == {0, 1}
        assert any(r["name"].endswith("-last") for r in hits) and any(r["raises"] for r in mine)
        assert {r["budget"] for r in hits if r["depth"] == 0} >= {0, 1}
        assert {"miss-found", "miss-budget", "miss-exhausted", "planted-cached-first", "planted-trivial-first",
                "planted-raise-cached-first", "planted-raise-raising-first"} <= {r["name"] for r in mine}
        assert sum(r["without"] is None or r["without"][:2] != [r["ok"], r["path"]] for r in hits) >= 10
    cut, control = ([r for r in recs if r["name"] == n][0] for n in ("cut-beyond", "cut-control"))
    assert cut["engine"] == "beam" and not cut["cache_hit"] and cut["nodes_explored"] == cut["budget"] == 4
    assert control["cache_hit"] and control["presentation"] == cut["presentation"] and control["cache"] == cut["cache"]


def test_yardstick_reproduces_every_backfill(z):
    for cyc in (False, True):
        pres, paths = inputs_of(z, cyc)
        for e in (False, True):
            d = {}
            for p, path in zip(pres, paths):
                CY.backfill(d, p, path, cyc, e)
            want = dict_of(z, f"bf_e{int(e)}c{int(cyc)}")
            assert d == want and list(d) == list(want), (e, cyc)
    pres, paths = inputs_of(z, False)
    d = {}
    for p, path in reversed(list(zip(pres, paths))):
        CY.backfill(d, p, path, False, True)
    assert d == dict_of(z, "rev_e1c0")


def test_yardstick_reproduces_every_lookup(z):
    q = z["q_states"]
    for tag, name in (("q_u", "bf_e0c0"), ("q_e", "bf_e1c0")):
        cache, want = dict_of(z, name), dict_of(z, tag, "row")
        assert 0 < len(want) < len(q)
        for i, s in enumerate(q):
            got = CY.check(tuple(int(x) for x in s), 18, cache)
            assert (None if got is None else got[0]) == want.get(i), (tag, i)


def cache_of(z, name):
    return dict_of(z, {"U": "bf_e0c0", "E": "bf_e1c0", "Uc": "bf_e0c1", "Ec": "bf_e1c1"}.get(name, name))


def test_yardstick_reproduces_every_greedy_record(z):
    recs = [r for r in load_records() if r["engine"] == "vgreedy"]
    assert len(recs) >= 60
    for r in recs:
        cache = cache_of(z, r["cache"])
        if r["raises"]:
            with pytest.raises(AssertionError):
                CY.vgreedy_length(r["presentation"], r["budget"], r["cyclical"], cache)
            continue
        ok, path, st = CY.vgreedy_length(r["presentation"], r["budget"], r["cyclical"], cache)
        assert (ok, [list(m) for m in path], st["nodes_explored"], st["min_length"], st.get("cache_hit", False)) == (
            r["ok"], r["path"], r["nodes_explored"], r["min_length"], r["cache_hit"]), r["name"]
        if r["without"] is not None:
            ok, path, st = CY.vgreedy_length(r["presentation"], r["budget"], r["cyclical"], None)
            assert [ok, [list(m) for m in path], st["nodes_explored"]] == r["without"], r["name"]


def test_yardstick_reproduces_every_beam_record(z):
    recs = [r for r in load_records() if r["engine"] == "beam"]
    assert len(recs) >= 60
    for r in recs:
        cache = cache_of(z, r["cache"])
        if r["raises"]:
            with pytest.raises(AssertionError):
                CY.beam_length(r["presentation"], 5, r["budget"], r["cyclical"], cache)
            continue
        ok, path, st = CY.beam_length(r["presentation"], 5, r["budget"], r["cyclical"], cache)
        assert (ok, [list(m) for m in path], st["nodes_explored"], st["steps"], st.get("cache_hit", False)) == (
            r["ok"], r["path"], r["nodes_explored"], r["steps"], r["cache_hit"]), r["name"]
        if r["without"] is not None:
            ok, path, st = CY.beam_length(r["presentation"], 5, r["budget"], r["cyclical"], None)
            assert [ok, [list(m) for m in path], st["nodes_explored"]] == r["without"], r["name"]


def test_unpack_keys_inverts_the_packing():
    from acx.search import _cache
    from acx.search._engine import _pack_key
    rng = np.random.default_rng(3)
    for L in (1, 7, 16, 18, 32, 33, 128):
        for _ in range(20):
            p = np.zeros(2 * L, np.int64)
            for h in range(2):
                n = int(rng.integers(1, L + 1))
                p[h * L:h * L + n] = rng.choice([1, -1, 2, -2], n)
            assert _cache.unpack_keys(_pack_key(p, L)[None], L)[0].tolist() == p.tolist(), (L, p)


def test_bytes_formula():
    """(8 kw + 8) C + 64 ceil(C / 4) + 16: include/acx.h, DESIGN.md "Solution cache"."""
    import acx  # noqa: F401
    from acx import _lib
    from acx.search import _cache
    lib = _lib.load()
    for L, C, want in ((7, 1, 96), (18, 1024, 40976), (18, 1025, 41064), (36, 1 << 20, 48 * (1 << 20) + 16), (128, 3, 320)):
        kw = (4 * L + 16 + 63) // 64
        assert want == (8 * kw + 8) * C + 64 * ((C + 3) // 4) + 16
        assert lib.acx_cache_bytes(L, C) == want == _cache.cache_bytes(L, C), (L, C)
    for L, C in ((0, 1), (129, 1), (18, 0), (18, (1 << 33) + 1)):
        assert lib.acx_cache_bytes(L, C) < 0
        with pytest.raises(ValueError):
            _cache.cache_bytes(L, C)


def test_argument_checks_without_a_gpu():
    import acx
    assert acx.SolutionCache is acx.search.SolutionCache and "SolutionCache" in acx.__all__
    for bad in (0, 129, 18.0, "18"):
        with pytest.raises(ValueError, match="L must be"):
            acx.SolutionCache(bad)
    with pytest.raises(ValueError, match="capacity"):
        acx.SolutionCache(18, capacity=0)
    c = acx.SolutionCache(2)
    assert len(c) == 0 and c.to_dict() == {} and c.capacity == 1024 and c.nbytes() == 16 * 1024 + 64 * 256 + 16
    assert [x.tolist() for x in c.lookup([[1, 0, 2, 0]])] == [[-1], [0], [0]] and c.paths_for([[1, 0, 2, 0]]) == [None]
    with pytest.raises(ValueError, match="2 presentations but 1 paths"):
        c.backfill_many([[1, 0, 2, 0], [1, 1, 2, 0]], [[(0, 2)]])
    with pytest.raises(ValueError, match="rows of 4 letters"):
        c.backfill_many([[1, 0, 0, 2, 0, 0]], [[(0, 2)]])
    with pytest.raises(ValueError, match="not a valid presentation"):
        c.backfill_many([[0, 1, 2, 0]], [[(0, 2)]])
    with pytest.raises(ValueError, match=r"letters \+-1"):
        c.backfill_many([[3, 0, 2, 0]], [[(0, 2)]])
    with pytest.raises(ValueError, match="pairs"):
        c.backfill_many([[1, 0, 2, 0]], [[0, 2]])
    with pytest.raises(ValueError, match="takes a dict"):
        acx.SolutionCache.from_dict([], 2)
    zero = lambda f: f[:, 0] * 0  # noqa: E731
    good = np.array([[1, 1, 2, 0], [1, 0, 2, 2]])
    for many in (acx.value_guided_greedy_search_many, acx.mcts_search_many, acx.beam_search_many):
        for bad in ([], "cache", 3):
            with pytest.raises(ValueError, match="solution_cache must be"):
                many(good, zero, solution_cache=bad)
        with pytest.raises(ValueError, match="max_relator_length 3"):
            many(good, zero, solution_cache=acx.SolutionCache(3))
        res, st = many(np.zeros((0, 4), np.int32), zero, solution_cache=c, return_stats=True)
        assert res == [] and st["cache_hit"].tolist() == []  # nothing to search: no GPU call either
    for single, model in ((acx.value_guided_greedy_search, None), (acx.mcts_search, object()),
                          (acx.beam_search, object())):
        for bad in ([], 3):
            with pytest.raises(ValueError, match="solution_cache must be"):  # not NotImplementedError
                single(good[0], model, solution_cache=bad)
        with pytest.raises(ValueError, match="max_relator_length 3"):
            single(good[0], model, solution_cache=acx.SolutionCache(3))
        with pytest.raises(NotImplementedError, match="from_dict"):  # the wrappers take no dict: the batch calls do
            single(good[0], model, solution_cache={(1, 0, 2, 0): []})


def _build(tmp, flags, name):
    exe = str(tmp / name)
    subprocess.check_call(["g++", "-std=c++17", *flags, "-I", os.path.join(REPO, "include"), "-I",
                           os.path.join(PKG_ROOT, "csrc"), os.path.join(REPO, "tests", "cache_key_check.cpp"), "-o", exe])
    return exe


def test_key_rotation_and_variant_order(tmp_path):
    """every n from 1 to L, every k, both relators, L in {7, 16, 18, 32, 33, 128}, and the skip cases"""
    r = subprocess.run([_build(tmp_path, ["-O2"], "cache_key_check"), "1"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.startswith("ok"), r.stdout[-2000:]


def test_key_rotation_under_sanitizers(tmp_path):
    exe = _build(tmp_path, ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"], "cache_key_san")
    r = subprocess.run([exe, "2"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and r.stdout.startswith("ok") and "runtime error" not in r.stderr, (r.stdout[-2000:],
                                                                                                   r.stderr[-2000:])
