"""acx.SolutionCache and the solution_cache= argument of acx.value_guided_greedy_search[_many],
acx.beam_search[_many] and acx.mcts_search[_many] on the GPU, against the reference's recorded dicts, lookups and runs
(tests/golden/cache_dicts.npz, cache_search.json: make_golden_cache.py) and, where the fixture has no
record, against the yardstick that reproduces them (tests/cache_yardstick.py, test_cache_cpu.py).
Every comparison is exact: keys, values -- and so which path won a state --, paths, node counts."""
import numpy as np
import pytest
import torch

import cache_yardstick as CY
from oracle import oracle as O
from scored_common import AK3, _FnModel, _pad
from test_cache_cpu import cache_of, dict_of, inputs_of, load_dicts, load_records
from weak_hash_common import ChildDied, run_child, skip_after_death

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
FOUND, BUDGET, CACHED = 1, 2, 4
ENGINES = ["vgreedy", "mcts", "beam"]
STAT = {"vgreedy": "min_length", "mcts": "iterations", "beam": "steps"}  # a record's third stat, and the stats dict's key
BEAM_W = 5  # the beam records' width (make_golden_cache.py)
DEAD = []  # why the weak-hash child died: the tests after it are skipped


@pytest.fixture(autouse=True)
def _one_death_ends_the_module():
    skip_after_death(DEAD)


@pytest.fixture(scope="module")
def z():
    return load_dicts()


def _length(f):
    return f[:, 0]


def _zero(f):
    return f[:, 0] * 0


def _cache(L, capacity=1024):
    import acx
    return acx.SolutionCache(L, DEV, capacity=capacity)


def _same_dict(got, want):
    assert len(got) == len(want) and set(got) == set(want)
    assert all(got[k] == want[k] for k in want)


# ---------------------------------------------------------------------------------------------
# backfill
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("expand", [False, True])
@pytest.mark.parametrize("cyc", [False, True])
def test_backfill_equals_the_reference_dict(z, expand, cyc):
    pres, paths = inputs_of(z, cyc)
    c = _cache(18)
    assert c.backfill_many(pres, paths, cyclically_reduce=cyc, expand_rotations=expand) is c
    want = dict_of(z, f"bf_e{int(expand)}c{int(cyc)}")
    _same_dict(c.to_dict(), want)
    assert len(c) == len(want)


def test_backfill_in_two_calls_and_in_reverse_order(z):
    pres, paths = inputs_of(z, False)
    want, rev = dict_of(z, "bf_e1c0"), dict_of(z, "rev_e1c0")
    c, h = _cache(18), len(paths) // 3
    c.backfill_many(pres[:h], paths[:h])
    c.backfill_many(pres[h:], paths[h:])
    _same_dict(c.to_dict(), want)
    r = _cache(18)
    r.backfill_many(pres[::-1], paths[::-1])
    got = r.to_dict()
    _same_dict(got, rev)
    assert sum(got[k] != want[k] for k in want) >= 3  # the first insertion wins: the order shows
    c.backfill_many(pres[::-1], paths[::-1])  # every state is held already: nothing changes
    _same_dict(c.to_dict(), want)


def test_a_raising_path_leaves_the_cache_unchanged(z):
    pres, paths = inputs_of(z, False)
    c = _cache(18)
    c.backfill_many(pres[:3], paths[:3])
    before = c.to_dict()
    twin = np.zeros(36, np.int32)
    twin[:5] = twin[18:23] = [-2, 1, -2, -1, -2]  # r0 == r1: move 1 empties r0 (utils.py:264-266)
    bad = [(4, 12), (8, 10), (1, 5)]  # a conjugation and its inverse first
    with pytest.raises(AssertionError, match=r"rows \[1, 3\] \(at steps \[2, 0\]\)"):
        c.backfill_many(np.stack([pres[3], twin, pres[4], twin]), [paths[3], bad, paths[4], bad[2:]])
    assert c.to_dict() == before and len(c) == len(before)
    y = {}
    with pytest.raises(AssertionError):  # (the reference keeps what it filled in before the move)
        CY.backfill(y, twin, bad)
    assert len(y) > 0


def test_growth_across_doublings(z):
    """capacity 8 -> at least 1024 rows: every doubling rehashes the entries, codes kept"""
    pres, paths = inputs_of(z, False)
    c, y = _cache(18, capacity=8), {}
    seen = [c.capacity]
    for i in range(0, 6):
        c.backfill_many(pres[i:i + 1], paths[i:i + 1])
        CY.backfill(y, pres[i], paths[i])
        _same_dict(c.to_dict(), y)
        seen.append(c.capacity)
    assert seen[0] == 8 and seen[-1] >= 32 * seen[0] and len(set(seen)) >= 3, seen
    q = np.array(list(y)[::7], np.int8)
    assert c.paths_for(q) == [CY.check(tuple(int(x) for x in s), 18, y)[0] for s in q]
    assert c.nbytes() == (8 * 2 + 8) * c.capacity + 64 * ((c.capacity + 3) // 4) + 16


# ---------------------------------------------------------------------------------------------
# lookup
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag, name", [("q_u", "bf_e0c0"), ("q_e", "bf_e1c0")])
def test_lookup_equals_the_reference(z, tag, name):
    """every fixture state, each with one relator rotated, with both rotated, and with a letter changed"""
    import acx
    d = dict_of(z, name)
    q, want = z["q_states"], dict_of(z, tag, "row")
    c = acx.SolutionCache.from_dict(d, 18, DEV)
    _same_dict(c.to_dict(), d)
    got = c.paths_for(q)
    assert got == [want.get(i) for i in range(len(q))]
    entry, rel, k = c.lookup(q)
    labels = [CY.check(tuple(int(x) for x in s), 18, d) for s in q]
    assert [(int(r), int(kk)) if e >= 0 else None for e, r, kk in zip(entry, rel, k)] == [
        None if lab is None else (lab[1], lab[2]) for lab in labels]
    assert {lab[1:] for lab in labels if lab} >= {(0, 0), (0, 1), (1, 1)}


def _word(rng, n):
    """a freely reduced word of n letters whose ends do not cancel"""
    while True:
        w = [int(rng.choice([1, -1, 2, -2]))]
        while len(w) < n:
            x = int(rng.choice([1, -1, 2, -2]))
            if x != -w[-1]:
                w.append(x)
        if n == 1 or w[0] != -w[-1]:
            return w


def _state(L, r0, r1):
    s = np.zeros(2 * L, np.int32)
    s[:len(r0)], s[L:L + len(r1)] = r0, r1
    return s


@pytest.mark.parametrize("L, n0, n1", [(7, 5, 7), (18, 13, 18), (128, 70, 40), (128, 128, 128)])
def test_shapes_against_the_yardstick(L, n0, n1):
    """one key word (L = 7), a relator that straddles words (18), more variants than lanes (128: a
    hit in the second round of 64, and in the fourth)"""
    import acx
    rng = np.random.default_rng(1000 * L + n0)
    r0, r1 = _word(rng, n0), _word(rng, n1)
    s = _state(L, r0, r1)
    path = [(7, n0 + n1), (0, 2 * n0 + n1), (3, 7)]  # (only the actions are replayed)
    y = CY.backfill({}, s, path)
    c = _cache(L, capacity=16).backfill_many(s[None], [path])
    _same_dict(c.to_dict(), y)
    # the entry alone, met from the state with relator 1 rotated right by k: variant 1 + (n0 - 1) + k
    for k in (1, n1 // 2, n1 - 1):
        d = {tuple(int(x) for x in s): [(5, 9)]}
        q = _state(L, r0, r1[-k:] + r1[:-k])
        want = CY.check(tuple(int(x) for x in q), L, d)
        assert want is not None and want[1:] == (1, k)
        u = acx.SolutionCache.from_dict(d, L, DEV)
        entry, rel, kk = u.lookup(np.stack([q, s, _state(L, r0[1:] + r0[:1], r1[-k:] + r1[:-k])]))
        assert (entry >= 0).tolist() == [True, True, False] and (int(rel[0]), int(kk[0])) == (1, k)
        assert u.paths_for(q[None]) == [want[0]]
        if L == 128:
            assert n0 + k > 64
        res, st = acx.value_guided_greedy_search_many(q[None], _length, 50, device=DEV, solution_cache=u,
                                                      return_stats=True)
        assert res == [(True, want[0])] and (st["status"][0], st["nodes"][0], st["steps"][0]) == (CACHED, 1, 0)


# ---------------------------------------------------------------------------------------------
# the engines
# ---------------------------------------------------------------------------------------------
def _groups(engine, names=None):
    groups = {}
    for r in load_records():
        if r["engine"] == engine and (names is None or r["name"].split("-")[0] in names):
            groups.setdefault((r["L"], r["cyclical"], r["cache"], r["c"]), []).append(r)
    return groups


def _many(engine, recs, cache, **kw):
    import acx
    pres, budgets = np.array([r["presentation"] for r in recs]), [r["budget"] for r in recs]
    if engine == "beam":
        return acx.beam_search_many(pres, _length, BEAM_W, budgets, recs[0]["cyclical"], device=DEV, on_error="return",
                                    return_stats=True, solution_cache=cache, **kw)
    if engine == "vgreedy":
        return acx.value_guided_greedy_search_many(pres, _length, budgets, recs[0]["cyclical"], device=DEV,
                                                   on_error="return", return_stats=True, solution_cache=cache, **kw)
    return acx.mcts_search_many(pres, _zero, budgets, recs[0]["c"], recs[0]["cyclical"], device=DEV, on_error="return",
                                return_stats=True, solution_cache=cache, **kw)


def _check(engine, recs, res, st, without=False):
    steps = STAT[engine]
    for i, r in enumerate(recs):
        if without:
            if r["without"] is None:
                assert res[i] is None, r["name"]
            else:
                assert [res[i][0], [list(m) for m in res[i][1]], st["nodes"][i]] == r["without"], r["name"]
            continue
        if r["raises"]:
            assert res[i] is None and not st["cache_hit"][i], r["name"]
            continue
        got = (res[i][0], [list(m) for m in res[i][1]], st["nodes"][i], st[steps][i], bool(st["cache_hit"][i]))
        assert got == (r["ok"], r["path"], r["nodes_explored"], r[steps], r["cache_hit"]), r["name"]
        assert (st["status"][i] == CACHED) == r["cache_hit"], r["name"]


@pytest.mark.parametrize("engine", ENGINES)
def test_every_record_through_the_batch_call(z, engine):
    import acx
    kinds = set()
    for (L, cyc, name, c), recs in sorted(_groups(engine).items()):
        cache = acx.SolutionCache.from_dict(cache_of(z, name), L, DEV)
        res, st = _many(engine, recs, cache)
        assert sorted(st) == sorted(["status", "nodes", "cache_hit"] + {
            "vgreedy": ["steps", "min_length"], "mcts": ["iterations"], "beam": ["steps"]}[engine])
        _check(engine, recs, res, st)
        mix = {"root" if r["depth"] == 0 else "child" if r["cache_hit"] else "miss" for r in recs if not r["raises"]}
        kinds.add(frozenset(mix))
    assert frozenset({"root", "child", "miss"}) in kinds  # one batch mixes them


@pytest.mark.parametrize("engine", ENGINES)
def test_records_through_the_reference_signature(z, engine):
    """every record but the plain misses of the sequential run, one search per call, the cache an
    acx.SolutionCache (the wrappers refuse a dict: test_cache_cpu.py)"""
    import acx
    zero, one = np.zeros(14, np.float32), np.ones(14, np.float32)
    model = _FnModel(_length if engine == "beam" else _zero).to(DEV)
    n = 0
    for (L, cyc, name, c), recs in sorted(_groups(engine).items()):
        d = cache_of(z, name)
        cache = acx.SolutionCache.from_dict(d, L, DEV)
        for r in recs:
            if r["name"].startswith("seq") and not r["cache_hit"]:
                continue
            p = np.array(r["presentation"], np.int8)
            if engine == "beam":
                call = lambda: acx.beam_search(  # noqa: E731
                    p, model, "mlp", zero, one, beam_width=BEAM_W, max_nodes_to_explore=r["budget"], device=DEV,
                    cyclically_reduce_after_moves=cyc, solution_cache=cache)
                want = dict(nodes_explored=r["nodes_explored"], steps=r.get("steps"))
            elif engine == "vgreedy":
                call = lambda: acx.value_guided_greedy_search(  # noqa: E731
                    p, max_nodes_to_explore=r["budget"], device=DEV, use_length_priority=True,
                    cyclically_reduce_after_moves=cyc, solution_cache=cache)
                want = dict(nodes_explored=r["nodes_explored"], min_length=r.get("min_length"))
            else:
                call = lambda: acx.mcts_search(  # noqa: E731
                    p, model, "mlp", zero, one, max_nodes_to_explore=r["budget"], c_explore=c, device=DEV,
                    cyclically_reduce_after_moves=cyc, solution_cache=cache)
                want = dict(nodes_explored=r["nodes_explored"], iterations=r.get("iterations"))
            n += 1
            if r["raises"]:
                with pytest.raises(AssertionError, match="invalid presentation"):
                    call()
                continue
            if r["cache_hit"]:
                want["cache_hit"] = True
            ok, path, stats = call()
            assert (ok, [list(m) for m in path], stats) == (r["ok"], r["path"], want), r["name"]
    assert n >= 25


@pytest.mark.parametrize("engine", ENGINES)
def test_attach_detach_and_a_dict_on_a_reused_handle(z, engine):
    """the same rows on the same cached handle: with the cache, without it, with it again, and with
    the cache handed over as the reference's dict"""
    import acx
    recs = [r for r in load_records() if r["engine"] == engine and r["cache"] == "U" and not r["cyclical"]]
    assert sum(r["cache_hit"] for r in recs) >= 8
    d = cache_of(z, "U")
    cache = acx.SolutionCache.from_dict(d, 18, DEV)
    _check(engine, recs, *_many(engine, recs, cache))
    res, st = _many(engine, recs, None)
    assert "cache_hit" not in st and CACHED not in st["status"]
    _check(engine, recs, res, st, without=True)
    _check(engine, recs, *_many(engine, recs, cache))
    before = {k: list(v) for k, v in d.items()}
    _check(engine, recs, *_many(engine, recs, d))
    assert d == before
    # the refinement round of the class's docstring: the solved rows are backfilled after the call
    res, st = _many(engine, recs, cache)
    solved = [i for i, r in enumerate(res) if r is not None and r[0]]
    n = len(cache)
    cache.backfill_many(np.array([recs[i]["presentation"] for i in solved]), [res[i][1] for i in solved])
    assert len(cache) > n
    res2, st2 = _many(engine, recs, cache)
    assert all(st2["cache_hit"][i] and st2["nodes"][i] == 1 for i in solved)  # every solved row is a root hit now
    rows = cache._info()["rows"]  # the same rows handed over again, as a second round does: no store row is spent
    cache.backfill_many(np.array([recs[i]["presentation"] for i in solved]), [res[i][1] for i in solved])
    assert cache._info()["rows"] == rows and len(cache) > n


def _beam_vs_yardstick(p, W, budget, d, L):
    import acx
    info = {}
    ok, path, want = CY.beam_length(p, W, budget, False, d, info)
    res, st = acx.beam_search_many(p[None], _length, W, budget, device=DEV, return_stats=True,
                                   solution_cache=acx.SolutionCache.from_dict(d, L, DEV))
    assert res == [(ok, path)] and (st["nodes"][0], st["steps"][0]) == (want["nodes_explored"], want["steps"])
    assert bool(st["cache_hit"][0]) == want.get("cache_hit", False)
    return info, want


def test_beam_hit_in_the_second_pass_and_with_keys_in_scratch(z):
    """a beam of 70: its entries 64 .. 69 are a pass of their own, whose children meet the first
    pass's as nodes; and L = 128, where a pass's child keys, which the probe reads, are not in LDS"""
    pres, paths = inputs_of(z, False)
    second = 0
    for p in pres[:4]:
        info = {}
        CY.beam_length(p, 70, 3000, False, None, info)
        for t in info.get("late", [])[:4]:
            got, want = _beam_vs_yardstick(p.astype(np.int32), 70, 3000, {t: [(1, 9)]}, 18)
            second += want.get("cache_hit", False) and got.get("rank", 0) >= 64
        if second >= 2:
            break
    assert second >= 2
    hits = 0
    for p, path in list(zip(pres, paths))[:3]:
        wide = np.zeros(256, np.int32)
        wide[:18], wide[128:146] = p[:18], p[18:]
        s = wide.copy()
        for m in path[:2]:
            s, _, err = O.move(s, 128, int(m[0]), False)
            assert err == 0
        r1 = s[128:][s[128:] != 0]
        rot = s.copy()
        rot[128:128 + len(r1)] = np.concatenate([r1[-1:], r1[:-1]])
        for key in (s, rot):
            _, want = _beam_vs_yardstick(wide, 5, 600, {tuple(int(x) for x in key): [tuple(m) for m in path[2:]]}, 128)
            hits += want.get("cache_hit", False)
    assert hits >= 3


# ---------------------------------------------------------------------------------------------
# every key-word instantiation of the cached begin and make kernels
# ---------------------------------------------------------------------------------------------
def first_child_case(L):
    """AK(3) padded to L, and a cache of one entry that the child of the root's first eligible action
    a meets through a rotation: -> (root, a, the child's total, the cache's dict, the path
    cache_yardstick.check returns for the child).  The entry's key is the child with relator 1
    rotated left by one letter; a is the first action whose child does not raise, is not trivial
    and is found, while the root and no earlier child raises, is trivial or is found."""
    root = _pad(AK3, L)
    children = [O.move(root, L, a, False) for a in range(12)]
    for a, (child, lens, err) in enumerate(children):
        if err != 0 or sum(lens) == 2:
            continue
        r1 = child[L:][child[L:] != 0]
        key = child.copy()
        key[L:L + len(r1)] = np.concatenate([r1[1:], r1[:1]])
        d = {tuple(int(x) for x in key): [(5, 9)]}
        hit = CY.check(child, L, d)
        if hit is None or CY.check(root, L, d) is not None:
            continue
        if all(e == 0 and sum(ln) != 2 and CY.check(c, L, d) is None for c, ln, e in children[:a]):
            assert hit[1:] == (1, 1) and len(hit[0]) == 2  # one rotation move, then the cached path
            return root, a, sum(lens), d, hit[0]
    raise AssertionError(f"no action of AK(3) at L = {L} has such a child")


def _one(engine, p, cache):
    import acx
    kw = dict(device=DEV, return_stats=True, solution_cache=cache)
    if engine == "beam":
        return acx.beam_search_many(p[None], _length, BEAM_W, 50, False, **kw)
    if engine == "vgreedy":
        return acx.value_guided_greedy_search_many(p[None], _length, 50, False, **kw)
    return acx.mcts_search_many(p[None], _zero, 50, 1.0, False, **kw)


@pytest.mark.parametrize("L", [16, 17, 33, 49, 65])
@pytest.mark.parametrize("engine", ENGINES)
def test_cached_kernels_at_every_key_word_count(engine, L):
    """one L per key-word class (1, 2, 3, 4 and 8 words) and both sides of the first boundary: the
    cached begin kernel misses the root and the cached make kernel hits the first pop's, pass's or
    expansion's child a; then the root itself hits; then the same handle searches without a cache.
    The expectation is oracle.move's and cache_yardstick.check's alone."""
    import acx
    root, a, total, d, tail = first_child_case(L)
    res, st = _one(engine, root, acx.SolutionCache.from_dict(d, L, DEV))
    assert res == [(True, [(a, total)] + tail)]
    assert st["status"][0] == CACHED and bool(st["cache_hit"][0])
    at_root = {tuple(int(x) for x in root): [(5, 9)]}
    res, st = _one(engine, root, acx.SolutionCache.from_dict(at_root, L, DEV))
    assert res == [(True, CY.check(root, L, at_root)[0])] and st["nodes"][0] == 1 and st["status"][0] == CACHED
    res, st = _one(engine, root, None)
    assert "cache_hit" not in st and CACHED not in st["status"]


# ---------------------------------------------------------------------------------------------
# under the colliding hash
# ---------------------------------------------------------------------------------------------
def test_weak_hash(z, tmp_path):
    """backfill in two calls from a capacity of 64 (so it grows), lookup and the value-guided greedy
    search with the cache attached, in a fresh process under libacx_weakhash.so: every probe of the
    cache's table collides, and the dict, the lookups and the searches are the reference's"""
    pres, paths = inputs_of(z, False)
    pres, paths = pres[:6], paths[:6]
    y = {}
    for p, path in zip(pres, paths):
        CY.backfill(y, p, path)
    recs = [r for r in load_records() if r["engine"] == "vgreedy" and r["cache"] == "U" and r["budget"] == 600][:12]
    queries = z["q_states"][::9]
    job = dict(op="cache", L=18, presentations=pres.tolist(), paths=[[list(m) for m in p] for p in paths],
               queries=queries.tolist(), searches=[r["presentation"] for r in recs], budget=150)
    try:
        (out,), _, _ = run_child([job], tmp_path, timeout=240)
    except ChildDied as e:
        DEAD.append(f"test_weak_hash: {e}")
        pytest.fail(DEAD[-1])
    assert out["classes"] == 8 and out["capacity"] > 64
    got = {tuple(k): [tuple(m) for m in v] for k, v in zip(out["keys"], out["values"])}
    _same_dict(got, y)
    assert out["entries"] == len(y)
    want = [CY.check(tuple(int(x) for x in s), 18, y) for s in queries]
    assert out["found"] == [None if w is None else [list(m) for m in w[0]] for w in want] and any(want)
    for i, rec in enumerate(recs):
        ok, path, st = CY.vgreedy_length(rec["presentation"], 150, False, y)
        assert out["results"][i] == [ok, [list(m) for m in path]] and out["nodes"][i] == st["nodes_explored"], rec["name"]
        assert out["cache_hit"][i] == st.get("cache_hit", False)
    assert any(out["cache_hit"])
