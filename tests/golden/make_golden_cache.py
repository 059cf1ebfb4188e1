"""tests/golden/cache_dicts.npz and tests/golden/cache_search.json: the reference's solution cache
(value_search/value_guided_search.py:100-250) and the reference's value_guided_greedy_search
(:253-414), beam_search (:417-561) and mcts_search (value_search/mcts.py:177-314) run with one, for acx.SolutionCache and
the solution_cache= argument of the batched searches.

    python tests/golden/make_golden_cache.py --reference ROOT

The reference is loaded as make_golden_beam.py loads it; everything runs its own functions on the
CPU.  The greedy runs use use_length_priority=True (no model); the MCTS runs use the all-zero model
MZ of tests/mcts_yardstick.py, whose expm1 is exact, so no table of expm1 values is needed.

cache_dicts.npz holds dicts as arrays -- NAME_states int8 (E, 2L), NAME_off int64 (E + 1), NAME_act
and NAME_tot int32, the values concatenated -- and the inputs of the backfills:
  in_c0 / in_c1   the solved ones of the first 30 of every 20th Miller-Schupp row (L = 18, length
                  priority, budget 600) with cyclically_reduce_after_moves False / True: _pres, and
                  the paths as _off, _act, _tot;
  bf_e{0,1}c{0,1} backfill_solution_cache of those, expand_rotations e, cyclically_reduce c;
  rev_e1c0        the same paths backfilled in reverse order (it differs from bf_e1c0: asserted);
  q_*             lookups: _states, and the reference's _check_cache_with_rotations of each against
                  bf_e0c0 (q_u_*) and bf_e1c0 (q_e_*) as a dict of the rows that hit (_row: their
                  indices);
  pl_*            the planted dicts of the search records below.
cache_search.json: {records: [...]}, a record {engine, name, presentation, L, budget, cyclical,
cache, c, raises, ok, path, nodes_explored, min_length | iterations | steps, cache_hit, hit: [rel, k] or
null, depth: the moves before the state that hit (0: the root), without: the same run with solution_cache=None as [ok, path, nodes_explored]}.

The beam runs use the total length as the model's output (S0; expm1 of it is strictly increasing),
beam width 5; `cut-beyond` is a step whose budget cut falls before a cached child, `cut-control` the
same search with room.  An MCTS record with "a cached state among
the children already visited" cannot exist: a visited state was the root, which is probed, or was a
new child once, when it was probed and would have ended the search.

The generator refuses to write a fixture that lacks any of the cases named in check_not_vacuous."""
import argparse
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
TESTS = os.path.dirname(HERE)
REPO = os.path.dirname(TESTS)
for _p in (HERE, TESTS, REPO, os.path.join(REPO, "ac-solver-caltech_amd")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

from make_golden import PKG_DATA, to_jsonable  # noqa: E402
from make_golden_beam import AK2, load_beam_search  # noqa: E402

L18 = 18
BEAM_W = 5  # the beam records' width
STAT = {"vgreedy": "min_length", "mcts": "iterations", "beam": "steps"}  # an engine's third stat
CONJ_INVERSE = {4: 8, 8: 4, 5: 9, 9: 5, 6: 10, 10: 6, 7: 11, 11: 7}


def dict_arrays(name, d, dtype=np.int8):
    states = np.array([list(k) for k in d], dtype).reshape(len(d), -1)
    off = np.zeros(len(d) + 1, np.int64)
    np.cumsum([len(v) for v in d.values()], out=off[1:])
    flat = [m for v in d.values() for m in v]
    return {f"{name}_states": states, f"{name}_off": off,
            f"{name}_act": np.array([m[0] for m in flat], np.int32), f"{name}_tot": np.array([m[1] for m in flat], np.int32)}


def tup(s):
    return tuple(int(x) for x in s)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True, help="a checkout of the reference project")
    args = ap.parse_args()
    load_beam_search(args.reference)
    import importlib

    import torch
    torch.set_num_threads(1)
    vgs = importlib.import_module("value_search.value_guided_search")
    mcts = importlib.import_module("value_search.mcts")
    ACMove = importlib.import_module("ac_solver.envs.ac_moves").ACMove
    import cache_yardstick as CY

    def move(a, s, cyc=False):
        s = np.array(s, np.int8)
        L = len(s) // 2
        out, _ = ACMove(a, s, L, [int(np.count_nonzero(s[:L])), int(np.count_nonzero(s[L:]))], cyclical=cyc)
        return out

    class MZ(torch.nn.Module):
        def forward(self, f):
            return (f[:, 0] * 0).to(torch.float32)[:, None]

    def greedy(p, budget, cyc, cache):
        return vgs.value_guided_greedy_search(np.array(p, np.int8), max_nodes_to_explore=budget, device="cpu",
                                              use_length_priority=True, cyclically_reduce_after_moves=cyc,
                                              solution_cache=cache)

    def tree(p, budget, cyc, cache, c=1.41):
        return mcts.mcts_search(np.array(p, np.int8), MZ(), "mlp", np.zeros(14, np.float32), np.ones(14, np.float32),
                                max_nodes_to_explore=budget, c_explore=c, device="cpu",
                                cyclically_reduce_after_moves=cyc, solution_cache=cache)

    class S0(torch.nn.Module):  # the total length; expm1 of it is strictly increasing over the integers up to 2L
        def forward(self, f):
            return f[:, 0:1].to(torch.float32)

    def beam(p, budget, cyc, cache, W=BEAM_W):
        return vgs.beam_search(np.array(p, np.int8), S0(), "mlp", np.zeros(14, np.float32), np.ones(14, np.float32),
                               beam_width=W, max_nodes_to_explore=budget, device="cpu",
                               cyclically_reduce_after_moves=cyc, solution_cache=cache)

    ms = np.load(os.path.join(PKG_DATA, "all_presentations.npy"))[::20]
    assert ms.shape[1] == 2 * L18
    out = {}
    # ---- the backfills ------------------------------------------------------------------------
    dicts, inputs = {}, {}
    for cyc in (False, True):
        solved = []
        for p in ms[:30]:
            ok, path, _ = greedy(p, 600, cyc, None)
            if ok:
                solved.append((np.array(p, np.int8), [tup(m) for m in path]))
        inputs[cyc] = solved
        name = f"in_c{int(cyc)}"
        off = np.zeros(len(solved) + 1, np.int64)
        np.cumsum([len(s[1]) for s in solved], out=off[1:])
        flat = [m for s in solved for m in s[1]]
        out.update({f"{name}_pres": np.stack([s[0] for s in solved]), f"{name}_off": off,
                    f"{name}_act": np.array([m[0] for m in flat], np.int32),
                    f"{name}_tot": np.array([m[1] for m in flat], np.int32)})
        for e in (False, True):
            d = {}
            for p, path in solved:
                vgs.backfill_solution_cache(d, p, path, cyclically_reduce=cyc, expand_rotations=e)
            dicts[(e, cyc)] = d
            out.update(dict_arrays(f"bf_e{int(e)}c{int(cyc)}", d))
    U, E = dicts[(False, False)], dicts[(True, False)]
    rev = {}
    for p, path in reversed(inputs[False]):
        vgs.backfill_solution_cache(rev, p, path, cyclically_reduce=False, expand_rotations=True)
    out.update(dict_arrays("rev_e1c0", rev))
    # two paths that share states, and the first one winning: the reversed order gives other values
    assert set(rev) == set(E) and any(rev[k] != E[k] for k in E), "no state that two paths share"
    shared = sum(1 for k in U if sum(1 for p, path in inputs[False] if k in CY.backfill({}, p, path, False, False)) > 1)
    assert shared >= 3, shared
    for (e, cyc), d in dicts.items():  # the yardstick first: what the GPU tests rest on
        y = {}
        for p, path in inputs[cyc]:
            CY.backfill(y, p, path, cyc, e)
        assert y == d and list(y) == list(d), (e, cyc)

    # ---- lookups ------------------------------------------------------------------------------
    rng = np.random.default_rng(5)
    queries = []
    for k in U:
        s = np.array(k, np.int8)
        queries.append(s)
        rot = {}
        for rel in range(2):
            nz = s[rel * L18:(rel + 1) * L18]
            nz = nz[nz != 0]
            r = s.copy()
            if len(nz) > 1:
                kk = int(rng.integers(1, len(nz)))
                r[rel * L18:rel * L18 + len(nz)] = np.concatenate([nz[-kk:], nz[:-kk]])  # rotated right
            rot[rel] = r
            queries.append(r)
        both = rot[0].copy()
        both[L18:] = rot[1][L18:]
        queries.append(both)
        near = s.copy()
        i = int(rng.integers(0, int(np.count_nonzero(s[:L18]))))
        near[i] = {1: 2, -1: -2, 2: 1, -2: -1}[int(near[i])]
        queries.append(near)
    queries = np.unique(np.stack(queries), axis=0)
    out["q_states"] = queries
    for tag, d in (("q_u", U), ("q_e", E)):
        hits = {}
        for i, q in enumerate(queries):
            v = vgs._check_cache_with_rotations(tuple(q), L18, d)
            assert (v is None) == (CY.check(tuple(q), L18, d) is None) and (v is None or v == CY.check(tuple(q), L18, d)[0])
            if v is not None:
                hits[i] = [tup(m) for m in v]
        arr = dict_arrays(tag, {(i,): v for i, v in hits.items()}, np.int64)
        arr[f"{tag}_row"] = arr.pop(f"{tag}_states").reshape(-1)
        out.update(arr)
        labels = {CY.check(tuple(queries[i]), L18, d)[1:] for i in hits}
        assert {(0, 0)} < labels and any(r == 1 for r, _ in labels) and any(r == 0 and k for r, k in labels), labels
        assert 0 < len(hits) < len(queries)

    # ---- searches -----------------------------------------------------------------------------
    caches = {"U": U, "E": E, "Uc": dicts[(False, True)], "Ec": dicts[(True, True)]}
    records = []

    def label(p, cyc, cache, path):
        """which state hit, and how: the root (path == its check), or the child the path's prefix
        reaches -- [rel, k], by the yardstick's check of that state"""
        L = len(p) // 2
        s = np.array(p, np.int8)
        for i in range(len(path) + 1):
            hit = CY.check(tup(s), L, cache)
            if hit is not None and [tup(m) for m in path[i:]] == [tup(m) for m in hit[0]]:
                return [int(hit[1]), int(hit[2])], i
            if i < len(path):
                s = move(path[i][0], s, cyc)
        raise AssertionError("no state of the path explains the hit")

    def run(engine, name, p, budget, cyc, cache_name, c=1.41):
        cache = caches[cache_name]
        fn = {"vgreedy": lambda ch: greedy(p, budget, cyc, ch), "mcts": lambda ch: tree(p, budget, cyc, ch, c),
              "beam": lambda ch: beam(p, budget, cyc, ch)}[engine]
        rec = dict(engine=engine, name=name, presentation=[int(x) for x in p], L=len(p) // 2, budget=int(budget),
                   cyclical=bool(cyc), cache=cache_name, c=float(c))
        before = {k: list(v) for k, v in cache.items()}
        try:
            ok, path, st = fn(cache)
            rec.update(raises=False, ok=bool(ok), path=to_jsonable(path), nodes_explored=int(st["nodes_explored"]),
                       cache_hit=bool(st.get("cache_hit", False)), hit=None, depth=None)
            rec[STAT[engine]] = int(st[STAT[engine]])
            if rec["cache_hit"]:
                rec["hit"], rec["depth"] = label(p, cyc, cache, path)
        except AssertionError:
            rec.update(raises=True, ok=False, path=None, nodes_explored=None, cache_hit=False, hit=None, depth=None)
        assert cache == before, "a search mutated its cache"
        try:
            ok, path, st = fn(None)
            rec["without"] = [bool(ok), to_jsonable(path), int(st["nodes_explored"])]
        except AssertionError:
            rec["without"] = None
        records.append(rec)
        return rec

    def rotated_right(s, rel, k):
        s = np.array(s, np.int8)
        L = len(s) // 2
        nz = s[rel * L:(rel + 1) * L]
        nz = nz[nz != 0]
        r = s.copy()
        r[rel * L:rel * L + len(nz)] = np.concatenate([nz[-k:], nz[:-k]])
        return r

    def parent_of(x, m):
        """the state from which move CONJ_INVERSE[m] gives x back, by stepping back with m; or None"""
        par = move(m, x)
        return par if tup(move(CONJ_INVERSE[m], par)) == tup(x) and tup(par) != tup(x) else None

    entries = [np.array(k, np.int8) for k in U if np.count_nonzero(k) > 6]
    for engine in ("vgreedy", "mcts", "beam"):
        b = 200 if engine == "mcts" else 600
        D = 2 if engine == "beam" else 4  # how deep the planted state of the deep-* cases lies
        # the sequential run of the issue, against the frozen dicts: rows 30 .. 60
        for i, p in enumerate(ms[30:60]):
            run(engine, "seq", p, b, False, "E")
        for i, p in enumerate(ms[30:44]):
            run(engine, "seq-cyc", p, b, True, "Ec")
        for p in ms[30:36]:  # (misses beside the root and child hits below: one batch mixes them)
            run(engine, "seq-u", p, b, False, "U")
        # root hits: direct, rotated (the unexpanded cache), at budgets 0 and 1
        e0 = entries[3]
        for name, p, budget in (("root-direct", e0, b), ("root-budget0", e0, 0), ("root-budget1", entries[5], 1),
                                ("root-rot0", rotated_right(entries[7], 0, 2), b),
                                ("root-rot1", rotated_right(entries[9], 1, 3), b)):
            run(engine, name, p, budget, False, "U")
        # child hits by a rotation of each relator: an entry, one relator rotated right by k, then
        # one step back with a conjugation of the other relator that the search undoes
        made = {0: 0, 1: 0, "last": 0}
        for e in entries:
            for rel, back in ((1, 11), (0, 8)):
                n = int(np.count_nonzero(e[rel * L18:(rel + 1) * L18]))
                for kind, k in (("k2", 2), ("last", n - 1)):
                    if n < 4 or made[rel if kind == "k2" else "last"] >= (4 if kind == "k2" else 3):
                        continue
                    x = rotated_right(e, rel, k)
                    par = parent_of(x, back)
                    if par is None or CY.check(tup(par), L18, U) is not None or CY.check(tup(x), L18, U) is None:
                        continue
                    r = run(engine, f"child-rot{rel}-{kind}", par, b, False, "U")
                    if r["cache_hit"] and r["hit"] == [rel, k] and r["depth"] == 1:
                        made[rel if kind == "k2" else "last"] += 1
                    else:
                        records.pop()
        assert made[0] and made[1] and made["last"], made
        # hits below the first pop: a planted dict that holds one state from deep in a solved row's
        # path, as itself and with a relator rotated
        deep = 0
        for j, (p, path) in enumerate(inputs[False]):
            if len(path) < 6 or deep >= 6:
                continue
            s = np.array(p, np.int8)
            for m in path[:D]:
                s = move(m[0], s)
            rel = j % 2
            n = int(np.count_nonzero(s[rel * L18:(rel + 1) * L18]))
            for kind, key in (("direct", s), ("rot", rotated_right(s, rel, 1) if n > 2 else None)):
                if key is None:
                    continue
                name = f"pl_{engine}_deep{j}_{kind}"
                caches[name] = {tup(key): [tup(m) for m in path[D:]]}
                r = run(engine, f"deep-{kind}", p, b, False, name)
                if r["cache_hit"] and r["depth"] > 1:
                    deep += 1
                else:
                    records.pop()
                    del caches[name]
        assert deep >= 2, deep
        # misses: found, on the budget, exhausted (a planted dict that nothing reaches)
        far = {tup(np.array([1, 1, 1, 1, 1, 1, 1] + [2] * 7, np.int8)): [(0, 14)]}
        caches["pl_far7"] = far
        caches["pl_far2"] = {(1, 2, 2, 2): [(0, 4)]}
        caches["pl_far18"] = {tup(np.array([1] * 17 + [0] + [2] * 17 + [0], np.int8)): [(0, 34)]}
        for p, path in inputs[False]:
            if run(engine, "miss-found", p, b, False, "pl_far18")["ok"]:
                break
            records.pop()
        else:  # (mcts with the all-zero model finds none of them: one step before the end, then)
            p, path = inputs[False][0]
            s = np.array(p, np.int8)
            for m in path[:-1]:
                s = move(m[0], s)
            run(engine, "miss-found", s, b, False, "pl_far18")
        run(engine, "miss-budget", AK2, 37, True, "pl_far7")
        run(engine, "miss-exhausted", [1, 1, 2, 2], 100 if engine == "vgreedy" else 6, False, "pl_far2")
        if engine == "beam":  # a cached child beyond the step's budget cut, and the same cache with room
            p = inputs[False][0][0]
            kids = [move(a, p) for a in range(12)]
            seen, new = {tup(p)}, []
            for a in range(12):
                if tup(kids[a]) not in seen:
                    seen.add(tup(kids[a]))
                    new.append(a)
            j = new[2]  # budget 4: total_nodes reaches 4 at the third new child
            a = next(a for a in new if a > j and np.count_nonzero(kids[a]) > 2
                     and all(CY.check(tup(x), L18, {tup(kids[a]): []}) is None for x in [p] + kids[:j + 1]))
            caches["pl_beam_cut"] = {tup(kids[a]): [(2, 55)]}
            run(engine, "cut-beyond", p, 4, False, "pl_beam_cut")
            run(engine, "cut-control", p, b, False, "pl_beam_cut")
        # a trivial child and a cached child in one pop, both orders: the state before a path's last
        done = set()
        for p, path in inputs[False]:
            s = np.array(p, np.int8)
            for m in path[:-1]:
                s = move(m[0], s)
            t = path[-1][0]
            kids = [move(a, s) for a in range(12)]
            for order, pick in (("cached-first", range(0, t)), ("trivial-first", range(t + 1, 12))):
                a = next((a for a in pick if np.count_nonzero(kids[a]) > 2
                          and CY.check(tup(s), L18, {tup(kids[a]): []}) is None), None)
                if a is None or order in done:
                    continue
                name = f"pl_{engine}_{order}"
                caches[name] = {tup(kids[a]): [(0, 99), (1, 98)]}
                run(engine, f"planted-{order}", s, b, False, name)
                done.add(order)
        assert done == {"cached-first", "trivial-first"}, done
        # a raising child and a cached child in one pop, both orders
        with open(os.path.join(HERE, "kat_search_extra.json")) as f:
            raising = [c for c in json.load(f) if c["raises"] and not c["cyclical"]]
        done = set()
        for c in raising:
            s = np.array(c["presentation"], np.int8)
            if np.count_nonzero(s) <= 2:  # (a terminal root for mcts.py)
                continue
            kids = []
            for a in range(12):
                try:
                    kids.append(move(a, s))
                except AssertionError:
                    kids.append(None)
            if all(k is not None for k in kids):
                continue
            e = next(a for a in range(12) if kids[a] is None)
            for order, pick in (("cached-first", range(0, e)), ("raising-first", range(e + 1, 12))):
                a = next((a for a in pick if kids[a] is not None and np.count_nonzero(kids[a]) > 2
                          and CY.check(tup(s), len(s) // 2, {tup(kids[a]): []}) is None), None)
                if a is None or order in done:
                    continue
                name = f"pl_{engine}_raise_{order}"
                caches[name] = {tup(kids[a]): [(3, 77)]}
                run(engine, f"planted-raise-{order}", s, b, False, name)
                done.add(order)
        assert done == {"cached-first", "raising-first"}, done

    if os.environ.get("CACHE_GOLDEN_SUMMARY"):
        for r in records:
            print(r["engine"], r["name"], r["cache"], r["raises"], r["ok"], r["cache_hit"], r["hit"], r["depth"],
                  r["nodes_explored"], r["without"] and r["without"][0])
    check_not_vacuous(records)
    for name, d in caches.items():
        if name.startswith("pl_"):
            out.update(dict_arrays(name, d))
    npz, js = os.path.join(HERE, "cache_dicts.npz"), os.path.join(HERE, "cache_search.json")
    np.savez_compressed(npz, **out)
    with open(js, "w") as f:
        json.dump(dict(records=records), f, separators=(",", ":"))
    print(len(records), "records;", {k: len(v) for k, v in dicts.items()}, "entries;", len(queries), "lookups;",
          os.path.getsize(npz), os.path.getsize(js), "bytes")
    assert os.path.getsize(npz) < 200_000 and os.path.getsize(js) < 200_000


def check_not_vacuous(records):
    cut, control = ([r for r in records if r["name"] == n][0] for n in ("cut-beyond", "cut-control"))
    assert not cut["cache_hit"] and not cut["ok"] and cut["nodes_explored"] == 4 and cut["steps"] == 1, cut
    assert control["cache_hit"] and control["depth"] == 1 and control["steps"] == 1, control
    for engine in ("vgreedy", "mcts", "beam"):
        recs = [r for r in records if r["engine"] == engine]
        names = {r["name"] for r in recs}
        by = lambda n: [r for r in recs if r["name"] == n]  # noqa: E731
        hits = [r for r in recs if r["cache_hit"]]
        assert all(r["ok"] and r["cache_hit"] and r["depth"] == 0 for n in ("root-direct", "root-budget0", "root-budget1",
                                                                         "root-rot0", "root-rot1") for r in by(n)), engine
        assert by("root-direct")[0]["hit"] == [0, 0] and by("root-rot0")[0]["hit"][0] == 0 and by("root-rot0")[0]["hit"][1]
        assert by("root-rot1")[0]["hit"][0] == 1 and all(r["nodes_explored"] == 1 for r in hits if r["depth"] == 0)
        assert any(r["depth"] and r["hit"] == [0, 0] for r in hits), (engine, "a child hit, direct")
        assert any(r["depth"] and r["hit"][0] == 0 and r["hit"][1] for r in hits), (engine, "a child hit, relator 0 rotated")
        assert any(r["depth"] and r["hit"][0] == 1 for r in hits), (engine, "a child hit, relator 1 rotated")
        assert any(n.endswith("-last") for n in names), (engine, "a hit at k = n - 1")
        assert any(r["cache_hit"] and r["depth"] > 1 and r["hit"] == [0, 0] for r in by("deep-direct")), engine
        assert any(r["cache_hit"] and r["depth"] > 1 and r["hit"][1] for r in by("deep-rot")), engine
        miss = {n: by(n)[0] for n in ("miss-found", "miss-budget", "miss-exhausted")}
        assert not any(r["cache_hit"] or r["raises"] for r in miss.values()) and miss["miss-found"]["ok"], engine
        assert not miss["miss-budget"]["ok"] and miss["miss-budget"]["nodes_explored"] >= 37, engine
        assert not miss["miss-exhausted"]["ok"] and miss["miss-exhausted"]["nodes_explored"] < miss["miss-exhausted"]["budget"]
        cf, tf = by("planted-cached-first")[0], by("planted-trivial-first")[0]
        assert cf["cache_hit"] and cf["path"][-2:] == [[0, 99], [1, 98]] and tf["ok"] and not tf["cache_hit"], engine
        cf, rf = by("planted-raise-cached-first")[0], by("planted-raise-raising-first")[0]
        assert rf["raises"] and (cf["raises"] if engine == "mcts" else cf["cache_hit"]), engine
        # the same searches end differently without a cache
        differ = [r for r in hits if r["without"] is None or r["without"][:2] != [r["ok"], r["path"]]]
        assert len(differ) >= 10 and any(r["without"] is not None and not r["without"][0] for r in hits), engine
        assert {r["cyclical"] for r in recs} == {False, True}, engine


if __name__ == "__main__":
    main()
