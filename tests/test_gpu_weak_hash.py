"""Every search engine's visited set under a colliding hash.  The engines run through
libacx_weakhash.so (build.py: the search units compiled with the hash seam of csrc/acx_test_hash.h
at 8 classes): every key hashes to one of 8 values whose low 61 bits are ones, so every probe starts
in the table's last bucket and wraps, a search's nodes form one chain, a state meets entries of
other states with its own fingerprint at every insert (false fingerprint matches; the full key
compare decides), a chunk's lanes claim along that one chain, and stale entries of earlier epochs
lie anywhere in it (tests/test_weak_hash_cpu.py pins those properties of the hash).  The searches
must not change: the expected values are the reference's recorded runs (tests/golden), the
yardsticks (tests/bfs_yardstick.py, tests/greedy_yardstick.py, tests/beam_yardstick.py,
tests/vgreedy_yardstick.py, tests/mcts_yardstick.py) and the same calls made in this process through libacx.so -- never the
variant's.

The variant cannot share a process with libacx.so: each test hands its calls to one fresh child
(tests/weak_hash_child.py), one at a time.  After a child that ended on a signal, an abort or its
timeout, the module's remaining tests are skipped.  Every job reports node counts and the number
of distinct key hashes over its final node keys: at most 8 classes of at least 64 nodes on average.

Budgets: at most 5,000 nodes for one search and 2,000 per search of a batch (an insert reads
nodes / 8 buckets), except AK(2) to its path (15,553 nodes) in the multi-rank job."""
import json
import os

import numpy as np
import pytest
import torch

import bfs_yardstick as YB
import greedy_yardstick as YG
import mcts_yardstick as YM
import test_gpu_beam_many as TBM
import test_gpu_bfs_many as TB
import test_gpu_greedy_many as TG
import test_gpu_vgreedy_many as TVM
import vgreedy_yardstick as YV
from conftest import GOLDEN
from many_common import AK2, _check_records, _dataset_rows, _load
from test_gpu_sbfs import _ak3, _check_cases, _extra_cases, _ms17
from weak_hash_common import ChildDied, check_classes, run_child, skip_after_death

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
BATCH_CAP = 2000  # nodes per search of a batch
DEAD = []  # why a child died: the tests after it are skipped


@pytest.fixture(autouse=True)
def _one_death_ends_the_module():
    skip_after_death(DEAD)


def _job(name, calls, tmp_path, timeout=240):
    """(a missing variant library fails the test here, with the build command in the message)"""
    try:
        out, arrays, dt = run_child(calls, tmp_path, timeout)
    except ChildDied as e:
        DEAD.append(f"{name}: {e}")
        pytest.fail(DEAD[-1])
    print(f"weak-hash job {name}: {len(calls)} calls in {dt:.1f} s")
    return out, arrays


def _report(name, what, nodes, classes):
    print(f"weak-hash job {name}: {what}: {nodes} nodes in {classes} hash classes")
    check_classes(nodes, classes, (name, what))


def _boundary_cases(mod, L):
    """mod.boundary_cases(L) with its large budget at BATCH_CAP (uncached: the module's own tests
    keep theirs), the searches above the cap left out"""
    big = mod.BIG
    mod.BIG = BATCH_CAP
    try:
        cases, flags = mod.boundary_cases.__wrapped__(L)
    finally:
        mod.BIG = big
    return [c for c in cases if c[1] <= BATCH_CAP], flags


def _tile(rows, n=64):
    """the rows repeated until there are at least n: that many searches in one launch"""
    return [rows[i % len(rows)] for i in range(max(n, len(rows)))]


def _st(answer):
    return {k: np.array(v) for k, v in answer["st"].items()}


def _wrap_calls(first):
    """a call twice on one handle, 64 small calls on it that take its table's 6-bit epoch past its
    wrap, and the call again: answers 0, 1, 2 .. 65, 66"""
    small = dict(first, pres=first["pres"][:2], budgets=first["budgets"][:2])
    return [first, first] + [small] * 64 + [first]


def _check_wrap(out):
    assert out[1] == out[0] and out[66] == out[0]
    for a in out[2:66]:
        assert a["res"] == out[0]["res"][:2] and all(v == out[0]["st"][k][:2] for k, v in a["st"].items())


# ---------------------------------------------------------------------------------------------
# the device BFS (csrc/acx_bfs.hip)
# ---------------------------------------------------------------------------------------------
def test_device_bfs(tmp_path):
    from acx.envs.utils import convert_relators_to_presentation
    from acx.search import _device_bfs as D
    from acx.search import _engine as E
    cases = _extra_cases()
    assert len(cases) >= 100
    chunks = (0, 3, 64)
    calls = [{"op": "device_bfs", "pres": c["presentation"], "budget": c["budget"], "cyc": c["cyclical"], "chunk": ch}
             for ch in chunks for c in cases]
    n_cases = len(calls)
    orders = [(L, ch) for L in (15, 36, 128) for ch in (0, 777)]
    calls += [{"op": "device_bfs", "pres": _ak3(L).tolist(), "budget": 4000, "cyc": False, "chunk": ch, "keys": True}
              for L, ch in orders]
    n_orders = len(calls)
    # (at L = 15, one workspace for both: at AK(2)'s own L = 7, AK(3) has 42 states in reach)
    row = [(convert_relators_to_presentation([1, 1, -2, -2, -2], [1, 2, 1, -2, -1, -2], 15).tolist(), 300),
           (_ak3(15).tolist(), 1000)]
    calls.append({"op": "release"})
    calls += [{"op": "device_bfs", "pres": row[i % 2][0], "budget": row[i % 2][1], "cyc": False, "chunk": 0, "keys": True}
              for i in range(70)]
    # recorded runs with two key words (L = 18; the random ones above have one)
    recs = [c for c in _load("search_many.json")["solvable"] if c["budget"] == 1000]
    recs = [c for c in recs if c["nodes"] is not None][:10] + [c for c in recs if c["ok"]][:14]
    n_recs = len(calls)
    calls += [{"op": "device_bfs", "pres": c["presentation"], "budget": c["budget"], "cyc": c["cyclical"], "chunk": 0}
              for c in recs]
    out, arrays = _job("device_bfs", calls, tmp_path)

    for k, ch in enumerate(chunks):  # the reference's recorded runs
        got = [("raises" if a.get("raises") else (a["ok"], a["path"], a["nodes"] if a["status"] == 2 else None))
               for a in out[k * len(cases):(k + 1) * len(cases)]]
        _check_cases(cases, got)
    host = {}
    for i, (L, ch) in enumerate(orders, n_cases):  # node for node the device queue and the host engine's
        a, keys = out[i], arrays[f"a{i}_keys"]
        ref = D.device_bfs(_ak3(L), 4000, device=DEV, chunk=ch, keep_node_keys=True)
        st = dict(D.LAST_STATS)
        assert (a["ok"], a["path"]) == (ref[0], ref[1]) == (False, None)
        assert (a["status"], a["nodes"], a["parents"], a["min_length"]) == \
            (st["status"], st["nodes"], st["parents"], st["min_length"]), (L, ch)
        assert keys.tobytes() == np.asarray(st["node_keys"])[:st["nodes"]].tobytes(), (L, ch)
        if L not in host:
            E.run_search(E.BFS, _ak3(L), 4000, False, False, device=DEV, keep_node_keys=True)
            host[L] = (E.LAST_STATS["nodes"], E.LAST_STATS["node_keys"])
        assert a["nodes"] == host[L][0] and keys.tobytes() == host[L][1].tobytes(), (L, ch)
        _report("device_bfs", f"AK(3) L={L} chunk={ch}", a["nodes"], a["classes"])
    D.release_workspaces()
    first = {}
    for i in range(70):  # one workspace, across the wrap of its epoch
        j = n_orders + 1 + i
        got = (json.dumps(out[j], sort_keys=True), arrays[f"a{j}_keys"].tobytes())
        if i % 2 not in first:
            first[i % 2] = got
            ref = D.device_bfs(np.array(row[i % 2][0]), row[i % 2][1], device=DEV, keep_node_keys=True)
            st = dict(D.LAST_STATS)
            a = out[j]
            assert (a["ok"], a["path"]) == (ref[0], None if ref[1] is None else [list(x) for x in ref[1]])
            assert (a["status"], a["nodes"], a["parents"], a["min_length"]) == \
                (st["status"], st["nodes"], st["parents"], st["min_length"]), i
            assert got[1] == np.asarray(st["node_keys"])[:st["nodes"]].tobytes(), i
        assert got == first[i % 2], i
    _report("device_bfs", "AK(3) L=15 on a reused workspace", out[n_orders + 2]["nodes"], out[n_orders + 2]["classes"])
    D.release_workspaces()
    assert len(recs) == 24 and {c["cyclical"] for c in recs} == {False, True} and recs[0]["nodes"] >= 1000
    for c, a in zip(recs, out[n_recs:]):
        assert [a["ok"], a["path"]] == [c["ok"], c["path"]], c
        assert (a["nodes"] if a["status"] == 2 else None) == c["nodes"], c


# ---------------------------------------------------------------------------------------------
# the batched engines (csrc/acx_mbfs.hip, csrc/acx_mgreedy.hip, csrc/acx_beam.hip, csrc/acx_vgreedy.hip,
# csrc/acx_mcts.hip)
# ---------------------------------------------------------------------------------------------
def _check_many(answer, part, tag):
    """a call's answer against the yardstick's results y of its searches [(presentation, y)]"""
    res, st = answer["res"], _st(answer)
    assert len(res) == len(part)
    for i, (_, y) in enumerate(part):
        want = None if y["raises"] else [y["ok"], None if y["path"] is None else [list(x) for x in y["path"]]]
        assert res[i] == want, (tag, i)
        assert (st["status"][i], st["nodes"][i], st["min_length"][i]) == (y["status"], y["nodes"], y["min_length"]), (tag, i)
        assert st["parents"][i] == y["parents"], (tag, i)


def test_bfs_many(tmp_path):
    recs = {cyc: [c for c in _load("search_many.json")["solvable"] if c["cyclical"] == cyc and c["budget"] <= BATCH_CAP]
            for cyc in (False, True)}
    assert all(len(r) >= 50 for r in recs.values())
    rec_call = {cyc: {"op": "bfs_many", "pres": [c["presentation"] for c in r], "budgets": [c["budget"] for c in r],
                      "cyc": cyc} for cyc, r in recs.items()}
    calls = _wrap_calls(rec_call[False]) + [rec_call[True]]  # 0 .. 66: one handle; 67
    bound = {}
    for L in (18, 36, 65):  # 65: the round's keys in the HBM scratch, not in LDS
        cases, flags = _boundary_cases(TB, L)  # (after the loop: those of L = 65)
        assert flags == set(TB.FLAGS), (L, flags)
        part = _tile([(c[0], c[1], c[2]) for c in cases])
        bound[L] = (len(calls), part)
        calls.append({"op": "bfs_many", "pres": [p[0].tolist() for p in part], "budgets": [int(p[1]) for p in part],
                      "cyc": False})
    # the batched engines return no node keys: the largest search again through the one-search engine
    s, budget, y = max(cases, key=lambda c: c[2]["nodes"])
    calls.append({"op": "device_bfs", "pres": s.tolist(), "budget": int(budget), "cyc": False, "chunk": 0, "keys": True})
    out, _ = _job("bfs_many", calls, tmp_path)

    for i, cyc in ((0, False), (67, True)):
        _check_records(recs[cyc], out[i]["res"], _st(out[i]))
    _check_wrap(out)
    for L, (i, part) in bound.items():
        assert len(part) >= 64
        _check_many(out[i], [(p[0], p[2]) for p in part], ("bfs_many", L))
    assert out[-1]["nodes"] >= y["nodes"] >= BATCH_CAP and out[-1]["status"] == y["status"] == YB.BUDGET
    _report("bfs_many", f"the largest search (L=65, budget {budget})", y["nodes"], out[-1]["classes"])


def test_greedy_many(tmp_path):
    gm = _load("greedy_many.json")
    recs = {cyc: [c for c in gm["solvable"] if c["cyclical"] == cyc and c["budget"] <= BATCH_CAP] for cyc in (False, True)}
    assert all(len(r) >= 50 for r in recs.values()) and {c["budget"] for c in gm["dataset"]} == {BATCH_CAP}

    def call(rows, budgets, cyc):
        return {"op": "greedy_many", "pres": rows, "budgets": budgets, "cyc": cyc}

    rec_call = {cyc: call([c["presentation"] for c in r], [c["budget"] for c in r], cyc) for cyc, r in recs.items()}
    calls = _wrap_calls(rec_call[False]) + [rec_call[True]]  # 0 .. 66: one handle; 67
    calls.append(call([c["presentation"] for c in gm["dataset"]], BATCH_CAP, False))  # 68
    bound = {}
    for L in (17, 36):
        cases, flags = _boundary_cases(TG, L)
        # among them a pop that yields one new child twice, and two frontier nodes whose heap keys tie
        assert {"same_child_in_pop", "k0_tie"} <= flags, (L, flags)
        for cyc in (False, True):
            part = _tile([(c[0], c[1], c[3]) for c in cases if c[2] == cyc])
            bound[(L, cyc)] = (len(calls), part)
            calls.append(call([p[0].tolist() for p in part], [int(p[1]) for p in part], cyc))
    rng = np.random.default_rng(65)
    rows = [TG._scrambled(65, rng, 4 + n) for n in range(8)]
    for cyc in (False, True):
        part = _tile([(s, b, YG.greedy(s, b, cyc)) for s in rows for b in (1500, 97)])
        bound[(65, cyc)] = (len(calls), part)
        calls.append(call([p[0].tolist() for p in part], [int(p[1]) for p in part], cyc))
    big = max(gm["dataset"], key=lambda c: c["nodes"] or 0)
    calls.append({"op": "greedy_device", "pres": big["presentation"], "budget": BATCH_CAP, "cyc": False, "keys": True})
    out, _ = _job("greedy_many", calls, tmp_path)

    for i, cyc in ((0, False), (67, True)):
        _check_records(recs[cyc], out[i]["res"], _st(out[i]))
    _check_wrap(out)
    _check_records(gm["dataset"], out[68]["res"], _st(out[68]))
    for (L, cyc), (i, part) in bound.items():
        assert len(part) >= 64
        _check_many(out[i], [(p[0], p[2]) for p in part], ("greedy_many", L, cyc))
    assert out[-1]["nodes"] == big["nodes"] >= BATCH_CAP
    _report("greedy_many", f"the largest dataset search (budget {BATCH_CAP})", big["nodes"], out[-1]["classes"])


def test_beam_many(tmp_path):
    """AK(3), S0, W = 50: the results are those of the shipped library"""
    call = dict(op="beam_many", pres=[TBM._pad(TBM.AK3, 18).tolist()], scorer="S0", W=50, budget=3000, cyc=False)
    out, _ = _job("beam_many", [call], tmp_path, timeout=300)
    got = out[0]
    _report("beam_many", "AK(3) L=18 W=50", got["nodes"][0], got["classes"][0])
    res, st = TBM._many(np.array(call["pres"], np.int32), "S0", 50, 3000)
    assert got["res"] == res and got["st"] == {k: v.tolist() for k, v in st.items()}
    assert st["nodes"][0] == got["nodes"][0] >= 512


def test_vgreedy_many(tmp_path):
    """AK(3), a pop with twins and Miller-Schupp rows at L = 18, at most 2,000 nodes per search,
    through the variant library in one child with one time limit: the results are those of the
    shipped library in this process, and every search's nodes fall in at most 8 hash classes"""
    twin = next(p for p, _, _, _ in YV.twin_cases() if len(p) == 36)
    rows = [TVM._pad(TVM.AK3, 18), twin] + list(_dataset_rows()[::40])
    budgets = [1989, 600] + [1200] * (len(rows) - 2)
    call = dict(op="vgreedy_many", pres=[r.tolist() for r in rows], scorer="S1", budgets=budgets, cyc=False)
    out, _ = _job("vgreedy_many", [call], tmp_path, timeout=300)
    got = out[0]
    res, st = TVM._many(np.stack(rows), "S1", budgets, on_error="return")
    assert got["res"] == res and got["st"] == {k: v.tolist() for k, v in st.items()}
    assert max(got["nodes"]) <= BATCH_CAP and got["nodes"] == [int(v) for v in st["nodes"]]
    big = [(n, c) for n, c in zip(got["nodes"], got["classes"]) if n >= 512]
    assert len(big) >= 3
    for n, c in big:
        _report("vgreedy_many", "a search at L=18", n, c)


def test_mcts_many(tmp_path):
    """AK(3), an expansion with twins and Miller-Schupp rows at L = 18, at most 2,000 nodes per
    search, on features at c = 1.41 and on token ids at c = 0: the results are the yardstick's, and
    every large search's nodes fall in at most 8 hash classes"""
    twin = next(p for p, _, _, _ in YV.twin_cases() if len(p) == 36)
    rows = [TVM._pad(TVM.AK3, 18), twin] + list(_dataset_rows()[::40])
    budgets = [1989, 600] + [1200] * (len(rows) - 2)
    calls = [dict(op="mcts_many", pres=[r.tolist() for r in rows], scorer=s, budgets=budgets, c=c, cyc=cyc)
             for s, c, cyc in (("M1", 1.41, False), ("TOK", 0.0, False))]
    out, _ = _job("mcts_many", calls, tmp_path, timeout=240)
    large = 0
    for call, got in zip(calls, out):
        tokens = call["scorer"] in YM.TOKEN_MODELS
        ys = [YM.mcts(p, YM.model_np(call["scorer"]), b, call["c"], call["cyc"], on_tokens=tokens)
              for p, b in zip(rows, budgets)]
        assert got["res"] == [None if y["raises"] else [y["ok"], y["path"]] for y in ys], call["scorer"]
        for k in ("status", "nodes", "iterations"):
            assert got["st"][k] == [y[k] for y in ys], (call["scorer"], k)
        assert got["nodes"] == [len(y["states"]) for y in ys] and max(got["nodes"]) <= BATCH_CAP
        assert any(y["twin_expansions"] for y in ys) and sum(y["ucb_sel"] for y in ys) >= 1000
        for n, c in zip(got["nodes"], got["classes"]):
            if n >= 512:
                check_classes(n, c, ("mcts_many", call["scorer"]))
                large += 1
    assert large >= 12


def test_edge_lengths(tmp_path):
    """The near-full starts of tests/search_edge_common.py at L = 49 (the first L of NW = 4) and
    L = 64 (its full tile: 5 key words), both flags, at their three budgets, through the device
    BFS (chunk 3), the device greedy and the two batched engines: the yardsticks' values.  Twins
    that differ in the top key word of a relator's tile share a chain with every other node here,
    so the compare over all the key's words alone keeps them apart."""
    import search_edge_common as SE
    from conftest import unpack_keys_np
    calls, want = [], []
    for L in (49, 64):
        for cyc in (False, True):
            cs = [SE.cases(L, cyc)[name] for name in ("N1", "N0")]
            for c in cs:
                for budget, y in c["bfs"]:
                    calls.append({"op": "device_bfs", "pres": c["start"].tolist(), "budget": int(budget), "cyc": cyc,
                                  "chunk": 3, "keys": True})
                    want.append(("device_bfs", L, y))
                for budget, y in c["greedy"]:
                    calls.append({"op": "greedy_device", "pres": c["start"].tolist(), "budget": int(budget), "cyc": cyc,
                                  "keys": True})
                    want.append(("greedy_device", L, y))
            for op, engine in (("bfs_many", "bfs"), ("greedy_many", "greedy")):
                part = [(c["start"], b, y) for c in cs for b, y in c[engine]]
                calls.append({"op": op, "pres": [p[0].tolist() for p in part], "budgets": [int(p[1]) for p in part],
                              "cyc": cyc})
                want.append((op, L, part))
    out, arrays = _job("edge_lengths", calls, tmp_path)
    for i, ((op, L, y), a) in enumerate(zip(want, out)):
        tag = (i, op, L)
        if op in ("bfs_many", "greedy_many"):
            _check_many(a, [(p[0], p[2]) for p in y], tag)
            continue
        assert not y["raises"] and not a.get("raises"), tag
        path = None if y["path"] is None else [list(x) for x in y["path"]]
        assert (a["ok"], a["min_length"]) == (y["ok"], y["min_length"]) and 1 <= a["classes"] <= 8, tag
        if y["status"] == YB.BUDGET:
            assert a["nodes"] == y["nodes"], tag
        if op == "device_bfs":
            assert (a["status"], a["parents"], a["path"]) == (y["status"], y["parents"], path), tag
            keys = arrays[f"a{i}_keys"]
            assert len(keys) >= y["nodes"] and np.array_equal(unpack_keys_np(keys[:y["nodes"]], L), y["states"]), tag
        else:  # acx_greedy_status: 1 success, 2 failed
            assert (a["status"], a["path"]) == (1 if y["ok"] else 2, path), tag


# ---------------------------------------------------------------------------------------------
# the device greedy (csrc/acx_greedy.hip: host_hash, Recent, read-only probe / CAS-only commit)
# ---------------------------------------------------------------------------------------------
def test_device_greedy(tmp_path):
    with open(os.path.join(GOLDEN, "kat_search_extra.json")) as f:
        cases = [c for c in json.load(f) if c["search_fn"] == "greedy_search"]
    assert len(cases) == 120
    calls = [{"op": "greedy_device", "pres": c["presentation"], "budget": c["budget"], "cyc": c["cyclical"],
              "keys": c["budget"] >= 1000} for c in cases]
    # recorded runs with two key words (L = 18; the random ones have one): 8 cut by the budget, 8 solved
    recs = _load("greedy_many.json")["dataset"]
    recs = [c for c in recs if not c["ok"]][:8] + [c for c in recs if c["ok"]][:8]
    calls += [{"op": "greedy_device", "pres": c["presentation"], "budget": c["budget"], "cyc": c["cyclical"]}
              for c in recs]
    out, _ = _job("device_greedy", calls, tmp_path)
    assert len(recs) == 16 and all(c["nodes"] >= 2000 for c in recs[:8])
    for c, a in zip(recs, out[len(cases):]):
        assert [a["ok"], a["path"]] == [c["ok"], c["path"]], c
        assert (a["nodes"] if a["status"] == 2 else None) == c["nodes"], c
    large = []
    for c, a in zip(cases, out):
        if c["raises"]:
            assert a.get("raises"), c
            continue
        assert a["status"] in (1, 2) and (a["status"] == 1) == a["ok"] == c["ok"], c
        assert a["path"] == c["path"], c
        if c["budget_nodes"] is not None:
            assert a["nodes"] == c["budget_nodes"], c
        if "classes" in a and a["nodes"] >= 512:
            large.append((a["nodes"], a["classes"]))
    assert large and max(n for n, _ in large) >= 5000
    for nodes, classes in large:
        _report("device_greedy", "a reference run", nodes, classes)


# ---------------------------------------------------------------------------------------------
# the owner-partitioned BFS (csrc/acx_sbfs.hip)
# ---------------------------------------------------------------------------------------------
def _device_queue(pres, budget, cyc, chunk):
    from acx.search import _device_bfs as D
    ref = D.device_bfs(np.array(pres), budget, cyclically_reduce_after_moves=cyc, device=DEV, chunk=chunk,
                       keep_node_keys=True)
    return (ref[0], None if ref[1] is None else [list(x) for x in ref[1]]), dict(D.LAST_STATS)


def test_sharded_bfs_one_rank(tmp_path):
    cases = _extra_cases()
    calls = [{"op": "sbfs", "pres": c["presentation"], "budget": c["budget"], "cyc": c["cyclical"], "chunk": 3}
             for c in cases]
    order = {"op": "sbfs", "pres": _ak3(36).tolist(), "budget": 4000, "cyc": False, "chunk": 500, "keys": True}
    calls += [order, dict(order, arena_log2_cap=6)]
    out, arrays = _job("sbfs_one_rank", calls, tmp_path)
    _check_cases(cases, [("raises" if a.get("raises") else (a["ok"], a["path"], a["nodes"] if a["status"] == 2 else None))
                         for a in out[:len(cases)]])
    ref, st = _device_queue(order["pres"], 4000, False, 500)
    nd, dk = st["nodes"], np.asarray(st["node_keys"])[:st["nodes"]]
    for i in (len(cases), len(cases) + 1):  # the plain run, the one whose key arena regrows from 64 records
        a = out[i]
        assert (a["ok"], a["path"]) == ref and a["nodes"] == nd
        assert (a["chunks"], a["parents"], a["min_length"]) == (st["chunks"], st["parents"], st["min_length"])
        assert np.array_equal(arrays[f"a{i}_ids"][:nd], np.arange(nd)) and np.array_equal(arrays[f"a{i}_keys"][:nd], dk)
        _report("sbfs_one_rank", "AK(3) L=36" + (" with arena regrowth" if i > len(cases) else ""), a["nodes"], a["classes"])


@pytest.mark.parametrize("world", [2, 3])
def test_sharded_bfs_ranks(world, tmp_path):
    orders = {"ak3_36": (_ak3(36).tolist(), 4000, False, 500),
              "ak2": (AK2, 10 ** 6, False, 64),  # to its path
              "ms17": (_ms17(), 4000, False, 500)}
    cases = _extra_cases(40)
    call = {"op": "sbfs_ranks", "world": world, "timeout": 200,
            "jobs": {"orders": orders, "cases": cases, "case_chunk": 3}}
    out, arrays = _job(f"sbfs_{world}_ranks", [call], tmp_path, timeout=300)
    a = out[0]
    assert a["error"] == [None] * world and a["exit"] == [0] * world, a
    for r in range(world):
        _check_cases(cases, [x if x == "raises" else tuple(x) for x in a["cases"][r]])
    for name, (pres, budget, cyc, chunk) in orders.items():
        ref, st = _device_queue(pres, budget, cyc, chunk)
        nd, dk = st["nodes"], np.asarray(st["node_keys"])
        for r, got in enumerate(a["orders"][name]):  # every rank returns the reference result
            assert (got["ok"], got["path"]) == ref and got["nodes"] == nd, (name, r)
            assert got["trace"] == st["min_trace"], (name, r)
            # every store is non-empty: the owners spread although sbfs's fingerprint is one value,
            # so a received record displaces an own child and the reverse
            _report(f"sbfs_{world}_ranks", f"{name}: the store of rank {r}", got["store_nodes"], got["store_classes"])
        ids = np.concatenate([arrays[f"a0_{name}_{r}_ids"] for r in range(world)])
        keys = np.concatenate([arrays[f"a0_{name}_{r}_keys"] for r in range(world)])
        order = np.argsort(ids, kind="stable")
        ids, keys = ids[order], keys[order]
        n = len(dk)  # the union of the stores, ordered by id, is the device queue
        assert n >= min(nd, 1) and len(ids) >= n and np.unique(ids).size == len(ids), name
        assert np.array_equal(ids[:n], np.arange(n)) and np.array_equal(keys[:n], dk), name
    from acx.search import _device_bfs as D
    D.release_workspaces()
