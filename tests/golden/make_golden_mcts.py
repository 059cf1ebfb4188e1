"""tests/golden/mcts_search.json: reference mcts_search runs (value_search/mcts.py:177-314) for the
batched MCTS (acx.mcts_search_many, acx.mcts_search).

    python tests/golden/make_golden_mcts.py --reference ROOT [--procs N]

The reference is loaded as make_golden_beam.py loads it.  Every run is the reference's own
mcts_search on the CPU with, as its model, an nn.Module that computes one of the exact model
outputs of tests/mcts_yardstick.py: 'mlp' with mean 0 and std 1 (M0, M1, MZ, MN), 'mlp' with
NORM_MEAN / NORM_STD (beam_yardstick's NORM_SCORERS on the normalised features), or 'seq' on the
token ids (TOK).

MCTS sums the values after expm1, so their order alone does not fix a run.  While a case runs,
torch.expm1 is wrapped: every (input bits, output bits) pair the reference computes is recorded, and
the fixture stores one table per scorer, {output bits: expm1 bits}.  The yardstick and the GPU test
scorers look their values up there (a miss is a failure), so they see the reference's values bit
for bit on any machine.  An input that got two different outputs would make the table ambiguous:
the generator asserts that none did.

The file: {"tables": {scorer: {bits: bits}}, "records": [...]}.  A record: {name, presentation, L,
scorer, arch, norm, budget, c, cyclical, raises, ok, path, nodes_explored, iterations, mingap} --
mingap is the yardstick's (the smallest nonzero relative gap between the best and the second UCB
score; null without one), for the test that scores with the GPU's own expm1.  The cases:
  ak      AK(2) at L = 7 and AK(3) at L = 18, both flags, budgets 0, 1, 2, 37, 500, 3000;
  c       c_explore 0.0 and 4.0 beside the default 1.41;
  roots   a trivial root, a root that spins to 50 * budget iterations;
  raise   presentations on which a move raises (the raising bfs cases of kat_search_extra.json);
  ms      20 Miller-Schupp rows padded to L = 36, budgets up to 1000;
  norm    NORM_SCORERS with NORM_MEAN / NORM_STD and TOK on AK(3) and Miller-Schupp rows;
  long    two L = 128 rows.
The generator refuses to write a fixture without: found, budget, exhausted and raising endings; a
found path of at least 20 moves; a descent of depth at least 30; at least 100 dead-end iterations
in one run; a budget overshoot of at least 2; a record that ends differently without its
normalisation (by the yardstick, tests/mcts_yardstick.py, which must reproduce every record first)."""
import argparse
import json
import os
import sys
from multiprocessing import Pool

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
TESTS = os.path.dirname(HERE)
REPO = os.path.dirname(TESTS)
for _p in (HERE, TESTS, REPO, os.path.join(REPO, "ac-solver-caltech_amd")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

from make_golden import PKG_DATA, repad, to_jsonable  # noqa: E402
from make_golden_beam import AK2, AK3, MS_L, load_beam_search  # noqa: E402

_SEARCH = None


def load_search(root):
    global _SEARCH
    if _SEARCH is None:
        load_beam_search(root)  # installs the bare package modules
        import importlib
        _SEARCH = importlib.import_module("value_search.mcts").mcts_search
    return _SEARCH


def run_case(args):
    root, case = args
    import torch
    torch.set_num_threads(1)
    import mcts_yardstick as Y
    search = load_search(root)
    arch = case["arch"]
    fn = Y.model_t(case["scorer"])
    mean, std = (Y.NORM_MEAN, Y.NORM_STD) if case["norm"] else (np.zeros(14, np.float32), np.ones(14, np.float32))
    if arch != "mlp":
        mean = std = None

    class Model(torch.nn.Module):
        def forward(self, f):
            return fn(f).to(torch.float32)[:, None]

    table = {}
    real = torch.expm1

    def recording(x):
        y = real(x)
        for a, b in zip(x.contiguous().view(torch.int32).reshape(-1).tolist(),
                        y.contiguous().view(torch.int32).reshape(-1).tolist()):
            a, b = a & 0xffffffff, b & 0xffffffff
            assert table.setdefault(a, b) == b, (case["name"], a, b, table[a])
        return y

    pres = np.array(case["presentation"], np.int8)
    rec = dict(case)
    torch.expm1 = recording
    try:
        ok, path, st = search(pres, Model(), arch, mean, std, max_nodes_to_explore=case["budget"],
                              c_explore=case["c"], device="cpu", cyclically_reduce_after_moves=case["cyclical"])
        rec.update(raises=False, ok=bool(ok), path=to_jsonable(path), nodes_explored=int(st["nodes_explored"]),
                   iterations=int(st["iterations"]))
    except AssertionError:
        rec.update(raises=True, ok=False, path=None, nodes_explored=None, iterations=None)
    finally:
        torch.expm1 = real
    return rec, table


def case(name, p, scorer, budget, cyc, c=1.41, arch="mlp", norm=False):
    p = [int(x) for x in p]
    return dict(name=name, presentation=p, L=len(p) // 2, scorer=scorer, arch=arch, norm=bool(norm),
                budget=int(budget), c=float(c), cyclical=bool(cyc))


def all_cases():
    from beam_yardstick import NORM_SCORERS
    cases = []
    for name, p in (("AK2", AK2), ("AK3", AK3)):
        for cyc in (False, True):
            for i, budget in enumerate((0, 1, 2, 37, 500, 3000)):
                for s in (("M0", "M1", "MZ", "MN") if budget in (37, 3000) else (("M0", "M1")[(i + cyc) % 2],)):
                    cases.append(case(f"ak-{name}", p, s, budget, cyc))
    for c in (0.0, 4.0):
        for j, (p, s) in enumerate(((AK2, "M0"), (AK3, "M1"), (AK3, "M0"))):
            cases.append(case("c", p, s, 600, bool(j % 2), c=c))
    cases.append(case("roots-trivial", [1, 0, 0, 2, 0, 0], "M0", 100, False))
    cases.append(case("roots-trivial", [-2, 0, 0, 0, 1, 0, 0, 0], "M1", 1, True))
    cases.append(case("roots-spins", [1, 1, 2, 2], "M0", 20, False))
    cases.append(case("roots-spins", [1, 1, 2, 2], "M1", 32, True))
    with open(os.path.join(HERE, "kat_search_extra.json")) as f:
        raising = [c for c in json.load(f) if c["search_fn"] == "bfs" and c["raises"]]
    for i, c in enumerate(raising[:8]):
        cases.append(case("raise", c["presentation"], ("M0", "M1")[i % 2], 500, c["cyclical"]))
    ms = np.load(os.path.join(PKG_DATA, "all_presentations.npy"))
    for i, r in enumerate(ms[:: len(ms) // 19][:19]):
        cases.append(case("ms", repad(r, MS_L), ("M0", "M1", "MZ")[i % 3], 1000 - 41 * i, bool(i % 4 == 3),
                          c=(1.41, 1.41, 0.0, 4.0)[i % 4]))
    cases.append(case("ms", repad(ms[1071], MS_L), "M0", 800, True))
    scorers = [("mlp", s) for s in NORM_SCORERS] + [("seq", "TOK")]
    i = 0
    for name, p in (("AK2", AK2), ("AK3", AK3)):
        for arch, s in scorers:
            for budget in (1000, 200):
                cases.append(case(f"norm-{name}", p, s, budget - 7 * i, bool(i % 2), arch=arch, norm=arch == "mlp"))
                i += 1
    for j, r in enumerate(ms[17:: len(ms) // 10][:10]):
        arch, s = scorers[j % len(scorers)]
        cases.append(case("norm-ms", repad(r, MS_L), s, 900 - 60 * j, bool(j % 4 >= 2), arch=arch, norm=arch == "mlp"))
    cases.append(case("long", repad(AK3, 128), "M1", 700, False))
    cases.append(case("long", repad(ms[-1], 128), "M0", 700, True))
    return cases


def _end(r):
    if r["raises"]:
        return "raises"
    if r["ok"]:
        return "found"
    return "budget" if r["nodes_explored"] >= max(r["budget"], 1) else "exhausted"


def yardstick_of(r, tables, norm=None):
    import mcts_yardstick as Y
    values = Y.value_fn(r["scorer"], tables[r["scorer"]])
    if norm is None:
        norm = r["norm"]
    else:  # not the record's own run: outputs the table does not hold, so numpy's expm1
        values = lambda x: np.expm1(np.asarray(Y.model_np(r["scorer"])(x), np.float32))  # noqa: E731
    kw = dict(mean=Y.NORM_MEAN, std=Y.NORM_STD) if norm else {}
    return Y.mcts(np.array(r["presentation"]), values, r["budget"], r["c"], r["cyclical"],
                  on_tokens=r["arch"] != "mlp", **kw)


def want_of(r):
    return (r["raises"], r["ok"], r["path"] or [], r["nodes_explored"], r["iterations"])


def _check_one(args):
    import mcts_yardstick as Y
    r, tables = args
    y = yardstick_of(r, tables)
    assert Y.result(y) == want_of(r), (r, Y.result(y))
    differs = r["norm"] and Y.result(yardstick_of(r, tables, norm=False)) != Y.result(y)
    return {k: y[k] for k in ("deepest", "dead_iters", "overshoot", "mingap", "ties", "ucb_sel")}, differs


def check_not_vacuous(recs, tables, pool):
    shapes = pool.map(_check_one, [(r, tables) for r in recs], chunksize=1)
    for r, (sh, _) in zip(recs, shapes):
        r["mingap"] = None if sh["mingap"] == float("inf") else sh["mingap"]
    ends = {_end(r) for r in recs}
    assert ends == {"found", "budget", "exhausted", "raises"}, ends
    facts = dict(longest_path=max(len(r["path"]) for r in recs if r["ok"]),
                 deepest=max(sh["deepest"] for sh, _ in shapes),
                 dead_iters=max(sh["dead_iters"] for sh, _ in shapes),
                 overshoot=max(sh["overshoot"] for sh, _ in shapes),
                 differ=sum(d for _, d in shapes), ties=sum(sh["ties"] for sh, _ in shapes),
                 ucb_sel=sum(sh["ucb_sel"] for sh, _ in shapes))
    assert facts["longest_path"] >= 20 and facts["deepest"] >= 30 and facts["dead_iters"] >= 100, facts
    assert facts["overshoot"] >= 2 and facts["differ"] >= 1, facts
    assert {r["cyclical"] for r in recs} == {False, True} and {r["c"] for r in recs} == {0.0, 1.41, 4.0}
    return ends, facts


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True, help="a checkout of the reference project")
    ap.add_argument("--procs", type=int, default=min(16, os.cpu_count() or 1))
    args = ap.parse_args()
    cases = all_cases()
    with Pool(args.procs) as pool:
        got = pool.map(run_case, [(args.reference, c) for c in cases], chunksize=1)
        recs = [r for r, _ in got]
        tables = {}
        for r, t in got:
            mine = tables.setdefault(r["scorer"], {})
            for a, b in t.items():
                assert mine.setdefault(str(a), b) == b, (r["scorer"], a)
        ends, facts = check_not_vacuous(recs, tables, pool)
    path = os.path.join(HERE, "mcts_search.json")
    with open(path, "w") as f:
        json.dump(dict(tables=tables, records=recs), f, separators=(",", ":"))
    print(len(recs), "records", sorted(ends), facts, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
