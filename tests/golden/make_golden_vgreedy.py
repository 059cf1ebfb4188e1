"""tests/golden/vgreedy_search.json: reference value_guided_greedy_search runs
(value_search/value_guided_search.py:253-414) for the batched value-guided greedy search
(acx.value_guided_greedy_search_many, acx.value_guided_greedy_search).

    python tests/golden/make_golden_vgreedy.py --reference ROOT [--procs N]

The reference is loaded as make_golden_beam.py loads it.  Every run is the reference's own
value_guided_greedy_search on the CPU with, as its model, an nn.Module that computes one of the exact
scorers of tests/beam_yardstick.py: 'mlp' with mean 0 and std 1 (SCORERS), 'mlp' with NORM_MEAN /
NORM_STD (NORM_SCORERS on the normalised features), 'seq' on the token ids (TOK), or no model at all
(use_length_priority=True).  The reference applies expm1 to the model's output before it pushes: the
module records every distinct value it returns, and the generator asserts that expm1 is finite and
strictly increasing over them, so the heap's order by score is the scorer's.

A record: {name, presentation, L, scorer, arch, norm, length_priority, budget, cyclical, raises, ok,
path, nodes_explored, min_length}.  The cases:
  ak      AK(2) at L = 7 and AK(3) at L = 18, both flags, S0 S1 S2 S4 (S3 at L = 7), budgets 1, 37, 3000;
  len     use_length_priority=True: AK(2), AK(3), Miller-Schupp rows;
  roots   a root with a trivial child, a root whose heap runs empty, budgets 0 and 1;
  raise   presentations on which a move raises (the raising bfs cases of kat_search_extra.json);
  ms      30 Miller-Schupp rows padded to L = 36, S0 / S1;
  norm    NORM_SCORERS with NORM_MEAN / NORM_STD and TOK on AK(3) and Miller-Schupp rows;
  long    L = 128 rows.
The generator refuses to write a fixture without: found, budget and exhausted endings; a budget
overshoot of at least 2; a budget-1 run; a record whose min_length is the total of a duplicate
child; a record that ends differently without its normalisation (both by the yardstick,
tests/vgreedy_yardstick.py, which must reproduce every record first).

On "min_length from a duplicate child": min_length can never DROP at a duplicate -- a state in the
visited set is the root or was a child before, so its total is already counted -- which is why an
engine may take the minimum before or after the visited test.  What a record can show is that the
final minimum is a total that a child failing the visited test also had (the yardstick's min_dup),
so a minimum taken over the duplicates alone, or over the survivors alone, is told apart from one
that skips a whole pop."""
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
        _SEARCH = importlib.import_module("value_search.value_guided_search").value_guided_greedy_search
    return _SEARCH


def run_case(args):
    root, case = args
    import torch
    torch.set_num_threads(1)
    from beam_yardstick import NORM_MEAN, NORM_STD, SCORERS, TOKEN_SCORERS
    search = load_search(root)
    arch = case["arch"]
    fn = (SCORERS if arch == "mlp" else TOKEN_SCORERS)[case["scorer"]][1]
    mean, std = (NORM_MEAN, NORM_STD) if case["norm"] else (np.zeros(14, np.float32), np.ones(14, np.float32))
    if arch != "mlp":
        mean = std = None
    seen = set()

    class Model(torch.nn.Module):
        def forward(self, f):
            y = fn(f).to(torch.float32)
            seen.update(y.tolist())
            return y[:, None]

    pres = np.array(case["presentation"], np.int8)
    rec = dict(case)
    try:
        ok, path, st = search(pres, None if case["length_priority"] else Model(), arch, mean, std,
                              max_nodes_to_explore=case["budget"], device="cpu",
                              use_length_priority=case["length_priority"],
                              cyclically_reduce_after_moves=case["cyclical"])
        rec.update(raises=False, ok=bool(ok), path=to_jsonable(path), nodes_explored=int(st["nodes_explored"]),
                   min_length=int(st["min_length"]))
    except AssertionError:
        rec.update(raises=True, ok=False, path=None, nodes_explored=None, min_length=None)
    # the reference pushed expm1(score): the same order as the scores', or the case is no fixture
    v = torch.tensor(sorted(seen), dtype=torch.float32)  # (-0.0 == 0.0: one of them)
    e = torch.expm1(v)
    assert bool(torch.isfinite(e).all()) and bool((e[1:] > e[:-1]).all()), (case["name"], v.tolist())
    return rec


def case(name, p, scorer, budget, cyc, arch="mlp", norm=False, length_priority=False):
    p = [int(x) for x in p]
    return dict(name=name, presentation=p, L=len(p) // 2, scorer=scorer, arch=arch, norm=bool(norm),
                length_priority=bool(length_priority), budget=int(budget), cyclical=bool(cyc))


def all_cases():
    from beam_yardstick import NORM_SCORERS
    cases = []
    for name, p in (("AK2", AK2), ("AK3", AK3)):
        for s in ("S0", "S1", "S2", "S4") + (("S3",) if name == "AK2" else ()):
            for budget in (1, 37, 3000):
                for cyc in (False, True):
                    cases.append(case(f"ak-{name}", p, s, budget, cyc))
    ms = np.load(os.path.join(PKG_DATA, "all_presentations.npy"))
    for i, (p, budget) in enumerate([(AK2, 3000), (AK2, 100), (AK3, 2000), (AK3, 1)] + [
            (repad(r, MS_L), 900 + 50 * j) for j, r in enumerate(ms[5::149][:8])]):
        cases.append(case("len", p, "S0", budget, bool(i % 2), length_priority=True))
    cases.append(case("roots-trivial", [1, 0, 0, 2, 0, 0], "S0", 100, False))
    cases.append(case("roots-trivial", [-2, 0, 0, 0, 1, 0, 0, 0], "S1", 100, True))
    cases.append(case("roots-dies", [1, 1, 2, 2], "S0", 100, False))
    cases.append(case("roots-budget1", AK2, "S0", 1, False))
    cases.append(case("roots-budget0", AK2, "S1", 0, False))
    with open(os.path.join(HERE, "kat_search_extra.json")) as f:
        raising = [c for c in json.load(f) if c["search_fn"] == "bfs" and c["raises"]]
    for i, c in enumerate(raising[:8]):
        cases.append(case("raise", c["presentation"], ("S0", "S1")[i % 2], 500, c["cyclical"]))
    for i, r in enumerate(ms[:: len(ms) // 30][:30]):
        cases.append(case("ms", repad(r, MS_L), ("S0", "S1")[i % 2], 1500 - 31 * i, bool(i % 4 == 3)))
    scorers = [("mlp", s) for s in NORM_SCORERS] + [("seq", "TOK")]
    i = 0
    for name, p in (("AK2", AK2), ("AK3", AK3)):
        for arch, s in scorers:
            for budget in (3000, 400):
                cases.append(case(f"norm-{name}", p, s, budget - 7 * i, bool(i % 2), arch, arch == "mlp"))
                i += 1
    for j, r in enumerate(ms[17:: len(ms) // 10][:10]):
        arch, s = scorers[j % len(scorers)]
        cases.append(case("norm-ms", repad(r, MS_L), s, 2500 - 100 * j, bool(j % 4 >= 2), arch, arch == "mlp"))
    cases.append(case("long", repad(AK3, 128), "S1q", 1500, False))
    cases.append(case("long", repad(ms[-1], 128), "S1q", 1500, True))
    return cases


def _end(r):
    return "raises" if r["raises"] else "found" if r["ok"] else "budget" if r["nodes_explored"] >= max(
        r["budget"], 1) else "died"


def yardstick_of(r, norm=None):
    import vgreedy_yardstick as Y
    norm = r["norm"] if norm is None else norm
    kw = dict(mean=Y.NORM_MEAN, std=Y.NORM_STD) if norm else {}
    return Y.vgreedy(np.array(r["presentation"]), r["scorer"], r["budget"], r["cyclical"], **kw)


def check_not_vacuous(recs):
    import vgreedy_yardstick as Y
    ys = [yardstick_of(r) for r in recs]
    for r, y in zip(recs, ys):
        want = (r["raises"], r["ok"], r["path"] or [], r["nodes_explored"], r["min_length"])
        assert Y.result(y) == want, (r, Y.result(y))
    ends = {_end(r) for r in recs}
    assert ends == {"found", "budget", "died", "raises"}, ends
    assert max(r["nodes_explored"] - r["budget"] for r in recs if _end(r) == "budget" and r["budget"] >= 1) >= 2
    assert any(r["budget"] == 1 and not r["raises"] and r["nodes_explored"] > 1 for r in recs)
    assert any(y["min_dup"] and y["min_length"] < int(np.count_nonzero(r["presentation"])) for r, y in zip(recs, ys))
    differ = [r for r, y in zip(recs, ys) if r["norm"] and Y.result(yardstick_of(r, norm=False)) != Y.result(y)]
    assert differ, "no record ends differently without its normalisation"
    assert any(r["length_priority"] for r in recs) and {r["cyclical"] for r in recs} == {False, True}
    return ends, len(differ)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True, help="a checkout of the reference project")
    ap.add_argument("--procs", type=int, default=min(16, os.cpu_count() or 1))
    args = ap.parse_args()
    cases = all_cases()
    with Pool(args.procs) as pool:
        recs = pool.map(run_case, [(args.reference, c) for c in cases], chunksize=1)
    ends, differ = check_not_vacuous(recs)
    with open(os.path.join(HERE, "vgreedy_search.json"), "w") as f:
        json.dump(recs, f, separators=(",", ":"))
    print(len(recs), "records", sorted(ends), differ, "end differently without their normalisation")


if __name__ == "__main__":
    main()
