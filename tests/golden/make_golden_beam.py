"""tests/golden/beam_search.json: reference beam_search runs (value_search/value_guided_search.py:
417-561) for the batched beam search (acx.beam_search_many, acx.beam_search).

    python tests/golden/make_golden_beam.py --reference ROOT [--procs N]
    python tests/golden/make_golden_beam.py --reference ROOT --scored    (beam_search_scored.json,
        real-valued scores: scored_cases() below; beam_search.json is left as it is)

The reference is loaded as make_golden.py loads it: bare package modules for ac_solver,
ac_solver.envs and value_search, so the learner's imports are never run.  Every run is the
reference's own beam_search with architecture='mlp', mean 0 and std 1, and as its model an nn.Module
that computes one of the exact scorers of tests/beam_yardstick.py (SCORERS) from the 14 features.
The reference applies expm1 to the model's output before it sorts: the module records every distinct
value it returns, and the generator asserts that expm1 is finite and strictly increasing over them
(so the order by score is the order the reference sorted by); a case that breaks this is an error
here, to be dropped or rescaled (S1q is S1 scaled by 0.25 for L = 128).

A record: {name, presentation, L, scorer, W, budget, cyclical, raises, ok, path, nodes_explored,
steps}.  The cases (tests/test_beam_cpu.py asserts what they cover):
  ak      AK(2) at L = 7 and AK(3) at L = 18, both flags, W in {1, 3, 50}, S0 S1 S2 S4 (S3 at L = 7);
  roots   a trivial root, and a root whose first step dies;
  raise   presentations on which a move raises (the raising bfs cases of kat_search_extra.json);
  ms      40 Miller-Schupp rows padded to L = 36;
  scr     scrambled trivial rows (many_common._scrambled);
  cut     budgets at which the cut falls on the first, a middle and the last child of a parent, and
          on a child that comes before a trivial child of the same step (chosen with the yardstick's
          shape report; the recorded results are the reference's);
  long    one L = 128 row.
"""
import argparse
import json
import os
import sys
import types
from multiprocessing import Pool

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
TESTS = os.path.dirname(HERE)
REPO = os.path.dirname(TESTS)
for _p in (HERE, TESTS, REPO, os.path.join(REPO, "ac-solver-caltech_amd")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

from make_golden import PKG_DATA, repad, to_jsonable  # noqa: E402

AK2 = [1, 1, -2, -2, -2, 0, 0, 1, 2, 1, -2, -1, -2, 0]
AK3 = repad([1, 1, 1, -2, -2, -2, -2, 0, 0, 1, 2, 1, -2, -1, -2, 0, 0, 0], 18).tolist()
MS_ROWS, MS_L, MS_BUDGET = 40, 36, 1500

_BEAM = None


def load_beam_search(root):
    global _BEAM
    if _BEAM is None:
        for name, sub in [("ac_solver", "ac_solver"), ("ac_solver.envs", "ac_solver/envs"),
                          ("value_search", "value_search")]:
            m = types.ModuleType(name)
            m.__path__ = [os.path.join(root, sub)]
            sys.modules[name] = m
        import importlib
        _BEAM = importlib.import_module("value_search.value_guided_search").beam_search
    return _BEAM


def run_case(args):
    root, case = args
    import torch
    torch.set_num_threads(1)
    from beam_yardstick import NORM_MEAN, NORM_STD, SCORERS, TOKEN_SCORERS
    beam_search = load_beam_search(root)
    arch = case.get("arch", "mlp")
    fn = (SCORERS if arch == "mlp" else TOKEN_SCORERS)[case["scorer"]][1]
    mean, std = (NORM_MEAN, NORM_STD) if case.get("norm") else (np.zeros(14, np.float32), np.ones(14, np.float32))
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
        ok, path, st = beam_search(pres, Model(), arch, mean, std,
                                   beam_width=case["W"], max_nodes_to_explore=case["budget"], device="cpu",
                                   cyclically_reduce_after_moves=case["cyclical"])
        rec.update(raises=False, ok=bool(ok), path=to_jsonable(path), nodes_explored=int(st["nodes_explored"]),
                   steps=int(st["steps"]))
    except AssertionError:
        rec.update(raises=True, ok=False, path=None, nodes_explored=None, steps=None)
    # the reference sorted expm1(score): the same order as the scores', or the case is no fixture
    v = torch.tensor(sorted(seen), dtype=torch.float32)  # (-0.0 == 0.0: one of them)
    e = torch.expm1(v)
    assert bool(torch.isfinite(e).all()) and bool((e[1:] > e[:-1]).all()), (case["name"], v.tolist())
    return rec


def case(name, p, scorer, W, budget, cyc):
    p = [int(x) for x in p]
    return dict(name=name, presentation=p, L=len(p) // 2, scorer=scorer, W=int(W), budget=int(budget),
                cyclical=bool(cyc))


def cut_cases():
    """budgets, found with the yardstick, at which the cut child is the first / a middle / the last
    child of its parent, and at which it comes before a trivial child of the same step"""
    from beam_yardstick import FOUND, beam
    out, want = [], {"first": lambda a: a == 0, "middle": lambda a: 0 < a < 11, "last": lambda a: a == 11}
    for b in range(15, 400):
        y = beam(AK3, "S0", 3, b)
        if not y["cut_at"]:
            continue
        a = y["cut_at"][0][1]
        for k in [k for k, f in want.items() if f(a)]:
            out.append(case(f"cut-{k}", AK3, "S0", 3, b, False))
            del want[k]
    assert not want, want
    full = beam(AK2, "S1", 50, 3000)
    assert full["status"] == FOUND
    # total_nodes at the success: with that budget the last new node before the trivial child is the cut
    out.append(case("cut-before-trivial", AK2, "S1", 50, full["nodes"], False))
    assert beam(AK2, "S1", 50, full["nodes"])["status"] != FOUND and full["nodes"] > full["nodes_after"][-1]
    return out


def all_cases():
    from many_common import _scrambled
    cases = []
    for name, p in (("AK2", AK2), ("AK3", AK3)):
        for s in ("S0", "S1", "S2", "S4") + (("S3",) if name == "AK2" else ()):
            for W in (1, 3, 50):
                for cyc in (False, True):
                    cases.append(case(f"ak-{name}", p, s, W, 3000, cyc))
    cases.append(case("roots-trivial", [1, 0, 0, 2, 0, 0], "S0", 3, 100, False))
    cases.append(case("roots-trivial", [-2, 0, 0, 0, 1, 0, 0, 0], "S1", 50, 100, True))
    cases.append(case("roots-dies", [1, 1, 2, 2], "S0", 3, 100, False))
    cases.append(case("roots-budget1", AK2, "S0", 3, 1, False))
    cases.append(case("roots-budget0", AK2, "S0", 3, 0, False))
    with open(os.path.join(HERE, "kat_search_extra.json")) as f:
        raising = [c for c in json.load(f) if c["search_fn"] == "bfs" and c["raises"]]
    for i, c in enumerate(raising[:8]):
        cases.append(case("raise", c["presentation"], ("S0", "S1")[i % 2], (1, 3, 50)[i % 3], 500, c["cyclical"]))
    ms = np.load(os.path.join(PKG_DATA, "all_presentations.npy"))
    for i, r in enumerate(ms[:: len(ms) // MS_ROWS][:MS_ROWS]):
        cases.append(case("ms", repad(r, MS_L), ("S0", "S1")[i % 2], (50, 5, 64)[i % 3], MS_BUDGET, bool(i % 4 == 3)))
    rng = np.random.default_rng(20261020)
    for i in range(8):
        cases.append(case("scr", _scrambled(18, rng, 3 + i), ("S1", "S0")[i % 2], (3, 50)[i % 2], 800, bool(i & 2)))
    cases += cut_cases()
    cases.append(case("long", repad(AK3, 128), "S1q", 5, 1500, False))
    cases.append(case("long", repad(ms[-1], 128), "S1q", 50, 1500, True))
    return cases


SCORED_W = (3, 50, 86, 342)  # 50 | 86 | 342: one width per LDS class of the select kernel


def scored_cases():
    """beam_search_scored.json: real-valued scores.  'mlp' with beam_yardstick's NORM_MEAN / NORM_STD
    passed to the reference and a scorer of NORM_SCORERS on the normalised features; 'seq' with the
    token scorer TOK.  AK(2) at L = 7, AK(3) at L = 18, twelve Miller-Schupp rows at L = 36; W in
    SCORED_W, budgets <= 3,000 (<= 7,000 at W = 342), both flags."""
    from beam_yardstick import NORM_SCORERS
    scorers = [("mlp", s) for s in NORM_SCORERS] + [("seq", "TOK")]

    def scored(name, p, arch, s, W, budget, cyc):
        c = case(name, p, s, W, budget, cyc)
        c.update(arch=arch, norm=arch == "mlp")
        return c

    cases, i = [], 0
    for name, p in (("AK2", AK2), ("AK3", AK3)):
        for arch, s in scorers:
            for W in SCORED_W[:3]:
                cases.append(scored(f"ak-{name}", p, arch, s, W, 3000 - 7 * i, bool(i % 2)))
                i += 1
    for j, (arch, s) in enumerate(scorers):
        cases.append(scored("ak-AK3", AK3, arch, s, 342, 7000 - 11 * j, bool(j % 2)))
    ms = np.load(os.path.join(PKG_DATA, "all_presentations.npy"))
    for j, r in enumerate(ms[17:: len(ms) // 12][:12]):
        arch, s = scorers[j % len(scorers)]
        cases.append(scored("ms", repad(r, MS_L), arch, s, SCORED_W[(j // 2) % 3], 3000 - 100 * j, bool(j % 4 >= 2)))
    cases.append(scored("ms", repad(ms[-1], MS_L), "mlp", "NNEG", 342, 7000, False))
    return cases


def check_not_vacuous(recs):
    kinds = {}
    for r in recs:
        end = "raises" if r["raises"] else "found" if r["ok"] else "budget" if r["nodes_explored"] >= max(
            r["budget"], 1) else "died"
        kinds.setdefault(r["name"].split("-")[0], set()).add(end)
    assert kinds["ak"] == {"found", "budget", "died"}, kinds
    assert kinds["raise"] == {"raises"} and "found" in kinds["scr"] and "found" in kinds["roots"], kinds
    assert {"found", "budget"} <= kinds["ms"], kinds
    by = {r["name"]: r for r in recs}
    assert not by["cut-before-trivial"]["ok"] and by["roots-dies"]["steps"] == 1
    return kinds


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True, help="a checkout of the reference project")
    ap.add_argument("--procs", type=int, default=min(16, os.cpu_count() or 1))
    ap.add_argument("--scored", action="store_true", help="write beam_search_scored.json only")
    args = ap.parse_args()
    cases = scored_cases() if args.scored else all_cases()
    with Pool(args.procs) as pool:
        recs = pool.map(run_case, [(args.reference, c) for c in cases], chunksize=1)
    if args.scored:
        assert not any(r["raises"] for r in recs)
        ends = {"found" if r["ok"] else "budget" if r["nodes_explored"] >= r["budget"] else "died" for r in recs}
        assert ends == {"found", "budget", "died"}, ends
        with open(os.path.join(HERE, "beam_search_scored.json"), "w") as f:
            json.dump(recs, f, separators=(",", ":"))
        print(len(recs), "records", sorted(ends))
        return
    kinds = check_not_vacuous(recs)
    with open(os.path.join(HERE, "beam_search.json"), "w") as f:
        json.dump(recs, f, separators=(",", ":"))
    print(len(recs), "records", {k: sorted(v) for k, v in kinds.items()})


if __name__ == "__main__":
    main()
