"""tests/golden/greedy_many.json: reference greedy_search runs (ac_solver/search/greedy.py:15-121)
for the batched greedy search (acx.greedy_search_many).

    python tests/golden/make_greedy_many_golden.py --reference ROOT [--procs N]

Two parts, each a list of records {presentation, budget, cyclical, raises, ok, path, nodes}:
  "dataset":  every fifth Miller-Schupp presentation (238 rows, L = 18), budget 2000, not cyclical:
              some are solved, most leave on the budget (greedy returns a path either way).
  "solvable": the scrambled-trivial construction of make_search_many_golden.py -- 160 states k
              random reference ACMoves (without cyclic reduction, none leading back to a state of
              the walk) away from a trivial presentation (L = 18), budgets drawn from
              {50, 1000, 30000}, both cyclical flags -- with k in 1..12: greedy with cyclic
              reduction solves every state up to 5 moves away at every one of the budgets, so the
              BFS fixture's k in 1..5 would leave that flag without a failed search.
The generator asserts that neither part is vacuous (check_not_vacuous).
`nodes` is the count the reference's "Exiting search ..." line prints (None when it prints none).
"""
import argparse
import contextlib
import io
import json
import os
import re
import sys
from multiprocessing import Pool

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden import PKG_DATA, load_reference, to_jsonable  # noqa: E402
from make_search_many_golden import BUDGETS, L  # noqa: E402

DATASET_STRIDE, DATASET_BUDGET = 5, 2000
SOLVABLE_SEED, SOLVABLE_CASES, SOLVABLE_DEPTH = 20261020, 160, 12

_REF = None


def _ref(root):
    global _REF
    if _REF is None:
        _REF = load_reference(root)
    return _REF


def run_case(args):
    root, pres, budget, cyc = args
    ref = _ref(root)
    pres = np.array(pres, np.int8)
    buf = io.StringIO()
    rec = dict(presentation=to_jsonable(pres), budget=int(budget), cyclical=bool(cyc))
    try:
        with contextlib.redirect_stdout(buf):
            ok, path = ref.greedy.greedy_search(presentation=pres, max_nodes_to_explore=int(budget),
                                                cyclically_reduce_after_moves=bool(cyc))
        rec.update(raises=False, ok=bool(ok), path=to_jsonable(path))
    except AssertionError:
        rec.update(raises=True, ok=False, path=None)
    m = re.search(r"number of explored nodes = (\d+)", buf.getvalue())
    rec["nodes"] = int(m.group(1)) if m else None
    return rec


def solvable_inputs(ref):
    """(presentation, budget, cyclical) per case: a trivial presentation scrambled by k reference moves"""
    rng = np.random.default_rng(SOLVABLE_SEED)
    cases = []
    while len(cases) < SOLVABLE_CASES:
        i = len(cases)
        k = 1 + i % SOLVABLE_DEPTH
        cyc = bool((i // SOLVABLE_DEPTH) % 2)
        budget = BUDGETS[int(rng.integers(len(BUDGETS)))]
        s = np.zeros(2 * L, np.int8)
        gens = [int(rng.choice([1, -1])), int(rng.choice([2, -2]))]
        if rng.integers(2):
            gens.reverse()
        s[0], s[L] = gens
        seen = {s.tobytes()}
        for _ in range(k):
            # a move that raises or leads back to a state of this walk is drawn again
            for _ in range(100):
                lens = [int(np.count_nonzero(s[:L])), int(np.count_nonzero(s[L:]))]
                try:
                    t, _ = ref.moves.ACMove(int(rng.integers(12)), s, L, lens, cyclical=False)
                except (AssertionError, IndexError):
                    continue
                t = np.asarray(t, np.int8)
                if t.tobytes() not in seen:
                    seen.add(t.tobytes())
                    s = t
                    break
        assert ref.utils.is_array_valid_presentation(s)
        cases.append((s.tolist(), budget, cyc))
    return cases


def check_not_vacuous(dataset, solvable):
    solved = [r for r in dataset if r["ok"] and len(r["path"]) >= 4]  # root entry + >= 3 moves
    cut = [r for r in dataset if not r["ok"] and r["nodes"] is not None]
    assert len(solved) >= 30, len(solved)
    assert len(cut) >= 60, len(cut)
    counts = [len(solved), len(cut)]
    for cyc in (False, True):
        part = [r for r in solvable if r["cyclical"] == cyc and not r["raises"]]
        found = [r for r in part if r["ok"]]
        failed = [r for r in part if not r["ok"]]
        assert found and failed, (cyc, len(found), len(failed))
        counts += [len(found), len(failed)]
    return counts


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True, help="a checkout of the reference project")
    ap.add_argument("--procs", type=int, default=min(16, os.cpu_count() or 1))
    args = ap.parse_args()
    ref = _ref(args.reference)
    ms = np.load(os.path.join(PKG_DATA, "all_presentations.npy"))
    assert ms.shape[1] == 2 * L
    rows = ms[::DATASET_STRIDE]
    jobs = [(args.reference, r.tolist(), DATASET_BUDGET, False) for r in rows]
    jobs += [(args.reference, p, b, c) for p, b, c in solvable_inputs(ref)]
    with Pool(args.procs) as pool:
        recs = pool.map(run_case, jobs, chunksize=1)
    dataset, solvable = recs[: len(rows)], recs[len(rows):]
    assert not any(r["raises"] for r in dataset)
    counts = check_not_vacuous(dataset, solvable)
    with open(os.path.join(HERE, "greedy_many.json"), "w") as f:
        json.dump(dict(L=L, dataset=dataset, solvable=solvable), f, separators=(",", ":"))
    print("dataset", len(dataset), "solved (>= 3 moves)", counts[0], "budget exits", counts[1])
    print("solvable", len(solvable), "found / failed, not cyclical", counts[2:4], "cyclical", counts[4:6],
          "raises", sum(r["raises"] for r in solvable))


if __name__ == "__main__":
    main()
