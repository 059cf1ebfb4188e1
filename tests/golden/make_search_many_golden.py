"""tests/golden/search_many.json: reference bfs runs (ac_solver/search/breadth_first.py:15-97) for
the batched BFS (acx.bfs_many).

    python tests/golden/make_search_many_golden.py --reference ROOT [--procs N]

Two parts, each a list of records {presentation, budget, cyclical, raises, ok, path, nodes}:
  "dataset":  every fifth Miller-Schupp presentation (238 rows, L = 18), budget 3000, not cyclical.
              Every one of them leaves on the budget: the part pins the dedup and the budget cut.
  "solvable": 160 states k in 1..5 random reference ACMoves (without cyclic reduction, none
              leading back to a state of the walk) away from a trivial presentation (L = 18),
              budgets drawn from {50, 1000, 30000}, both cyclical flags.  Every AC move has an
              inverse among the 12, so bfs solves them within 12^k nodes; the small budgets cut
              some.  The generator asserts the part is not vacuous (check_not_vacuous).
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

L = 18
DATASET_STRIDE, DATASET_BUDGET = 5, 3000
SOLVABLE_SEED, SOLVABLE_CASES = 20261020, 160
BUDGETS = (50, 1000, 30000)

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
            ok, path = ref.bfs.bfs(presentation=pres, max_nodes_to_explore=int(budget),
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
        k = 1 + i % 5
        cyc = bool((i // 5) % 2)
        budget = BUDGETS[int(rng.integers(len(BUDGETS)))]
        s = np.zeros(2 * L, np.int8)
        gens = [int(rng.choice([1, -1])), int(rng.choice([2, -2]))]
        if rng.integers(2):
            gens.reverse()
        s[0], s[L] = gens
        seen = {s.tobytes()}
        for _ in range(k):
            # scrambled without cyclic reduction for both flags (with it a conjugation of a short
            # relator is undone at once and every state stays a move or two from trivial); a move
            # that raises or leads back to a state of this walk is drawn again
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


def check_not_vacuous(recs):
    for cyc in (False, True):
        part = [r for r in recs if r["cyclical"] == cyc]
        solved = [r for r in part if r["ok"] and len(r["path"]) >= 4]  # root entry + >= 3 moves
        cut = [r for r in part if not r["ok"] and r["nodes"] is not None]
        assert solved and cut, (cyc, len(solved), len(cut))
    solved = [r for r in recs if r["ok"] and len(r["path"]) >= 4]
    cut = [r for r in recs if not r["ok"] and r["nodes"] is not None]
    assert len(solved) >= 20, len(solved)
    assert len(cut) >= 10, len(cut)
    return len(solved), len(cut)


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
    assert all(not r["ok"] and not r["raises"] and r["nodes"] is not None for r in dataset)
    n_solved, n_cut = check_not_vacuous(solvable)
    with open(os.path.join(HERE, "search_many.json"), "w") as f:
        json.dump(dict(L=L, dataset=dataset, solvable=solvable), f, separators=(",", ":"))
    print("dataset", len(dataset), "first nodes", dataset[0]["nodes"])
    print("solvable", len(solvable), "solved (>= 3 moves)", n_solved, "budget exits", n_cut,
          "raises", sum(r["raises"] for r in solvable))


if __name__ == "__main__":
    main()
