"""One refinement round with the solution cache: the 1,190 Miller-Schupp presentations (L = 18),
budget 10^4, not cyclical, scorer = the total length -- the setup of tools/bench_search_many.py
--engine vgreedy -- searched, backfilled, and searched again.

    python tools/bench_cache.py [--budget N] [--rows N] [--out PATH]

  1. acx.value_guided_greedy_search_many without a cache: wall time, best of 3 after a warm-up.
  2. acx.SolutionCache.backfill_many of the solved rows (expand_rotations=True): wall time of a fill
     into a fresh cache, best of 3; the entries, the rows of the key store, the bytes; beside it the
     same backfill on the host by tests/cache_yardstick.py (a literal restatement of the
     reference's, over the C oracle's move), once, and the two dicts must be equal.
  3. The call again with the cache: wall time, best of 3; the split of a step into pop, gather +
     features, scorer and push from HIP events of a further run, next to the same split of step 1's
     call; the rows solved, and how many of them by a hit (at the root, at a child).
Writes profiles/cache/bench_cache.json and prints the same line.  Nothing here asserts a ratio."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (os.path.join(REPO, "ac-solver-caltech_amd"), os.path.join(REPO, "tests"), REPO):
    sys.path.insert(0, _p)
import acx  # noqa: E402
from acx import _lib  # noqa: E402
from acx.search import _scored  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--budget", type=int, default=10 ** 4)
ap.add_argument("--rows", type=int, default=0, help="only the first N presentations (0: all)")
ap.add_argument("--out", default=os.path.join(REPO, "profiles", "cache", "bench_cache.json"))
ap.add_argument("--no-host", action="store_true", help="skip the host backfill (and the comparison of the dicts)")
args = ap.parse_args()

dev = torch.device("cuda:0")
rows = acx.data.load_initial_states("all").astype(np.int32)
if args.rows:
    rows = rows[: args.rows]
N, L = rows.shape[0], rows.shape[1] // 2
PHASES = ("pop", "gather_features", "scorer", "push", "between")


def s0(f):
    return f[:, 0]


def search(cache):
    return acx.value_guided_greedy_search_many(rows, s0, args.budget, device=dev, return_stats=True, solution_cache=cache)


def timed(fn, name, warm=True):
    if warm:
        fn()
    walls, res = [], None
    for _ in range(3):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        res = fn()
        torch.cuda.synchronize()
        walls.append(time.perf_counter() - t0)
        print(f"{name}: {walls[-1] * 1e3:.2f} ms", file=sys.stderr, flush=True)
    return res, walls


class Marks:
    def __init__(self):
        self.ev = []

    def mark(self, phase):
        e = torch.cuda.Event(enable_timing=True)
        e.record()
        self.ev.append((phase, e))

    def split(self):
        torch.cuda.synchronize()
        ms = dict.fromkeys(PHASES, 0.0)
        for (_, a), (phase, b) in zip(self.ev, self.ev[1:]):
            ms[phase] += a.elapsed_time(b)
        steps = sum(p == "pop" for p, _ in self.ev)
        return {"steps": steps, **{f"{n}_ms": round(v, 3) for n, v in ms.items()},
                "pop_us_per_step": round(1e3 * ms["pop"] / max(steps, 1), 3)}


def split_of(fn):
    marks = _scored._TIMING = Marks()
    try:
        fn()
    finally:
        _scored._TIMING = None
    return marks.split()


(res0, st0), walls0 = timed(lambda: search(None), "no cache")
split0 = split_of(lambda: search(None))
solved = [i for i, r in enumerate(res0) if r[0]]
pres, paths = rows[solved], [res0[i][1] for i in solved]


def fill():
    return acx.SolutionCache(L, dev).backfill_many(pres, paths)


cache, walls_fill = timed(fill, "backfill_many")
info = cache._info()
host_s = None
if not args.no_host:
    import cache_yardstick as CY
    t0 = time.perf_counter()
    d = {}
    for p, path in zip(pres, paths):
        CY.backfill(d, p, path)
    host_s = time.perf_counter() - t0
    got = cache.to_dict()
    assert got == d, "the device cache and the host backfill differ"

(res1, st1), walls1 = timed(lambda: search(cache), "with the cache")
split1 = split_of(lambda: search(cache))
hit = st1["cache_hit"]
out = {
    "searches": N, "L": L, "budget": args.budget, "scorer": "S0 (total length)",
    "no_cache_wall_ms": round(min(walls0) * 1e3, 2), "no_cache_wall_ms_runs": [round(w * 1e3, 2) for w in walls0],
    "no_cache_wall_ms_recorded_for_the_parent": 197.5,
    "no_cache_solved": len(solved), "no_cache_split": split0,
    "backfill_paths": len(paths), "backfill_path_steps": int(sum(len(p) for p in paths)),
    "backfill_wall_ms": round(min(walls_fill) * 1e3, 2), "backfill_wall_ms_runs": [round(w * 1e3, 2) for w in walls_fill],
    "backfill_host_yardstick_s": None if host_s is None else round(host_s, 2),
    "cache_entries": info["entries"], "cache_store_rows": info["rows"], "cache_capacity": info["capacity"],
    "cache_bytes": int(_lib.load().acx_cache_bytes(L, info["capacity"])),
    "cache_wall_ms": round(min(walls1) * 1e3, 2), "cache_wall_ms_runs": [round(w * 1e3, 2) for w in walls1],
    "cache_solved": int(sum(bool(r[0]) for r in res1)), "cache_hits": int(hit.sum()),
    "cache_root_hits": int((hit & (st1["steps"] == 0)).sum()), "cache_split": split1,
    "nodes_no_cache": int(st0["nodes"].sum()), "nodes_cache": int(st1["nodes"].sum()),
    "version": _lib.load().acx_version().decode(),
}
os.makedirs(os.path.dirname(args.out), exist_ok=True)
with open(args.out, "w") as f:
    json.dump(out, f, indent=1)
print(json.dumps(out))
