"""A batched search against the loop it replaces: the 1,190 Miller-Schupp presentations (L = 18),
budget 10^4, not cyclical -- what the reference's trivialize_miller_schupp_through_search (and, for
greedy, scripts/parallel_search.py) does, one search per presentation.

    python tools/bench_search_many.py --engine bfs|greedy [--budget N] [--rows N] [--out PATH]

Once as a loop of acx.bfs / acx.greedy_search with engine="device" (one search per call,
csrc/acx_bfs.hip / csrc/acx_greedy.hip) and once as one acx.bfs_many / acx.greedy_search_many call
(csrc/acx_mbfs.hip / csrc/acx_mgreedy.hip), in the same process, each warmed by a full run and then
timed wall-clock, 3 runs (the figure is the best).  The two result lists must be equal (the tool
fails otherwise).  Writes both wall times, their ratio, the launches and the workspace bytes as
JSON (default profiles/bfs_many/bench_bfs_many.json or profiles/greedy_many/bench_greedy_many.json)
and prints the same line.  For greedy it also counts how many of the shipped greedy-solved set
(acx/data/greedy_solved_presentations.npy) are among the solved ones at this budget and
max_relator_length."""
import argparse
import contextlib
import io
import json
import os
import sys
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "ac-solver-caltech_amd"))
import acx  # noqa: E402
from acx import _lib  # noqa: E402
from acx.search import _batch_bfs, _batch_greedy, _device_bfs, _engine  # noqa: E402

# per engine: the one-search call and where it leaves its stats, the batch call, its handles, its
# bytes function, and the names its JSON uses
ENGINES = {
    "bfs": dict(one=acx.bfs, one_stats=_device_bfs, many=acx.bfs_many, handles=_batch_bfs._HANDLES,
                bytes="acx_mbfs_bytes", name="bfs", parents_key="parents_total"),
    "greedy": dict(one=acx.greedy_search, one_stats=_engine, many=acx.greedy_search_many,
                   handles=_batch_greedy._HANDLES, bytes="acx_mgreedy_bytes", name="greedy_search",
                   parents_key="pops_total"),
}

ap = argparse.ArgumentParser()
ap.add_argument("--engine", choices=sorted(ENGINES), required=True)
ap.add_argument("--budget", type=int, default=10 ** 4)
ap.add_argument("--rows", type=int, default=0, help="only the first N presentations (0: all)")
ap.add_argument("--out", default=None)
args = ap.parse_args()
E = ENGINES[args.engine]
if args.out is None:
    args.out = os.path.join(REPO, "profiles", f"{args.engine}_many", f"bench_{args.engine}_many.json")

dev = torch.device("cuda:0")
rows = acx.data.load_initial_states("all").astype(np.int32)
if args.rows:
    rows = rows[: args.rows]
N, L = rows.shape[0], rows.shape[1] // 2


def loop():
    out, nodes = [], []
    with contextlib.redirect_stdout(io.StringIO()):  # the budget message of every search
        for p in rows:
            out.append(E["one"](p, args.budget, device=dev, engine="device"))
            nodes.append(E["one_stats"].LAST_STATS["nodes"])
    return out, nodes


def batch():
    return E["many"](rows, args.budget, device=dev, return_stats=True)


def timed(fn, name):
    res = fn()  # warm-up: workspaces allocated, code loaded
    walls = []
    for _ in range(3):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        res = fn()
        torch.cuda.synchronize()
        walls.append(time.perf_counter() - t0)
        print(f"{name}: {walls[-1] * 1e3:.2f} ms", file=sys.stderr, flush=True)
    return res, walls


def norm(res):
    return [(bool(ok), None if path is None else [tuple(int(v) for v in e) for e in path]) for ok, path in res]


(loop_res, loop_nodes), loop_walls = timed(loop, "loop")
(batch_res, stats), batch_walls = timed(batch, "batch")
assert norm(batch_res) == norm(loop_res), f"{E['many'].__name__} and the loop of acx.{E['one'].__name__} disagree"
on_budget = stats["status"] == _lib.BFS_BUDGET
assert np.array_equal(stats["nodes"][on_budget], np.array(loop_nodes)[on_budget])
solved = np.array([bool(r[0]) for r in batch_res])
h = E["handles"][(0, L, False)]
out = {
    "workload": f"{E['name']} of {N} Miller-Schupp presentations, L = {L}, budget {args.budget}, not cyclical",
    "device": torch.cuda.get_device_name(dev),
    "searches": N, "solved": int(solved.sum()), "left_on_budget": int(on_budget.sum()),
}
if args.engine == "greedy":
    shipped = {p.tobytes() for p in acx.data.load_initial_states("solved").astype(np.int32)}
    in_shipped = np.array([p.tobytes() in shipped for p in rows])
    out.update({"shipped_greedy_solved": int(in_shipped.sum()),
                "shipped_greedy_solved_among_solved": int((solved & in_shipped).sum()),
                "solved_not_in_shipped": int((solved & ~in_shipped).sum())})
out.update({
    "nodes_total": int(stats["nodes"].sum()), E["parents_key"]: int(stats["parents"].sum()),
    "loop_wall_ms": min(loop_walls) * 1e3, "loop_walls_ms": [w * 1e3 for w in loop_walls],
    "batch_wall_ms": min(batch_walls) * 1e3, "batch_walls_ms": [w * 1e3 for w in batch_walls],
    "loop_over_batch": min(loop_walls) / min(batch_walls),
})
if args.engine == "greedy":
    out["batch_slowest_below_loop_fastest"] = bool(max(batch_walls) < min(loop_walls))
out.update({
    "batch_launches": -(-N // h[1]), "batch_workspace_bytes": int(h[1] * getattr(_lib.load(), E["bytes"])(L, h[2])),
    "results_equal": True,
})
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    json.dump(out, f, indent=1)
    f.write("\n")
print(json.dumps(out))
