"""The batched BFS against the loop it replaces: the 1,190 Miller-Schupp presentations (L = 18),
budget 10^4, not cyclical -- what the reference's trivialize_miller_schupp_through_search does,
one bfs per presentation.

    python tools/bench_bfs_many.py [--budget N] [--rows N] [--out PATH]

Once as a loop of acx.bfs(engine="device") (one search per call, csrc/acx_bfs.hip) and once as one
acx.bfs_many call (csrc/acx_mbfs.hip), in the same process, each warmed by a full run and then
timed wall-clock, best of 3.  The two result lists must be equal (the tool fails otherwise).
Writes both wall times and their ratio as JSON (default profiles/bfs_many/bench_bfs_many.json) and
prints the same line."""
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
from acx.search import _batch_bfs, _device_bfs  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--budget", type=int, default=10 ** 4)
ap.add_argument("--rows", type=int, default=0, help="only the first N presentations (0: all)")
ap.add_argument("--out", default=os.path.join(REPO, "profiles", "bfs_many", "bench_bfs_many.json"))
args = ap.parse_args()

dev = torch.device("cuda:0")
rows = acx.data.load_initial_states("all").astype(np.int32)
if args.rows:
    rows = rows[: args.rows]
N, L = rows.shape[0], rows.shape[1] // 2


def loop():
    out, nodes = [], []
    with contextlib.redirect_stdout(io.StringIO()):  # the budget message of every search
        for p in rows:
            out.append(acx.bfs(p, args.budget, device=dev, engine="device"))
            nodes.append(_device_bfs.LAST_STATS["nodes"])
    return out, nodes


def batch():
    return acx.bfs_many(rows, args.budget, device=dev, return_stats=True)


def timed(fn):
    res = fn()  # warm-up: workspaces allocated, code loaded
    walls = []
    for _ in range(3):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        res = fn()
        torch.cuda.synchronize()
        walls.append(time.perf_counter() - t0)
    return res, walls


(loop_res, loop_nodes), loop_walls = timed(loop)
(batch_res, stats), batch_walls = timed(batch)
assert batch_res == loop_res, "bfs_many and the loop of acx.bfs disagree"
on_budget = stats["status"] == _lib.BFS_BUDGET
assert np.array_equal(stats["nodes"][on_budget], np.array(loop_nodes)[on_budget])
h = _batch_bfs._HANDLES[(0, L, False)]
out = {
    "workload": f"bfs of {N} Miller-Schupp presentations, L = {L}, budget {args.budget}, not cyclical",
    "device": torch.cuda.get_device_name(dev),
    "searches": N, "solved": int(sum(r[0] for r in batch_res)), "left_on_budget": int(on_budget.sum()),
    "nodes_total": int(stats["nodes"].sum()), "parents_total": int(stats["parents"].sum()),
    "loop_wall_ms": min(loop_walls) * 1e3, "loop_walls_ms": [w * 1e3 for w in loop_walls],
    "batch_wall_ms": min(batch_walls) * 1e3, "batch_walls_ms": [w * 1e3 for w in batch_walls],
    "loop_over_batch": min(loop_walls) / min(batch_walls),
    "batch_launches": -(-N // h[1]), "batch_workspace_bytes": int(h[1] * _lib.load().acx_mbfs_bytes(L, h[2])),
    "results_equal": True,
}
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    json.dump(out, f, indent=1)
    f.write("\n")
print(json.dumps(out))
