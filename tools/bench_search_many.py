"""A batched search against the loop it replaces: the 1,190 Miller-Schupp presentations (L = 18),
budget 10^4, not cyclical -- what the reference's trivialize_miller_schupp_through_search (and, for
greedy, scripts/parallel_search.py) does, one search per presentation.

    python tools/bench_search_many.py --engine bfs|greedy|beam|vgreedy|mcts [--budget N] [--rows N] [--out PATH]

Once as a loop of acx.bfs / acx.greedy_search with engine="device" (one search per call,
csrc/acx_bfs.hip / csrc/acx_greedy.hip) and once as one acx.bfs_many / acx.greedy_search_many call
(csrc/acx_mbfs.hip / csrc/acx_mgreedy.hip), in the same process, each warmed by a full run and then
timed wall-clock, 3 runs (the figure is the best).  The two result lists must be equal (the tool
fails otherwise).  Writes both wall times, their ratio, the launches and the workspace bytes as
JSON (default profiles/bfs_many/bench_bfs_many.json or profiles/greedy_many/bench_greedy_many.json)
and prints the same line.  For greedy it also counts how many of the shipped greedy-solved set
(acx/data/greedy_solved_presentations.npy) are among the solved ones at this budget and
max_relator_length.

--engine beam: the same rows through one acx.beam_search_many call (csrc/acx_beam.hip), W = 50,
scorer S0 = the total length (the first feature), timed the same way, with the split of a step into
expand, gather + features (the host's read of the candidate count falls in it), scorer and select
from HIP events of a further run.  Beside it the same search written with the parent commit's public
API -- ops.expand12 once per step over every live beam, the children copied to the host, the
visited sets, the budget cut and the stable selection in Python -- on every fifth row (238), run
once after a warm-up on 8 rows; its wall time is scaled by rows / 238 to set it beside the batch
call, and the JSON says so.  The results of those 238 rows must be equal.  Writes
profiles/beam_many/bench_beam_many.json.

--engine vgreedy: the same rows through one acx.value_guided_greedy_search_many call
(csrc/acx_vgreedy.hip), scorer S0 = the total length, timed the same way, with the split of a step
into pop, gather + features (the host's read of the candidate count falls in it, or, at a step
without candidates, in the time between steps), scorer and push from HIP events of a further run.
Beside it the same search written with the parent commit's public API -- ops.expand12 once per pop
step over every live search's popped node, the children copied to the host, the heaps (heapq) and the
visited sets in Python -- on every fifth row (238), run once after a warm-up on 8 rows and scaled as
for the beam.  The results of those 238 rows must be equal.  Writes
profiles/vgreedy_many/bench_vgreedy_many.json.

--engine mcts: the same rows through one acx.mcts_search_many call (csrc/acx_mcts.hip), c_explore
1.41, the value of a node = its total length, timed the same way, with the split of a step into
select, gather + features, scorer and backup from HIP events of a further run.  Beside it the same
search written with the parent commit's public API -- ops.expand12 once per iteration over every
live search's selected leaf, the children copied to the host, the trees (visit counts, value sums,
UCB1 with math.log), the visited sets and the backups in Python -- on every fifth row (238), run once
after a warm-up on 8 rows and scaled as for the beam.  The results of those 238 rows must be equal.
Writes profiles/mcts_many/bench_mcts_many.json."""
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
ap.add_argument("--engine", choices=sorted(ENGINES) + ["beam", "vgreedy", "mcts"], required=True)
ap.add_argument("--width", type=int, default=50, help="beam width (--engine beam)")
ap.add_argument("--budget", type=int, default=10 ** 4)
ap.add_argument("--rows", type=int, default=0, help="only the first N presentations (0: all)")
ap.add_argument("--out", default=None)
args = ap.parse_args()
E = ENGINES.get(args.engine)
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


def s0(f):
    return f[:, 0]


class Marks:
    """HIP events at the marks of _scored._run_group: each mark names the phase that has just ended
    ("between": the host's time from the end of a step to the next step's first launch); split()
    gives the milliseconds of the phases in `names` and the steps (marks of the phase `step`)"""

    def __init__(self, step, names):
        self.step, self.names, self.ev = step, names, []

    def mark(self, phase):
        e = torch.cuda.Event(enable_timing=True)
        e.record()
        self.ev.append((phase, e))

    def split(self):
        torch.cuda.synchronize()
        ms = dict.fromkeys(self.names, 0.0)
        for (_, a), (phase, b) in zip(self.ev, self.ev[1:]):
            if phase in ms:
                ms[phase] += a.elapsed_time(b)
        return {"steps": sum(p == self.step for p, _ in self.ev), **{f"{n}_ms": v for n, v in ms.items()}}


def split_of(many, step, names):
    """the step split of one more run of `many`"""
    from acx.search import _scored
    marks = _scored._TIMING = Marks(step, names)
    try:
        many()
    finally:
        _scored._TIMING = None
    return marks.split()


def host_beam(rows, W, budget):
    """beam_search of every row with ops.expand12 as the only device call: [(ok, path)], nodes"""
    n = len(rows)
    beams = [[(r, 0)] for r in rows]
    visited = [{r.tobytes()} for r in rows]
    parent = [{0: None} for _ in rows]
    nodes, live, res = [1] * n, list(range(n)), [(False, [])] * n
    while live:
        live = [q for q in live if beams[q] and nodes[q] < budget]
        if not live:
            break
        par = torch.from_numpy(np.stack([b[0] for q in live for b in beams[q]])).to(dev)
        out = acx.ops.expand12(par, cyclical=False)
        ch, lens, err = (out[k].cpu().numpy() for k in ("children", "lengths", "err"))
        tot = lens.sum(2)
        base, nxt = 0, []
        for q in live:
            new, done = [], False
            for r, (_, pid) in enumerate(beams[q]):
                for a in range(12):
                    assert not err[base + r, a]
                    t = int(tot[base + r, a])
                    if t == 2:
                        path, v = [(a, 2)], pid
                        while parent[q][v] is not None:
                            path.append(parent[q][v][:2])
                            v = parent[q][v][2]
                        res[q], done = (True, path[::-1]), True
                        break
                    key = ch[base + r, a].tobytes()
                    if key not in visited[q]:
                        visited[q].add(key)
                        parent[q][nodes[q]] = (a, t, pid)
                        new.append((ch[base + r, a], nodes[q], t))
                        nodes[q] += 1
                        if nodes[q] >= budget:
                            done = None
                            break
                if done is not False:
                    break
            base += len(beams[q])
            if done:
                continue
            new.sort(key=lambda c: float(c[2]))  # stable
            beams[q] = [(c[0], c[1]) for c in new[:W]]
            if new:
                nxt.append(q)
        live = nxt
    return res, nodes


def bench_beam():
    from acx.search import _batch_beam
    W = args.width

    def many(r=rows):
        return acx.beam_search_many(r, s0, beam_width=W, max_nodes_to_explore=args.budget, device=dev,
                                    return_stats=True)

    (batch_res, stats), batch_walls = timed(many, "batch")
    split = split_of(many, "expand", ("expand", "gather_features", "scorer", "select"))
    sub = rows[::5]
    host_beam(sub[:8], W, args.budget)  # warm-up
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    host_res, host_nodes = host_beam(sub, W, args.budget)
    host_wall = time.perf_counter() - t0
    print(f"host: {host_wall * 1e3:.2f} ms for {len(sub)} rows", file=sys.stderr, flush=True)
    assert norm(host_res) == norm(batch_res[::5]), "beam_search_many and the host-side beam search disagree"
    assert np.array_equal(stats["nodes"][::5], np.array(host_nodes))
    h = _batch_beam._HANDLES[(0, L, False)]
    return {
        "workload": f"beam_search of {N} Miller-Schupp presentations, L = {L}, W = {W}, budget {args.budget}, "
                    "scorer S0 (total length), not cyclical",
        "device": torch.cuda.get_device_name(dev),
        "searches": N, "solved": int(sum(bool(r[0]) for r in batch_res)),
        "left_on_budget": int((stats["status"] == _lib.BFS_BUDGET).sum()),
        "beam_died": int((stats["status"] == _lib.BFS_EXHAUSTED).sum()),
        "nodes_total": int(stats["nodes"].sum()), "steps_max": int(stats["steps"].max()),
        "batch_wall_ms": min(batch_walls) * 1e3, "batch_walls_ms": [w * 1e3 for w in batch_walls],
        "batch_step_split_hip_events": split,
        "host_rows": len(sub), "host_wall_ms": host_wall * 1e3, "host_runs": 1,
        "host_wall_scaled_to_all_rows_ms": host_wall * 1e3 * N / len(sub),
        "host_scaled_note": f"the host-side search ran on every fifth row ({len(sub)}); its wall time is scaled by "
                            f"{N}/{len(sub)} to stand beside the batch call",
        "host_scaled_over_batch": host_wall * N / len(sub) / min(batch_walls),
        "batch_workspace_bytes": int(h[1] * _lib.load().acx_beam_bytes(L, h[2], h[3])),
        "results_equal": True,
    }


def host_vgreedy(rows, budget):
    """value_guided_greedy_search of every row, scored by total length, with ops.expand12 as the only
    device call (one per pop step, over the popped node of every live search): [(ok, path)], nodes,
    min_length"""
    import heapq
    n = len(rows)
    heaps = [[(0.0, 0, 0, r.tobytes())] for r in rows]
    ids = [{r.tobytes(): 0} for r in rows]
    parent = [{0: None} for _ in rows]
    min_len = [int(np.count_nonzero(r)) for r in rows]
    res, live = [(False, [])] * n, list(range(n))
    while live:
        pops = [heapq.heappop(heaps[q]) for q in live]
        par = torch.from_numpy(np.stack([np.frombuffer(p[3], np.int32) for p in pops])).to(dev)
        out = acx.ops.expand12(par, cyclical=False)
        ch, lens, err = (out[k].cpu().numpy() for k in ("children", "lengths", "err"))
        tot = lens.sum(2)
        nxt = []
        for j, q in enumerate(live):
            _, plen, cur, _ = pops[j]
            new, done = [], False
            for a in range(12):
                assert not err[j, a]
                t = int(tot[j, a])
                min_len[q] = min(min_len[q], t)
                if t == 2:
                    path, v = [(a, 2)], cur
                    while parent[q][v] is not None:
                        path.append(parent[q][v][:2])
                        v = parent[q][v][2]
                    res[q], done = (True, path[::-1]), True
                    break
                key = ch[j, a].astype(np.int32).tobytes()
                if key not in ids[q]:
                    new.append((key, a, t))
            if done:
                continue
            for key, a, t in new:  # (twins: both pushed, as the reference does)
                nid = len(parent[q])
                parent[q][nid] = (a, t, cur)
                ids[q][key] = nid
                heapq.heappush(heaps[q], (float(t), plen + 1, nid, key))
            if len(ids[q]) < budget and heaps[q]:
                nxt.append(q)
        live = nxt
    return res, [len(d) for d in ids], min_len


def bench_vgreedy():
    from acx.search import _batch_vgreedy

    def many(r=rows):
        return acx.value_guided_greedy_search_many(r, s0, max_nodes_to_explore=args.budget, device=dev,
                                                   return_stats=True)

    (batch_res, stats), batch_walls = timed(many, "batch")
    split = split_of(many, "pop", ("between", "gather_features", "pop", "push", "scorer"))
    sub = rows[::5]
    host_vgreedy(sub[:8], args.budget)  # warm-up
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    host_res, host_nodes, host_min = host_vgreedy(sub, args.budget)
    host_wall = time.perf_counter() - t0
    print(f"host: {host_wall * 1e3:.2f} ms for {len(sub)} rows", file=sys.stderr, flush=True)
    assert norm(host_res) == norm(batch_res[::5]), "value_guided_greedy_search_many and the host-side search disagree"
    assert np.array_equal(stats["nodes"][::5], np.array(host_nodes))
    assert np.array_equal(stats["min_length"][::5], np.array(host_min))
    h = _batch_vgreedy._HANDLES[(0, L, False)]
    return {
        "workload": f"value_guided_greedy_search of {N} Miller-Schupp presentations, L = {L}, budget {args.budget}, "
                    "scorer S0 (total length), not cyclical",
        "device": torch.cuda.get_device_name(dev),
        "searches": N, "solved": int(sum(bool(r[0]) for r in batch_res)),
        "left_on_budget": int((stats["status"] == _lib.BFS_BUDGET).sum()),
        "heap_ran_empty": int((stats["status"] == _lib.BFS_EXHAUSTED).sum()),
        "nodes_total": int(stats["nodes"].sum()), "pops_total": int(stats["steps"].sum()),
        "pops_max": int(stats["steps"].max()),
        "batch_wall_ms": min(batch_walls) * 1e3, "batch_walls_ms": [w * 1e3 for w in batch_walls],
        "batch_step_split_hip_events": split,
        "host_rows": len(sub), "host_wall_ms": host_wall * 1e3, "host_runs": 1,
        "host_wall_scaled_to_all_rows_ms": host_wall * 1e3 * N / len(sub),
        "host_scaled_note": f"the host-side search ran on every fifth row ({len(sub)}); its wall time is scaled by "
                            f"{N}/{len(sub)} to stand beside the batch call",
        "host_scaled_over_batch": host_wall * N / len(sub) / min(batch_walls),
        "batch_workspace_bytes": int(h[1] * _lib.load().acx_vgreedy_bytes(L, h[2])),
        "results_equal": True,
    }


class _Tree:
    """one search of host_mcts: the reference's nodes as parallel lists"""

    def __init__(self, row):
        self.states, self.total = [row], [int(np.count_nonzero(row))]
        self.parent, self.action, self.children = [None], [None], [[]]
        self.visit, self.vsum, self.prior = [1], [0.0], [0.0]
        self.visited, self.iterations = {row.tobytes()}, 0

    def select(self, c):
        import math
        node = 0
        while self.children[node]:
            kids = self.children[node]
            unvisited = [k for k in kids if self.visit[k] == 0]
            if unvisited:
                node = min(unvisited, key=self.prior.__getitem__)
                continue
            best, logn = -math.inf, math.log(self.visit[node])
            for k in kids:
                score = -(self.vsum[k] / self.visit[k]) + c * math.sqrt(logn / self.visit[k])
                if score > best:
                    best, node_k = score, k
            node = node_k
        return node

    def back_up(self, node, value):
        while node is not None:
            self.visit[node] += 1
            self.vsum[node] += value
            node = self.parent[node]

    def path(self, node):
        p = []
        while self.parent[node] is not None:
            p.append((self.action[node], self.total[node]))
            node = self.parent[node]
        return p[::-1]


def host_mcts(rows, budget, c):
    """mcts_search of every row, the value of a node its total length, with ops.expand12 as the only
    device call (one per iteration, over the selected leaf of every live search): [(ok, path)],
    nodes, iterations"""
    trees = [_Tree(r) for r in rows]
    res, live = [(False, [])] * len(rows), list(range(len(rows)))
    while live:
        live = [q for q in live if len(trees[q].visited) < budget and trees[q].iterations < 50 * budget]
        if not live:
            break
        leaves = []
        for q in live:
            trees[q].iterations += 1
            leaves.append(trees[q].select(c))
        par = torch.from_numpy(np.stack([trees[q].states[v] for q, v in zip(live, leaves)])).to(dev)
        out = acx.ops.expand12(par, cyclical=False)
        ch, lens, err = (out[k].cpu().numpy() for k in ("children", "lengths", "err"))
        tot = lens.sum(2)
        assert not err.any()
        nxt = []
        for j, (q, leaf) in enumerate(zip(live, leaves)):
            t, new = trees[q], []
            for a in range(12):
                state = ch[j, a].astype(np.int32)
                key = state.tobytes()
                if key in t.visited:
                    continue
                t.visited.add(key)
                nid = len(t.states)
                t.states.append(state)
                t.total.append(int(tot[j, a]))
                t.parent.append(leaf)
                t.action.append(a)
                t.children.append([])
                t.visit.append(0)
                t.vsum.append(0.0)
                t.prior.append(float(tot[j, a]))  # the scorer: the total length
                t.children[leaf].append(nid)
                new.append(nid)
            trivial = [v for v in new if t.total[v] == 2]
            if trivial:
                res[q] = (True, t.path(trivial[0]))
                continue
            t.back_up(leaf, min(t.prior[v] for v in new) if new else t.prior[leaf] + 50)
            nxt.append(q)
        live = nxt
    return res, [len(t.visited) for t in trees], [t.iterations for t in trees]


def bench_mcts():
    from acx.search import _batch_mcts
    C = 1.41

    def many(r=rows):
        return acx.mcts_search_many(r, s0, max_nodes_to_explore=args.budget, c_explore=C, device=dev, return_stats=True)

    (batch_res, stats), batch_walls = timed(many, "batch")
    split = split_of(many, "select", ("between", "gather_features", "select", "backup", "scorer"))
    sub = rows[::5]
    host_mcts(sub[:8], args.budget, C)  # warm-up
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    host_res, host_nodes, host_iters = host_mcts(sub, args.budget, C)
    host_wall = time.perf_counter() - t0
    print(f"host: {host_wall * 1e3:.2f} ms for {len(sub)} rows", file=sys.stderr, flush=True)
    assert norm(host_res) == norm(batch_res[::5]), "mcts_search_many and the host-side search disagree"
    assert np.array_equal(stats["nodes"][::5], np.array(host_nodes))
    assert np.array_equal(stats["iterations"][::5], np.array(host_iters))
    h = _batch_mcts._HANDLES[(0, L, False)]
    return {
        "workload": f"mcts_search of {N} Miller-Schupp presentations, L = {L}, budget {args.budget}, c_explore {C}, "
                    "value = total length, not cyclical",
        "device": torch.cuda.get_device_name(dev),
        "searches": N, "solved": int(sum(bool(r[0]) for r in batch_res)),
        "left_on_budget": int((stats["status"] == _lib.BFS_BUDGET).sum()),
        "iteration_cap_reached": int((stats["status"] == _lib.BFS_EXHAUSTED).sum()),
        "nodes_total": int(stats["nodes"].sum()), "iterations_total": int(stats["iterations"].sum()),
        "iterations_max": int(stats["iterations"].max()),
        "batch_wall_ms": min(batch_walls) * 1e3, "batch_walls_ms": [w * 1e3 for w in batch_walls],
        "batch_step_split_hip_events": split,
        "host_rows": len(sub), "host_wall_ms": host_wall * 1e3, "host_runs": 1,
        "host_wall_scaled_to_all_rows_ms": host_wall * 1e3 * N / len(sub),
        "host_scaled_note": f"the host-side search ran on every fifth row ({len(sub)}); its wall time is scaled by "
                            f"{N}/{len(sub)} to stand beside the batch call",
        "host_scaled_over_batch": host_wall * N / len(sub) / min(batch_walls),
        "batch_workspace_bytes": int(h[1] * _lib.load().acx_mcts_bytes(L, h[2])),
        "results_equal": True,
    }


def write(out):
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


if args.engine in ("beam", "vgreedy", "mcts"):
    write({"beam": bench_beam, "vgreedy": bench_vgreedy, "mcts": bench_mcts}[args.engine]())
    sys.exit(0)

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
write(out)
