"""The reference's greedy_search (ac_solver/search/greedy.py:15-121) restated over the CPU oracle's
12-way expansion (oracle.expand12), with heapq on the literal (total, path length, state tuple):
the yardstick of the batched greedy tests.  tests/test_greedy_many_cpu.py checks it against the
reference's own recorded runs."""
import heapq

import numpy as np

from oracle import oracle as O

EXHAUSTED, FOUND, BUDGET, MOVE_ERROR = 0, 1, 2, 3  # ACX_BFS_* of include/acx.h
FAN = 64  # heap fan-out of csrc/acx_mgreedy.hip: its levels hold 1, 64, 4096, ... entries


def greedy(presentation, max_nodes, cyclical=False, shape=False):
    """dict: status, ok, path, raises, nodes (len(tree_nodes) at the ending event), parents (nodes
    popped), min_length, and for the tests that need the search's shape: pops = the popped states
    in order (tuples), nodes_after[i] = len(tree_nodes) after pop i's 12 children,
    frontier_after[i] = len(to_explore) then, same_child = pops that yield one new child twice,
    k0_ties (with shape=True: it scans the frontier at every pop) = pops at which another frontier
    node shares the popped node's total, path length and first 8 letters, success_beats_cut = the
    success came in a pop whose earlier children had already met the budget.  With shape=True
    also runner_up[i] = the (total, path length, state) of the frontier's second entry in heap
    order at pop i (None when the popped node was alone), and stored = the states of tree_nodes in
    the order they were added."""
    start = np.asarray(presentation, np.int32)
    L = len(start) // 2
    total0 = int(np.count_nonzero(start))
    heap = [(total0, 0, tuple(int(x) for x in start), [(-1, total0)])]
    seen = {heap[0][2]}
    stored, runner_up = [heap[0][2]], []
    min_length = total0
    out = dict(status=EXHAUSTED, ok=False, path=None, raises=False, success_beats_cut=False)
    pops, nodes_after, frontier_after, same_child, k0_ties = [], [], [], [], []
    path, a, total = None, -1, total0
    while heap and out["status"] == EXHAUSTED:
        top = heap[0]
        if shape and any(e is not top and e[:2] == top[:2] and e[2][:8] == top[2][:8] for e in heap):
            k0_ties.append(len(pops))
        if shape:
            runner_up.append(min((e[:3] for e in heap if e is not top), default=None))
        _, depth, state, path = heapq.heappop(heap)
        pops.append(state)
        ch, lens, err = (x[0] for x in O.expand12(np.array([state], np.int32), L, cyclical))
        new = set()
        for a in range(12):
            if err[a]:  # ACMove raises (utils.py:264-266)
                out.update(status=MOVE_ERROR, raises=True)
                break
            total = int(lens[a].sum())
            min_length = min(min_length, total)
            if total == 2:
                out.update(status=FOUND, ok=True, path=path + [(a, total)],
                           success_beats_cut=len(seen) >= max_nodes)
                break
            key = tuple(int(x) for x in ch[a])
            if key in new and same_child[-1:] != [len(pops) - 1]:
                same_child.append(len(pops) - 1)
            if key not in seen:
                seen.add(key)
                new.add(key)
                if shape:
                    stored.append(key)
                heapq.heappush(heap, (total, depth + 1, key, path + [(a, total)]))
        else:
            nodes_after.append(len(seen))
            frontier_after.append(len(heap))
            if len(seen) >= max_nodes:
                out["status"] = BUDGET
    if out["status"] in (EXHAUSTED, BUDGET):
        out["path"] = path + [(a, total)]  # greedy.py:121
    out.update(nodes=len(seen), parents=len(pops), min_length=min_length, pops=pops, nodes_after=nodes_after,
               frontier_after=frontier_after, same_child=same_child, k0_ties=k0_ties)
    if shape:
        out.update(runner_up=runner_up, stored=stored)
    return out
