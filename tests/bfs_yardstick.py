"""The reference's bfs (ac_solver/search/breadth_first.py:15-97) restated over the CPU oracle's
12-way expansion (oracle.expand12): the yardstick of the batched BFS tests.
tests/test_search_many_cpu.py checks it against the reference's own recorded runs."""
import numpy as np

from oracle import oracle as O

EXHAUSTED, FOUND, BUDGET, MOVE_ERROR = 0, 1, 2, 3  # ACX_BFS_* of include/acx.h
ROUND = 64  # parents a round of csrc/acx_mbfs.hip takes at most


def bfs(presentation, max_nodes, cyclical=False, ahead=256, states=False):
    """dict: status, ok, path, raises, nodes (len(tree_nodes) at the ending event), parents
    expanded, min_length, and for the tests that need the search's shape: nodes_after[i] =
    len(tree_nodes) after parent i, node_parent[j] = the parent that appended node j, dups =
    (parent, node it met again) per child whose state was already seen.  With states=True also
    states = tree_nodes itself, an (n, 2L) int32 array in the order the nodes were stored."""
    start = np.asarray(presentation, np.int32)
    L = len(start) // 2
    nodes, seen, node_parent = [start], {start.tobytes(): 0}, [-1]
    paths = [[(-1, int(np.count_nonzero(start)))]]
    min_length = paths[0][0][1]
    nodes_after, dups, cache, base = [], [], None, 0
    out = dict(status=EXHAUSTED, ok=False, path=None, raises=False)
    at = 0
    while at < len(nodes) and out["status"] == EXHAUSTED:  # to_explore.popleft()
        if cache is None or at >= base + len(cache[0]):  # expand the next queued parents in one call
            base, cache = at, O.expand12(np.stack(nodes[at:at + ahead]), L, cyclical)
        ch, lens, err = (x[at - base] for x in cache)
        for a in range(12):
            if err[a]:  # ACMove raises (utils.py:264-266)
                out.update(status=MOVE_ERROR, raises=True)
                break
            total = int(lens[a].sum())
            min_length = min(min_length, total)
            if total == 2:
                out.update(status=FOUND, ok=True, path=paths[at] + [(a, total)])
                break
            key = ch[a].tobytes()
            if key in seen:
                dups.append((at, seen[key]))
            else:
                seen[key] = len(nodes)
                nodes.append(ch[a].copy())
                node_parent.append(at)
                paths.append(paths[at] + [(a, total)])
        else:
            nodes_after.append(len(nodes))
            if len(nodes) >= max_nodes:
                out["status"] = BUDGET
        at += 1
    out.update(nodes=len(nodes), parents=at, min_length=min_length, nodes_after=nodes_after,
               node_parent=node_parent, dups=dups)
    if states:
        out["states"] = np.stack(nodes)
    return out


def rounds(nodes_after):
    """(head, parents) of the rounds csrc/acx_mbfs.hip takes: the next min(64, queued) parents"""
    out, h, n = [], 0, 1
    while h < len(nodes_after):
        P = min(ROUND, n - h, len(nodes_after) - h)
        out.append((h, P))
        n = nodes_after[h + P - 1]
        h += P
    return out


def round_of(rs, parent):
    return next(i for i, (h, P) in enumerate(rs) if h <= parent < h + P)
