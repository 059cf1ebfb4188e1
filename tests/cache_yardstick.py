"""The reference's solution cache restated literally (value_search/value_guided_search.py:100-250:
_check_cache_with_rotations, _expand_cache_with_rotations, backfill_solution_cache), over the
oracle's move; and the two searches that read it, restated from their yardsticks' parts: the
value-guided greedy search with use_length_priority=True (:253-414) and the beam search scored by
the total length (:417-561), each with what a cache adds to it.
tests/test_cache_cpu.py checks that this reproduces every record of tests/golden/cache_*.{npz,json}
(make_golden_cache.py: the reference's own functions); the GPU tests compare acx.SolutionCache with it
where the fixture has no record.  Plain dicts and lists, as the reference's."""
import heapq

import numpy as np

from oracle import oracle as O

# (relator, generator g) -> the move r_i -> g r_i g^-1 (:119-122)
CONJ_MOVE = {(0, 1): 7, (0, -1): 11, (0, 2): 9, (0, -2): 5, (1, 1): 8, (1, -1): 4, (1, 2): 10, (1, -2): 6}


def _tup(state):
    return tuple(int(x) for x in state)


def rotations(state_tup, mrl):
    """the rotation variants of a state in the reference's order: (rel, k, nz, rotated tuple) for
    relator 0 then 1, k = 1 .. n - 1; a relator of one letter, or one whose ends cancel, has none"""
    state = np.array(state_tup, dtype=np.int8)
    for rel in range(2):
        offset = rel * mrl
        relator = state[offset:offset + mrl]
        nz = relator[relator != 0]
        n = len(nz)
        if n <= 1 or nz[-1] + nz[0] == 0:
            continue
        for k in range(1, n):
            rotated = state.copy()
            rotated[offset:offset + n] = np.concatenate([nz[k:], nz[:k]])
            yield rel, k, nz, _tup(rotated)


def check(state_tup, mrl, cache):
    """_check_cache_with_rotations: (path, rel, k) of the first hit, or None"""
    state_tup = _tup(state_tup)
    if state_tup in cache:
        return list(cache[state_tup]), 0, 0
    total = int(np.count_nonzero(np.array(state_tup)))
    for rel, k, nz, rot in rotations(state_tup, mrl):
        if rot in cache:
            moves = [(CONJ_MOVE[(rel, -int(nz[j]))], total) for j in range(k)]
            return moves + list(cache[rot]), rel, k
    return None


def expand(cache, state_tup, suffix, mrl):
    """_expand_cache_with_rotations"""
    total = int(np.count_nonzero(np.array(state_tup)))
    for rel, k, nz, rot in rotations(state_tup, mrl):
        if rot not in cache:
            undo = [(CONJ_MOVE[(rel, int(nz[j]))], total) for j in range(k)]
            cache[rot] = list(reversed(undo)) + suffix


def backfill(cache, presentation, path, cyclically_reduce=False, expand_rotations=True):
    """backfill_solution_cache; a raising move raises AssertionError, the partial fill kept, as the
    reference does"""
    state = np.array(presentation, dtype=np.int32)
    mrl = len(state) // 2
    for i in range(len(path)):
        tup = _tup(state)
        suffix = list(path[i:])
        if tup not in cache:
            cache[tup] = suffix
        if expand_rotations:
            expand(cache, tup, suffix, mrl)
        state, _, err = O.move(state, mrl, int(path[i][0]), cyclically_reduce)
        assert err == 0, f"a move produced an invalid presentation at step {i}"
    return cache


def vgreedy_length(presentation, max_nodes, cyclical=False, cache=None):
    """value_guided_greedy_search(..., use_length_priority=True, solution_cache=cache):
    (ok, path, stats) with the reference's stats dict; a raising move raises AssertionError"""
    start = np.asarray(presentation, np.int32)
    L = len(start) // 2
    root = _tup(start)
    total0 = int(np.count_nonzero(start))
    parent = {0: (None, total0, None)}
    state_to_id = {root: 0}
    next_id = 1

    def path_to(node):
        path = []
        while node is not None:
            action, length, par = parent[node]
            if par is None:
                break
            path.append((action, length))
            node = par
        path.reverse()
        return path

    if cache is not None:
        hit = check(root, L, cache)
        if hit is not None:
            return True, hit[0], {"nodes_explored": 1, "min_length": 2, "cache_hit": True}
    heap = [(float(total0), 0, 0, root)]
    min_length = total0
    while heap:
        _, depth, cur, state = heapq.heappop(heap)
        ch, lens, err = O.expand12(np.array(state, np.int32), L, cyclical)
        children = []
        for action in range(12):
            assert err[0, action] == 0, "a move produced an invalid presentation"
            new_length = int(lens[0, action].sum())
            tup = _tup(ch[0, action])
            min_length = min(min_length, new_length)
            if new_length == 2:
                return True, path_to(cur) + [(action, new_length)], {"nodes_explored": len(state_to_id),
                                                                      "min_length": min_length}
            if cache is not None:
                hit = check(tup, L, cache)
                if hit is not None:
                    return True, path_to(cur) + [(action, new_length)] + hit[0], {
                        "nodes_explored": len(state_to_id), "min_length": 2, "cache_hit": True}
            if tup not in state_to_id:
                children.append((action, new_length, tup))
        for action, new_length, tup in children:
            node = next_id
            next_id += 1
            parent[node] = (action, new_length, cur)
            state_to_id[tup] = node
            heapq.heappush(heap, (float(new_length), depth + 1, node, tup))
        if len(state_to_id) >= max_nodes:
            break
    return False, [], {"nodes_explored": len(state_to_id), "min_length": min_length}


def beam_length(presentation, width, max_nodes, cyclical=False, cache=None, info=None):
    """beam_search(..., solution_cache=cache) with the total length as the score (a stable sort by
    it, as expm1 of a model that returns it sorts): (ok, path, stats) with the reference's stats.
    info: a dict that receives rank (the place in the beam of the parent whose child hit the cache)
    and late (the first new children of parents at places >= 64: the engine's second pass)"""
    start = np.asarray(presentation, np.int32)
    L = len(start) // 2
    root = _tup(start)
    if cache is not None:
        hit = check(root, L, cache)
        if hit is not None:
            return True, hit[0], {"nodes_explored": 1, "steps": 0, "cache_hit": True}
    parent = {0: (None, int(np.count_nonzero(start)), None)}

    def path_to(node):
        path = []
        while parent[node][2] is not None:
            action, length, node = parent[node]
            path.append((action, length))
        path.reverse()
        return path

    beam, visited, total, step, next_id = [(root, 0)], {root}, 1, 0, 1
    while beam and total < max_nodes:
        step += 1
        children = []
        for rank, (state, node) in enumerate(beam):
            ch, lens, err = O.expand12(np.array(state, np.int32), L, cyclical)
            for action in range(12):
                assert err[0, action] == 0, "a move produced an invalid presentation"
                new_length = int(lens[0, action].sum())
                tup = _tup(ch[0, action])
                if new_length == 2:
                    return True, path_to(node) + [(action, new_length)], {"nodes_explored": total, "steps": step}
                if cache is not None:
                    hit = check(tup, L, cache)
                    if hit is not None:
                        if info is not None:
                            info["rank"] = rank
                        return True, path_to(node) + [(action, new_length)] + hit[0], {
                            "nodes_explored": total, "steps": step, "cache_hit": True}
                if tup not in visited:
                    if info is not None and rank >= 64 and len(info.setdefault("late", [])) < 8:
                        info["late"].append(tup)
                    visited.add(tup)
                    total += 1
                    parent[next_id] = (action, new_length, node)
                    children.append((new_length, tup, next_id))
                    next_id += 1
                    if total >= max_nodes:
                        break
            if total >= max_nodes:
                break
        if not children:
            break
        children.sort(key=lambda c: c[0])
        beam = [(c[1], c[2]) for c in children[:width]]
    return False, [], {"nodes_explored": total, "steps": step}
