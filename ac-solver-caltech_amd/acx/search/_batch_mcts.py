"""mcts_search over a batch of presentations, scored by the caller's model (csrc/acx_mcts.hip, C-ABI
acx_mcts_* in include/acx.h): one wave owns one search -- node store, visited set, the tree's visit
statistics -- and a step of all searches is two launches (select, backup) with the scorer between
them, called once on every live search's new children together.  Given equal scores, each result
equals the reference's mcts_search(p_i, ...) (value_search/mcts.py:177-314, with
solution_cache=None and time_limit=None), paths, nodes_explored and iterations included: the
statistics are doubles, the UCB1 score is computed in the reference's operation order, and log(N)
comes from a table of math.log's own values."""

from __future__ import annotations

import math

import numpy as np
import torch

from .. import _lib
from . import _batch_bfs, _cache, _scored

_HANDLES = {}  # (device, L, cyclical) -> (handle, searches, max_nodes_each)
NO_PATH = (False, [])

_MCTS = _batch_bfs._Engine("mcts_search_many", "acx_mcts", _HANDLES, (_lib.BFS_FOUND, _lib.BFS_CACHED), NO_PATH)

# log_table[k] = math.log(k) (k >= 1; entry 0 is never read), per device: (host list, device tensor).
# It grows in chunks.  A launch runs at most MCTS_SPIN iterations of a search, and an iteration adds
# one visit to the root, the most visited node: step s needs more than 1 + MCTS_SPIN * (s + 1) entries.
_LOG_CHUNK = 1 << 16
_LOG_TABLES = {}


def _log_table(dev, n):
    """a device table of at least n entries"""
    host, t = _LOG_TABLES.get(dev.index, ([-math.inf], None))
    if t is None or len(host) < n:
        want = -(-n // _LOG_CHUNK) * _LOG_CHUNK
        host = host + [math.log(k) for k in range(len(host), want)]  # math.log: the reference's, not numpy's
        t = torch.tensor(host, dtype=torch.float64, device=dev)
        _LOG_TABLES[dev.index] = (host, t)
    return t


def _select_args(dev, step, c_explore):
    t = _log_table(dev, _lib.MCTS_SPIN * (step + 1) + 2)
    return t.data_ptr(), t.numel(), c_explore


# select writes (M, live); M == 0 with live searches: launches of dead ends.  A launch gives a search
# at least one new node, its ending, or MCTS_SPIN of its at most 50 * budget iterations
_STEPS = _scored._Steps(_MCTS, "select", "backup", lambda M, live: (M, live), lambda cap: cap + 50 * cap // 64 + 3,
                        (("nodes", np.int64), ("iterations", np.int64)), make_args=_select_args)


def release_workspaces() -> None:
    """Free the cached batch workspaces of the MCTS and its log tables."""
    _batch_bfs._release(_MCTS)
    _LOG_TABLES.clear()


def mcts_search_many(presentations, scorer, max_nodes_to_explore=10000, c_explore=1.41,
                     cyclically_reduce_after_moves=False, scorer_input="features", feat_mean=None, feat_std=None,
                     device=None, on_error="raise", return_stats=False, workspace_bytes=None, solution_cache=None):
    """mcts_search of every row of `presentations` ((N, 2L) array, tensor or list of equal-length
    rows), all searches stepping together: a list of (True, path) | (False, []), entry i equal to the
    reference's mcts_search(presentations[i], ..., budget_i) wherever the scorer's values equal the
    reference's model's.  Prints nothing.

    scorer: called once per step with one device tensor holding the new children of the expanded
      leaf of every live search, rows in (search, child) order: float32 (M, 14) -- compute_features'
      values, (f - mean) / std when feat_mean and feat_std are given -- or, with
      scorer_input="tokens", int64 (M, 2L) token ids (letter + 2).  It returns (M,) or (M, 1), taken
      as float32: the value itself (the reference's expm1 of the model's output); the engine clamps
      it at 0.  A NaN or +inf raises ValueError.  The root is never scored -- its value is never
      read -- so the scorer is called once fewer than the reference's model.
    max_nodes_to_explore: one budget, or one per row; it is tested before every iteration, together
      with iterations < 50 * budget, so a budget of 0 or 1 runs no iteration and an iteration
      overshoots it by up to 11 nodes.
    c_explore: the UCB1 constant, a float that is not a NaN.
    on_error: a search in which a move raises in the reference makes the call raise AssertionError
      naming the rows ("raise"), or puts None at their positions ("return").
    return_stats: also return a dict of (N) arrays -- status (ACX_BFS_* of include/acx.h;
      ACX_BFS_BUDGET: the budget was reached, ACX_BFS_EXHAUSTED: 50 * budget iterations were),
      nodes (the reference's nodes_explored), iterations.
    workspace_bytes: the most device memory the searches' workspace may take (default: half of the
      free device memory); a larger batch runs as consecutive groups, each with its own steps.
    solution_cache: an acx.SolutionCache (or the reference's dict, uploaded for this call and never
      mutated; pass a SolutionCache to avoid the re-upload).  The root is checked before the first
      iteration, and after every expansion its new children in action order, the terminal test
      first (mcts.py:224-229, 265-289): a hit ends the search with (True, path to that state + the
      rotation moves + the cached path), status ACX_BFS_CACHED, and nodes counting all of that
      expansion's new children (1 and 0 iterations for a root hit).  Every search of the batch
      sees the cache as it was when the call began (acx.SolutionCache).  With return_stats the
      dict gains cache_hit, an (N) bool array."""
    states, budgets = _scored._validate_scorer(presentations, scorer, max_nodes_to_explore, scorer_input, on_error,
                                               _MCTS.name)
    _cache.check(solution_cache, states.shape[1] // 2)
    mean, std = _scored._validate_norm(scorer_input, feat_mean, feat_std)
    try:
        c = float(c_explore)
    except (TypeError, ValueError) as e:
        raise ValueError(f"c_explore must be a number, not {c_explore!r}") from e
    if math.isnan(c):
        raise ValueError("c_explore must not be a NaN")
    return _scored._run(_STEPS, states, budgets, (), (), scorer, scorer_input, mean, std,
                        cyclically_reduce_after_moves, device, workspace_bytes, on_error, return_stats, margs=c,
                        solution_cache=solution_cache)


def mcts_search(presentation, model, architecture="mlp", feat_mean=None, feat_std=None, max_nodes_to_explore=10000,
                c_explore=1.41, device=None, cyclically_reduce_after_moves=False, verbose=False, solution_cache=None,
                time_limit=None):
    """The reference's mcts_search (value_search/mcts.py:177-314): (solved, path, stats) with stats =
    {'nodes_explored', 'iterations'}.  The new children are scored as evaluate_leaves scores them
    -- the model on the normalised features ('mlp') or on the token ids (any other architecture),
    then torch.expm1, then the clamp at 0 -- but on `device` (default: the current GPU), where
    `model` must live.  With a real float model the result equals the reference's only where the
    two sides' values lead to the same selections; the tree, the visited set and both loop tests
    are exact.  The root is not scored.

    solution_cache: an acx.SolutionCache (the reference's dict is refused with NotImplementedError:
    upload it once with acx.SolutionCache.from_dict, or hand it to the batch call, which uploads it
    for that call); on a hit the stats also hold 'cache_hit': True, as the reference's.  time_limit is accepted only as None; verbose prints
    nothing."""
    solved, path, st = _scored._single(
        "mcts_search", mcts_search_many, presentation, model, architecture, feat_mean, feat_std, solution_cache,
        time_limit, dict(max_nodes_to_explore=max_nodes_to_explore), no_model="a model is needed",
        c_explore=c_explore, cyclically_reduce_after_moves=cyclically_reduce_after_moves, device=device)
    stats = {"nodes_explored": st["nodes"], "iterations": st["iterations"]}
    if st.get("cache_hit"):
        stats["cache_hit"] = True
    return solved, path, stats
