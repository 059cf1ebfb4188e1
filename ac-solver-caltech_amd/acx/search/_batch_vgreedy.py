"""value_guided_greedy_search over a batch of presentations, scored by the caller's model
(csrc/acx_vgreedy.hip, C-ABI acx_vgreedy_* in include/acx.h): one wave owns one search -- node
store, visited set, the heap of (score, path length, node index) -- and a step of all searches is
two launches (pop, push) with the scorer between them, called once on every live search's candidates
together -- or, with an acx.DeviceMLP as the scorer, launches of many pops each in which the device
scores the candidates itself (acx_vgreedy_run_mlp).  Given equal scores, each result equals the reference's
value_guided_greedy_search(p_i, ...) (value_search/value_guided_search.py:253-414, with
solution_cache=None and time_limit=None), paths included: the pop order, the order-dependent dedup
and the once-per-pop budget test are exact, and the only floats are the scorer's."""

from __future__ import annotations

import functools

import numpy as np

from .. import _lib
from .._mlp import DeviceMLP
from . import _batch_bfs, _cache, _scored

_HANDLES = {}  # (device, L, cyclical) -> (handle, searches, max_nodes_each)
NO_PATH = (False, [])

_VGREEDY = _batch_bfs._Engine("value_guided_greedy_search_many", "acx_vgreedy", _HANDLES,
                              (_lib.BFS_FOUND, _lib.BFS_CACHED), NO_PATH)
# pop writes (M, live); M == 0 with live searches: pops whose children were all known.  A pop takes
# one of a search's at most budget + 11 nodes off its heap: budget + 13 steps
_STEPS = _scored._Steps(_VGREEDY, "pop", "push", lambda M, live: (M, live), 13,
                        (("nodes", np.int64), ("steps", np.int64), ("min_length", np.int32)))


def release_workspaces() -> None:
    """Free the cached batch workspaces of the value-guided greedy search."""
    _batch_bfs._release(_VGREEDY)


def value_guided_greedy_search_many(presentations, scorer, max_nodes_to_explore=10000,
                                    cyclically_reduce_after_moves=False, scorer_input="features", feat_mean=None,
                                    feat_std=None, device=None, on_error="raise", return_stats=False,
                                    workspace_bytes=None, solution_cache=None, fused=None, pops_per_launch=4096):
    """value_guided_greedy_search of every row of `presentations` ((N, 2L) array, tensor or list of
    equal-length rows), all searches stepping together: a list of (True, path) | (False, []), entry i
    equal to the reference's value_guided_greedy_search(presentations[i], ..., budget_i) wherever the
    scorer's values order as the reference's model's do.  Prints nothing.

    scorer: called once per step with one device tensor holding the candidates (the new children of
      the popped node) of every live search, rows in (search, candidate) order: float32 (M, 14) --
      compute_features' values, (f - mean) / std when feat_mean and feat_std are given -- or, with
      scorer_input="tokens", int64 (M, 2L) token ids (letter + 2).  It returns (M,) or (M, 1), taken
      as float32; lower is better.  Ties go to the shorter path, then to the node made first, and
      -0.0 ties with +0.0; a NaN raises ValueError.  The root is never scored -- it is the only heap
      entry when it is popped -- so the scorer is called once fewer than the reference's model.  Two
      actions of one pop that give the same new state are one node here, while the reference pushes
      both: the results are the same wherever the scorer gives equal rows equal scores.
    max_nodes_to_explore: one budget, or one per row; it is tested once per pop, after up to 12 new
      nodes, and a budget of 1 still pops the root.
    on_error: a search in which a move raises in the reference makes the call raise AssertionError
      naming the rows ("raise"), or puts None at their positions ("return").
    return_stats: also return a dict of (N) arrays -- status (ACX_BFS_* of include/acx.h;
      ACX_BFS_EXHAUSTED: the heap ran empty), nodes (the reference's nodes_explored), steps (pops),
      min_length.
    workspace_bytes: the most device memory the searches' workspace may take (default: half of the
      free device memory); a larger batch runs as consecutive groups, each with its own steps.
    solution_cache: an acx.SolutionCache (or the reference's dict, uploaded for this call and never
      mutated; pass a SolutionCache to avoid the re-upload).  The root is checked before anything,
      and in every pop each child, after its trivial test and before its visited test, as itself
      and with either relator rotated (value_guided_search.py:326-330, 372-380): a hit ends the
      search with (True, path to that state + the rotation moves + the cached path), status
      ACX_BFS_CACHED, min_length 2 and nodes as for a found search (1 for a root hit).  Every
      search of the batch sees the cache as it was when the call began -- the reference's loop
      backfills between two searches; here the backfill follows the call (acx.SolutionCache).
      With return_stats the dict gains cache_hit, an (N) bool array.
    fused: with an acx.DeviceMLP as the scorer on scorer_input="features", the searches run on the
      device alone: launches of up to pops_per_launch pops of every live search -- pop, features,
      normalisation, the network (csrc/acx_mlp.h), push -- with one host read per launch instead of
      one per pop, and the same results as the stepped loop with that scorer.  None (default): fused
      exactly when it can be; False: the stepped loop; True with any other scorer or input:
      ValueError.  The scores are the network's y, not expm1(y) (acx.DeviceMLP)."""
    can_fuse = isinstance(scorer, DeviceMLP) and scorer_input == "features"
    if fused and not can_fuse:
        raise ValueError("fused=True needs an acx.DeviceMLP as the scorer and scorer_input='features'")
    if int(pops_per_launch) < 1:
        raise ValueError("pops_per_launch must be at least 1")
    fused = (int(pops_per_launch),) if (can_fuse if fused is None else fused) else None
    states, budgets = _scored._validate_scorer(presentations, scorer, max_nodes_to_explore, scorer_input, on_error,
                                               _VGREEDY.name)
    _cache.check(solution_cache, states.shape[1] // 2)
    mean, std = _scored._validate_norm(scorer_input, feat_mean, feat_std)
    return _scored._run(_STEPS, states, budgets, (), (), scorer, scorer_input, mean, std,
                        cyclically_reduce_after_moves, device, workspace_bytes, on_error, return_stats,
                        solution_cache=solution_cache, fused=fused)


def _total_length(f):
    return f[:, 0]


def value_guided_greedy_search(presentation, model=None, architecture="mlp", feat_mean=None, feat_std=None,
                               max_nodes_to_explore=10000, device=None, use_length_priority=False,
                               cyclically_reduce_after_moves=False, verbose=False, solution_cache=None,
                               time_limit=None, fused=False):
    """The reference's value_guided_greedy_search (value_search/value_guided_search.py:253-414):
    (solved, path, stats) with stats = {'nodes_explored', 'min_length'}.  The candidates are scored
    as _score_states_mlp / _score_states_seq score them -- the model on the normalised features
    ('mlp') or on the token ids (any other architecture), then torch.expm1 -- but on `device`
    (default: the current GPU), where `model` must live.  use_length_priority=True runs the same
    engine with the raw total-length feature as the score and ignores `model`.  With a real float
    model the result equals the reference's only where the two sides' scores order the same; the
    expansion order, the visited set and the budget test are exact.  The root is not scored.

    solution_cache: an acx.SolutionCache (the reference's dict is refused with NotImplementedError:
    upload it once with acx.SolutionCache.from_dict, or hand it to the batch call, which uploads it
    for that call); on a hit the stats also hold 'cache_hit': True, as the reference's.  time_limit is accepted only as None; verbose prints
    nothing.

    fused=True: `model` (a FeatureMLP; architecture must be "mlp") becomes an acx.DeviceMLP and the search
    runs on the device alone, ordered by the network's output y instead of expm1(y): the same
    order as the exact scores', without float32 expm1's ties and overflow."""
    many, scorer = value_guided_greedy_search_many, _total_length if use_length_priority else None
    if fused:
        if architecture != "mlp" or use_length_priority:
            raise ValueError("fused=True needs architecture='mlp' and a model")
        if model is None or feat_mean is None or feat_std is None:
            raise ValueError("fused=True needs a model, feat_mean and feat_std")
        scorer = DeviceMLP.from_module(model)
        many = functools.partial(many, feat_mean=feat_mean, feat_std=feat_std, fused=True)
    solved, path, st = _scored._single(
        "value_guided_greedy_search", many, presentation, model, architecture, feat_mean,
        feat_std, solution_cache, time_limit, dict(max_nodes_to_explore=max_nodes_to_explore),
        no_model="a model is needed unless use_length_priority=True", scorer=scorer,
        cyclically_reduce_after_moves=cyclically_reduce_after_moves, device=device)
    stats = {"nodes_explored": st["nodes"], "min_length": st["min_length"]}
    if st.get("cache_hit"):
        stats["cache_hit"] = True
    return solved, path, stats
