"""beam_search over a batch of presentations, scored by the caller's model (csrc/acx_beam.hip,
C-ABI acx_beam_* in include/acx.h): one workgroup owns one search -- node store, visited set,
beam -- and a step of all searches is two launches (expand, select) with the scorer between them,
called once on every live search's candidates together.  Given equal scores, each result equals
the reference's beam_search(p_i, ...) (value_search/value_guided_search.py:417-561, with
solution_cache=None and time_limit=None), paths included: the order-dependent dedup, the budget
cut in the middle of a parent and the stable top-W selection are exact, and the only floats are
the scorer's."""

from __future__ import annotations

import numpy as np

from .. import _lib
from . import _batch_bfs, _cache, _scored

_HANDLES = {}  # (device, L, cyclical) -> (handle, searches, max_nodes_each, max_width)
MAX_WIDTH = _lib.BEAM_MAX_WIDTH
NO_PATH = (False, [])


def _wclass(w):
    return 0 if 12 * w <= 1024 else 1 if 12 * w <= 4096 else 2


# (a wider handle selects in a larger LDS class: reused only within its class)
_BEAM = _batch_bfs._Engine("beam_search_many", "acx_beam", _HANDLES, (_lib.BFS_FOUND, _lib.BFS_CACHED), NO_PATH,
                           extra=("max_width",),
                           reuse=lambda have, want: _wclass(have[0]) == _wclass(want[0]))
# expand writes the candidates' number M, and the searches are over when there are none; a step
# without a verdict adds a node to a search, and a search ends at its budget: budget + 2 steps
_STEPS = _scored._Steps(_BEAM, "expand", "select", lambda M, _: (M, M), 2,
                        (("nodes", np.int64), ("steps", np.int64)))


def release_workspaces() -> None:
    """Free the cached batch workspaces of the beam search."""
    _batch_bfs._release(_BEAM)


def _validate_beam(presentations, scorer, beam_width, max_nodes_to_explore, scorer_input, feat_mean, feat_std,
                   on_error):
    """(states, budgets, widths (N) int32, mean, std as float32 arrays or None) or ValueError; no
    GPU call."""
    states, budgets = _scored._validate_scorer(presentations, scorer, max_nodes_to_explore, scorer_input, on_error,
                                               _BEAM.name)
    N = len(states)
    if np.ndim(beam_width) == 0:
        if isinstance(beam_width, (bool, np.bool_)) or not isinstance(beam_width, (int, np.integer)):
            raise ValueError("beam_width must be an integer or a sequence of integers")
        w = np.full(N, int(beam_width), np.int64)
    else:
        w = np.asarray(beam_width)
        if w.ndim != 1 or len(w) != N or not np.issubdtype(w.dtype, np.integer):
            raise ValueError(f"beam_width must be an integer or a sequence of {N} integers")
        w = w.astype(np.int64)
    if N and (int(w.min()) < 1 or int(w.max()) > MAX_WIDTH):
        raise ValueError(f"beam_width must lie in [1, {MAX_WIDTH}]")
    mean, std = _scored._validate_norm(scorer_input, feat_mean, feat_std)
    return states, budgets, w.astype(np.int32), mean, std


def beam_search_many(presentations, scorer, beam_width=50, max_nodes_to_explore=10000,
                     cyclically_reduce_after_moves=False, scorer_input="features", feat_mean=None, feat_std=None,
                     device=None, on_error="raise", return_stats=False, workspace_bytes=None, solution_cache=None):
    """beam_search of every row of `presentations` ((N, 2L) array, tensor or list of equal-length
    rows), all searches stepping together: a list of (True, path) | (False, []), entry i equal to the
    reference's beam_search(presentations[i], ..., beam_width_i, budget_i) wherever the scorer's
    values order as the reference's model's do.  Prints nothing.

    scorer: called once per step with one device tensor holding the candidates of every live search,
      rows in (search, candidate) order: float32 (M, 14) -- compute_features' values, (f - mean) / std
      when feat_mean and feat_std are given -- or, with scorer_input="tokens", int64 (M, 2L) token
      ids (letter + 2).  It returns (M,) or (M, 1), taken as float32; lower is better.  Ties keep
      candidate order and -0.0 ties with +0.0; a NaN raises ValueError.
    beam_width, max_nodes_to_explore: one value, or one per row (widths 1 .. 1024).
    on_error: a search in which a move raises in the reference makes the call raise AssertionError
      naming the rows ("raise"), or puts None at their positions ("return").
    return_stats: also return a dict of (N) arrays -- status (ACX_BFS_* of include/acx.h;
      ACX_BFS_EXHAUSTED: a step had no candidate), nodes (the reference's nodes_explored), steps.
    workspace_bytes: the most device memory the searches' workspace may take (default: half of the
      free device memory); a larger batch runs as consecutive groups, each with its own steps.
    solution_cache: an acx.SolutionCache (or the reference's dict, uploaded for this call and never
      mutated; pass a SolutionCache to avoid the re-upload).  The root is checked before anything,
      and in every step each child in sequential order, after its trivial test and before its
      visited test, as itself and with either relator rotated (value_guided_search.py:460-464,
      503-511): a hit ends the search with (True, path to that state + the rotation moves + the
      cached path), status ACX_BFS_CACHED and nodes = total_nodes as counted up to that child (1
      and 0 steps for a root hit); a child beyond the step's budget cut is never looked at.  Every
      search of the batch sees the cache as it was when the call began (acx.SolutionCache).  With
      return_stats the dict gains cache_hit, an (N) bool array."""
    states, budgets, widths, mean, std = _validate_beam(presentations, scorer, beam_width, max_nodes_to_explore,
                                                        scorer_input, feat_mean, feat_std, on_error)
    _cache.check(solution_cache, states.shape[1] // 2)
    return _scored._run(_STEPS, states, budgets, (widths,), (int(widths.max()),) if len(widths) else (), scorer,
                        scorer_input, mean, std, cyclically_reduce_after_moves, device, workspace_bytes, on_error,
                        return_stats, solution_cache=solution_cache)


def beam_search(presentation, model, architecture="mlp", feat_mean=None, feat_std=None, beam_width=50,
                max_nodes_to_explore=10000, device=None, cyclically_reduce_after_moves=False, verbose=False,
                solution_cache=None, time_limit=None):
    """The reference's beam_search (value_search/value_guided_search.py:417-561): (solved, path,
    stats) with stats = {'nodes_explored', 'steps'}.  The candidates are scored as _score_states_mlp
    / _score_states_seq score them -- the model on the normalised features ('mlp') or on the token
    ids (any other architecture), then torch.expm1 -- but on `device` (default: the current GPU),
    where `model` must live.  With a real float model the result equals the reference's only where
    the two sides' scores order the same: a GPU's float32 sums are not bit-equal to a CPU's, and a
    near-tie resolved the other way changes the beam.  Everything else -- expansion order, the
    visited set, the budget cut, the stable selection -- is exact.

    solution_cache: an acx.SolutionCache (the reference's dict is refused with NotImplementedError:
    upload it once with acx.SolutionCache.from_dict, or hand it to the batch call, which uploads it
    for that call); on a hit the stats also hold 'cache_hit': True, as the reference's.  time_limit
    is accepted only as None; verbose prints nothing."""
    solved, path, st = _scored._single(
        "beam_search", beam_search_many, presentation, model, architecture, feat_mean, feat_std, solution_cache,
        time_limit, dict(beam_width=beam_width, max_nodes_to_explore=max_nodes_to_explore),
        cyclically_reduce_after_moves=cyclically_reduce_after_moves, device=device)
    stats = {"nodes_explored": st["nodes"], "steps": st["steps"]}
    if st.get("cache_hit"):
        stats["cache_hit"] = True
    return solved, path, stats
