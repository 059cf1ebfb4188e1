"""value_guided_greedy_search over a batch of presentations, scored by the caller's model
(csrc/acx_vgreedy.hip, C-ABI acx_vgreedy_* in include/acx.h): one wave owns one search -- node
store, visited set, the heap of (score, path length, node index) -- and a step of all searches is
two launches (pop, push) with the scorer between them, called once on every live search's candidates
together.  Given equal scores, each result equals the reference's
value_guided_greedy_search(p_i, ...) (value_search/value_guided_search.py:253-414, with
solution_cache=None and time_limit=None), paths included: the pop order, the order-dependent dedup
and the once-per-pop budget test are exact, and the only floats are the scorer's."""

from __future__ import annotations

import numpy as np
import torch

from .. import _lib, ops
from . import _batch_bfs
from ._batch_beam import _scores, _validate_norm, _validate_scorer

_HANDLES = {}  # (device, L, cyclical) -> (handle, searches, max_nodes_each)
NO_PATH = (False, [])
_TIMING = None  # tools/bench_search_many.py: an object whose mark(phase) is called after each phase of a step

_VGREEDY = _batch_bfs._Engine("value_guided_greedy_search_many", "acx_vgreedy", _HANDLES, (_lib.BFS_FOUND,), NO_PATH)


def release_workspaces() -> None:
    """Free the cached batch workspaces of the value-guided greedy search."""
    _batch_bfs._release(_VGREEDY)


def value_guided_greedy_search_many(presentations, scorer, max_nodes_to_explore=10000,
                                    cyclically_reduce_after_moves=False, scorer_input="features", feat_mean=None,
                                    feat_std=None, device=None, on_error="raise", return_stats=False,
                                    workspace_bytes=None):
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
      free device memory); a larger batch runs as consecutive groups, each with its own steps."""
    states, budgets = _validate_scorer(presentations, scorer, max_nodes_to_explore, scorer_input, on_error,
                                       _VGREEDY.name)
    mean, std = _validate_norm(scorer_input, feat_mean, feat_std)
    N, L = states.shape[0], states.shape[1] // 2
    stats = dict(status=np.zeros(N, np.int32), nodes=np.zeros(N, np.int64), steps=np.zeros(N, np.int64),
                 min_length=np.zeros(N, np.int32))
    results = [NO_PATH] * N
    if N:
        dev, lib, cyc = _batch_bfs._device(device), _lib.load(), bool(cyclically_reduce_after_moves)
        cap = int(budgets.max())
        group = _batch_bfs._group_size(_VGREEDY, lib, dev, L, cyc, N, cap, workspace_bytes)
        for g0 in range(0, N, group):
            g1 = min(N, g0 + group)
            _run_group(lib, dev, L, cyc, states[g0:g1], budgets[g0:g1], group, cap, scorer, scorer_input, mean, std,
                       g0, stats, results)
    nan = np.nonzero(stats["status"] == _lib.BEAM_NAN)[0]
    if len(nan):
        raise ValueError(f"{_VGREEDY.name}: the scorer returned NaN in searches {nan.tolist()}")
    _batch_bfs._check_status("acx_vgreedy", stats["status"])
    return _batch_bfs._finish(_VGREEDY, results, stats, on_error, return_stats)


def _run_group(lib, dev, L, cyc, states, budgets, n_cap, cap, scorer, scorer_input, mean, std, g0, stats, results):
    n, kw = len(states), _lib.key_words(L)
    h = _batch_bfs._handle(_VGREEDY, lib, dev, L, cyc, n_cap, cap)
    stream = torch.cuda.current_stream(dev).cuda_stream
    with torch.cuda.device(dev):
        st = torch.from_numpy(states).to(dev)
        bd = torch.from_numpy(budgets).to(dev)
        mean_d, std_d = (None if x is None else torch.from_numpy(x).to(dev) for x in (mean, std))
        pair = torch.zeros(2, dtype=torch.int64, device=dev)
        _lib.check(lib.acx_vgreedy_begin(h, st.data_ptr(), bd.data_ptr(), n, stream), "acx_vgreedy_begin")
        mark = (lambda phase: None) if _TIMING is None else _TIMING.mark
        # a pop takes one of a search's at most budget + 11 nodes off its heap
        for _ in range(cap + 13):
            mark("between")
            _lib.check(lib.acx_vgreedy_pop(h, pair.data_ptr(), stream), "acx_vgreedy_pop")
            mark("pop")
            M, live = pair.tolist()  # the step's one host synchronisation
            if live == 0:
                break
            if M == 0:  # pops whose children were all known: nothing to score
                continue
            keys = torch.empty((M, kw), dtype=torch.int64, device=dev)
            _lib.check(lib.acx_vgreedy_gather(h, keys.data_ptr(), M, stream), "acx_vgreedy_gather")
            if scorer_input == "features":
                x = ops.features(keys=keys, L=L, mean=mean_d, std=std_d)
            else:
                x = ops.token_ids(keys=keys, L=L)
            mark("gather_features")
            y = _scores(scorer, x, M)
            mark("scorer")
            _lib.check(lib.acx_vgreedy_push(h, y.data_ptr(), M, stream), "acx_vgreedy_push")
            mark("push")
        else:
            raise _lib.ACXError("acx_vgreedy: the searches did not end within their budgets")
        status = torch.empty(n, dtype=torch.int32, device=dev)
        min_len = torch.empty(n, dtype=torch.int32, device=dev)
        nodes, steps, plen = (torch.empty(n, dtype=torch.int64, device=dev) for _ in range(3))
        _lib.check(lib.acx_vgreedy_finish(h, status.data_ptr(), nodes.data_ptr(), steps.data_ptr(),
                                          min_len.data_ptr(), plen.data_ptr(), stream), "acx_vgreedy_finish")
        stats["status"][g0:g0 + n] = _batch_bfs._read_results(_VGREEDY, lib, h, dev, stream, g0, status, plen, results)
        stats["nodes"][g0:g0 + n] = nodes.cpu().numpy()
        stats["steps"][g0:g0 + n] = steps.cpu().numpy()
        stats["min_length"][g0:g0 + n] = min_len.cpu().numpy()


def _total_length(f):
    return f[:, 0]


def value_guided_greedy_search(presentation, model=None, architecture="mlp", feat_mean=None, feat_std=None,
                               max_nodes_to_explore=10000, device=None, use_length_priority=False,
                               cyclically_reduce_after_moves=False, verbose=False, solution_cache=None,
                               time_limit=None):
    """The reference's value_guided_greedy_search (value_search/value_guided_search.py:253-414):
    (solved, path, stats) with stats = {'nodes_explored', 'min_length'}.  The candidates are scored
    as _score_states_mlp / _score_states_seq score them -- the model on the normalised features
    ('mlp') or on the token ids (any other architecture), then torch.expm1 -- but on `device`
    (default: the current GPU), where `model` must live.  use_length_priority=True runs the same
    engine with the raw total-length feature as the score and ignores `model`.  With a real float
    model the result equals the reference's only where the two sides' scores order the same; the
    expansion order, the visited set and the budget test are exact.  The root is not scored.

    solution_cache and time_limit are accepted only as None; verbose prints nothing."""
    if solution_cache is not None or time_limit is not None:
        raise NotImplementedError("acx.value_guided_greedy_search supports solution_cache=None and time_limit=None only")
    mlp = architecture == "mlp"
    if use_length_priority:
        scorer, kw = _total_length, {}
    else:
        if model is None:
            raise ValueError("a model is needed unless use_length_priority=True")
        if mlp and (feat_mean is None or feat_std is None):
            raise ValueError("architecture='mlp' needs feat_mean and feat_std")

        def scorer(x):
            return torch.expm1(model(x).squeeze(-1))

        kw = dict(scorer_input="features", feat_mean=feat_mean, feat_std=feat_std) if mlp else dict(scorer_input="tokens")
    p = np.asarray(presentation)
    res, st = value_guided_greedy_search_many(p.reshape(1, -1).astype(np.int32), scorer,
                                              max_nodes_to_explore=int(max_nodes_to_explore),
                                              cyclically_reduce_after_moves=cyclically_reduce_after_moves,
                                              device=device, on_error="raise", return_stats=True, **kw)
    solved, path = res[0]
    return solved, path, {"nodes_explored": int(st["nodes"][0]), "min_length": int(st["min_length"][0])}
