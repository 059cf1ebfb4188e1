"""What the batched searches scored by the caller share (_batch_beam.py, _batch_vgreedy.py, _batch_mcts.py; the
step frame of csrc/acx_scored.h): the checks of the scorer's arguments, the scorer call, the body
of their reference-signature wrappers of one search, and the loop of steps -- make the candidates,
read their count (the step's one host synchronisation), gather them, score them, hand the scores
back."""

from __future__ import annotations

import numpy as np
import torch

from .. import _lib, ops
from . import _batch_bfs, _cache

_TIMING = None  # tools/bench_search_many.py: an object whose mark(phase) is called after each phase of a step


class _Steps:
    """How an engine steps: its _Engine, the names of its two step calls (`make` the candidates,
    `take` their scores: beam expand / select, vgreedy pop / push, mcts select / backup), `report`: what the two numbers
    make wrote mean, as (M rows to score, live searches), the loop's bound -- the steps beyond the
    largest budget, or a function of the largest budget -- with its reason, and the stats it
    returns besides status.  `make_args(dev, step, margs)`: the engine's own arguments of its make
    call at step `step`, before the output pair (mcts: the log table and the constant), from what
    its entry passed to _run as `margs`.  Every engine has acx_*_set_cache / _cache_hits
    (csrc/acx_cache.h) and its searches take a solution cache."""

    def __init__(self, eng, make, take, report, bound, stats, make_args=None):
        self.eng, self.make, self.take, self.report, self.stats = eng, make, take, report, stats
        self.bound = bound if callable(bound) else (lambda cap: cap + bound)
        self.make_args = make_args


def _validate_scorer(presentations, scorer, max_nodes_to_explore, scorer_input, on_error, name):
    """the first checks of every search scored by the caller: (states, budgets) or ValueError; no
    GPU call."""
    states, budgets = _batch_bfs._validate(presentations, max_nodes_to_explore, on_error, name)
    if not callable(scorer):
        raise ValueError("scorer must be callable")
    if scorer_input not in ("features", "tokens"):
        raise ValueError(f"scorer_input must be 'features' or 'tokens', not {scorer_input!r}")
    return states, budgets


def _validate_norm(scorer_input, feat_mean, feat_std):
    """their last checks: (mean, std) as float32 arrays or (None, None), or ValueError"""
    if (feat_mean is None) != (feat_std is None):
        raise ValueError("pass both feat_mean and feat_std, or neither")
    mean = std = None
    if feat_mean is not None:
        if scorer_input != "features":
            raise ValueError("feat_mean / feat_std go with scorer_input='features'")
        mean, std = (np.ascontiguousarray(torch.as_tensor(x).detach().cpu().numpy(), dtype=np.float32)
                     for x in (feat_mean, feat_std))
        if mean.shape != (14,) or std.shape != (14,):
            raise ValueError("feat_mean and feat_std hold 14 values each")
    return mean, std


def _scores(scorer, x, M):
    with torch.no_grad():
        y = scorer(x)
    if not isinstance(y, torch.Tensor) or y.device != x.device:
        raise ValueError("the scorer must return a tensor on its input's device")
    if y.shape not in ((M,), (M, 1)):
        raise ValueError(f"the scorer must return ({M},) or ({M}, 1) values, not {tuple(y.shape)}")
    return y.reshape(M).to(torch.float32).contiguous()


def _model_scorer(model):
    """the scorer of the single-search wrappers: _score_states_mlp / _score_states_seq of the reference"""
    return lambda x: torch.expm1(model(x).squeeze(-1))


def _single(name, many, presentation, model, architecture, feat_mean, feat_std, solution_cache, time_limit, ints,
            no_model=None, scorer=None, **kw):
    """A reference-signature wrapper `name` around its batch call `many`: one row, on_error="raise"
    -> (solved, path, {stat: its int}).  `solution_cache`: an acx.SolutionCache goes to `many`; the reference's
    dict is refused here (NotImplementedError: upload it once with SolutionCache.from_dict -- the
    batch calls take a dict), anything else is a ValueError.  `no_model`: the message when `model` is None (None: not
    checked), `scorer`: one to use on the raw features in place of the model's (`model` and
    `architecture` are then not looked at), `ints`: the keywords of `many` the reference takes as ints."""
    if time_limit is not None:
        raise NotImplementedError(f"acx.{name} supports time_limit=None only")
    if solution_cache is not None:
        if isinstance(solution_cache, dict):
            raise NotImplementedError(f"acx.{name} takes an acx.SolutionCache, not the reference's dict: upload it "
                                      "once with acx.SolutionCache.from_dict(d, L, device)")
        _cache.check(solution_cache, np.asarray(presentation).size // 2)
        kw["solution_cache"] = solution_cache
    if scorer is None:
        if no_model is not None and model is None:
            raise ValueError(no_model)
        if architecture != "mlp":
            kw["scorer_input"] = "tokens"
        elif feat_mean is None or feat_std is None:
            raise ValueError("architecture='mlp' needs feat_mean and feat_std")
        else:
            kw.update(scorer_input="features", feat_mean=feat_mean, feat_std=feat_std)
        scorer = _model_scorer(model)
    p = np.asarray(presentation)
    res, st = many(p.reshape(1, -1).astype(np.int32), scorer, on_error="raise", return_stats=True,
                   **{k: int(v) for k, v in ints.items()}, **kw)
    return (*res[0], {k: int(v[0]) for k, v in st.items()})


def _run(sc, states, budgets, own, extra, scorer, scorer_input, mean, std, cyclical, device, workspace_bytes, on_error,
         return_stats, margs=None, solution_cache=None, fused=None):
    """the validated searches, in groups that fit the workspace -> the call's return value.  `own`:
    the engine's per-search arrays for its begin call (beam: the widths), `extra`: its handle's
    shape arguments, `margs`: what its _Steps.make_args needs, `solution_cache`: what the caller
    passed, already through _cache.check.  `fused`: None, or (pops per launch,): `scorer` is an
    acx.DeviceMLP and the engine's run_mlp call (vgreedy) steps the searches on the device, many
    pops per launch, in place of the loop of steps."""
    eng = sc.eng
    N, L = states.shape[0], states.shape[1] // 2
    stats = {k: np.zeros(N, t) for k, t in (("status", np.int32), *sc.stats)}
    if solution_cache is not None:
        stats["cache_hit"] = np.zeros(N, bool)
    results = [eng.no_path] * N
    if N:
        dev, lib, cyc = _batch_bfs._device(device), _lib.load(), bool(cyclical)
        cache, ours = _cache.resolve(solution_cache, L, dev)
        try:
            cap = int(budgets.max())
            group = _batch_bfs._group_size(eng, lib, dev, L, cyc, N, cap, workspace_bytes, extra)
            for g0 in range(0, N, group):
                g1 = min(N, g0 + group)
                _run_group(sc, lib, dev, L, cyc, states[g0:g1], budgets[g0:g1], [x[g0:g1] for x in own], group, cap,
                           extra, scorer, scorer_input, mean, std, g0, stats, results, margs, cache, fused)
        finally:
            if ours:
                cache.close()
    nan = np.nonzero(stats["status"] == _lib.BEAM_NAN)[0]
    if len(nan):
        raise ValueError(f"{eng.name}: the scorer returned NaN in searches {nan.tolist()}")
    _batch_bfs._check_status(eng.prefix, stats["status"])
    return _batch_bfs._finish(eng, results, stats, on_error, return_stats)


def _run_group(sc, lib, dev, L, cyc, states, budgets, own, n_cap, cap, extra, scorer, scorer_input, mean, std, g0,
               stats, results, margs=None, cache=None, fused=None):
    eng = sc.eng
    n, kw = len(states), _lib.key_words(L)
    h = _batch_bfs._handle(eng, lib, dev, L, cyc, n_cap, cap, extra)
    # a reused handle keeps its attachment: set it, or clear it, for this run
    _lib.check(eng.fn(lib, "set_cache")(h, cache.attach_to(dev) if cache is not None else None),
               f"{eng.prefix}_set_cache")
    try:
        stream = torch.cuda.current_stream(dev).cuda_stream
        call = lambda what, *args: _lib.check(eng.fn(lib, what)(h, *args, stream), f"{eng.prefix}_{what}")  # noqa: E731
        with torch.cuda.device(dev):
            st = torch.from_numpy(states).to(dev)
            bd = torch.from_numpy(budgets).to(dev)
            own_d = [torch.from_numpy(x).to(dev) for x in own]
            mean_d, std_d = (None if x is None else torch.from_numpy(x).to(dev) for x in (mean, std))
            out = torch.zeros(2, dtype=torch.int64, device=dev)
            call("begin", st.data_ptr(), bd.data_ptr(), *(x.data_ptr() for x in own_d), n)
            mark = (lambda phase: None) if _TIMING is None else _TIMING.mark
            if fused is not None:
                _fused_loop(sc, call, scorer, dev, mean_d, std_d, fused[0], cap, out, mark)
            else:
                for step in range(sc.bound(cap)):
                    mark("between")
                    call(sc.make, *(sc.make_args(dev, step, margs) if sc.make_args else ()), out.data_ptr())
                    mark(sc.make)
                    M, live = sc.report(*out.tolist())  # the step's one host synchronisation
                    if live == 0:
                        break
                    if M == 0:  # nothing to score
                        continue
                    keys = torch.empty((M, kw), dtype=torch.int64, device=dev)
                    call("gather", keys.data_ptr(), M)
                    if scorer_input == "features":
                        x = ops.features(keys=keys, L=L, mean=mean_d, std=std_d)
                    else:
                        x = ops.token_ids(keys=keys, L=L)
                    mark("gather_features")
                    y = _scores(scorer, x, M)
                    mark("scorer")
                    call(sc.take, y.data_ptr(), M)
                    mark(sc.take)
                else:
                    raise _lib.ACXError(f"{eng.prefix}: the searches did not end within their budgets")
            status = torch.empty(n, dtype=torch.int32, device=dev)
            min_len = torch.empty(n, dtype=torch.int32, device=dev)
            nodes, steps, plen = (torch.empty(n, dtype=torch.int64, device=dev) for _ in range(3))
            call("finish", status.data_ptr(), nodes.data_ptr(), steps.data_ptr(), min_len.data_ptr(), plen.data_ptr())
            stats["status"][g0:g0 + n] = _batch_bfs._read_results(eng, lib, h, dev, stream, g0, status, plen, results)
            for k, v in (("nodes", nodes), ("steps", steps), ("iterations", steps), ("min_length", min_len)):
                if k in stats:
                    stats[k][g0:g0 + n] = v.cpu().numpy()
            if cache is not None:
                _cache_hits(eng, lib, h, dev, stream, cache, g0, n, stats, results)
    finally:  # the handle outlives the call and the cache may not: it never keeps a pointer to it
        if cache is not None:
            eng.fn(lib, "set_cache")(h, None)


def _fused_loop(sc, call, mlp, dev, mean_d, std_d, pops_per_launch, cap, out, mark):
    """launches of up to pops_per_launch pops of every live search until none is live: one host read
    per launch.  The engine's step bound, in pops, bounds the launches."""
    params = mlp.params_on(dev)
    for _ in range(-(-sc.bound(cap) // pops_per_launch)):
        call("run_mlp", params.data_ptr(), mlp.dims, mlp.n_layers, ops._ptr(mean_d), ops._ptr(std_d),
             pops_per_launch, out.data_ptr())
        _, live = out.tolist()  # (pops of this launch, live searches): the launch's host synchronisation
        mark("run_mlp")
        if live == 0:
            return
    raise _lib.ACXError(f"{sc.eng.prefix}: the searches did not end within their budgets")


def _cache_hits(eng, lib, h, dev, stream, cache, g0, n, stats, results):
    """the searches of a group that ended on a cache hit: (True, the path to the state that hit + the
    rotation moves + the cached path) (value_guided_search.py:375-377, mcts.py:276-277)"""
    hit = np.nonzero(stats["status"][g0:g0 + n] == _lib.BFS_CACHED)[0]
    if not len(hit):
        return
    entry = torch.empty(n, dtype=torch.int64, device=dev)
    rel, k = (torch.empty(n, dtype=torch.int32, device=dev) for _ in range(2))
    _lib.check(eng.fn(lib, "cache_hits")(h, n, entry.data_ptr(), rel.data_ptr(), k.data_ptr(), stream),
               f"{eng.prefix}_cache_hits")
    entry, rel, k = (x.cpu().numpy()[hit] for x in (entry, rel, k))
    for i, tail in zip(hit.tolist(), cache.tails(entry, rel, k)):
        results[g0 + i] = (True, list(results[g0 + i][1]) + tail)
        stats["cache_hit"][g0 + i] = True
