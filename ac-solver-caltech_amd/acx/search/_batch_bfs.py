"""bfs over a batch of presentations in one launch (csrc/acx_mbfs.hip, C-ABI acx_mbfs_* in
include/acx.h): one workgroup runs one search from root to verdict, so many small searches fill
the GPU that a loop of acx.bfs leaves idle.  Each result equals the reference's
bfs(p_i, budget_i) (ac_solver/search/breadth_first.py:15-97), paths included."""

from __future__ import annotations

import numpy as np
import torch

from .. import _lib

_HANDLES = {}  # (device, L, cyclical) -> (handle, searches, max_nodes_each)
MAX_NODES_EACH = 1 << 24

# default workspace_bytes: this fraction of the device memory free at the call.  Half leaves the
# caller's own tensors and the allocator's cached blocks alone; a batch that needs more is split
# into consecutive groups, one launch each.
WORKSPACE_FRACTION = 0.5


class _Engine:
    """One batched search of the library: the C functions `prefix`_bytes / _create / _paths /
    _destroy (and _run, or the beam search's step calls), its cached handles, and which searches
    return a path.  `extra` names the shape arguments its _bytes and _create take after
    max_nodes_each (beam: max_width); a cached handle whose extras are at least the wanted ones is
    reused if `reuse(cached extras, wanted extras)` also agrees.  _batch_greedy.py,
    _batch_beam.py and _batch_vgreedy.py run their searches through the same code."""

    def __init__(self, name, prefix, handles, path_statuses, no_path, extra=(), reuse=None):
        self.name, self.prefix, self.handles = name, prefix, handles
        self.path_statuses, self.no_path = path_statuses, no_path
        self.extra, self.reuse = extra, reuse

    def fn(self, lib, what):
        return getattr(lib, f"{self.prefix}_{what}")


_BFS = _Engine("bfs_many", "acx_mbfs", _HANDLES, (_lib.BFS_FOUND,), (False, None))


def _device(device) -> torch.device:
    dev = torch.device(device if device is not None else "cuda")
    return dev if dev.index is not None else torch.device("cuda", torch.cuda.current_device())


def _handle(eng, lib, dev: torch.device, L: int, cyclical: bool, n: int, max_nodes: int, extra=()):
    key = (dev.index, L, bool(cyclical))
    h = eng.handles.get(key)
    if (h is not None and h[1] >= n and h[2] >= max_nodes and all(a >= b for a, b in zip(h[3:], extra))
            and (eng.reuse is None or eng.reuse(h[3:], extra))):
        return h[0]
    if h is not None:
        eng.fn(lib, "destroy")(h[0])
        del eng.handles[key]
    with torch.cuda.device(dev):
        ptr = eng.fn(lib, "create")(L, n, max_nodes, *extra, int(bool(cyclical)))
    if not ptr:
        shape = "".join(f", {k}={v}" for k, v in zip(eng.extra, extra))
        raise _lib.ACXError(f"{eng.prefix}_create(L={L}, n_searches={n}, max_nodes_each={max_nodes}{shape}) failed "
                            "(device memory?)")
    eng.handles[key] = (ptr, n, max_nodes, *extra)
    return ptr


def _group_size(eng, lib, dev, L, cyclical, N, max_nodes, workspace_bytes, extra=()):
    """how many of N searches run at once: what fits workspace_bytes (None: WORKSPACE_FRACTION of
    the free device memory), at least one"""
    per = int(eng.fn(lib, "bytes")(L, max_nodes, *extra))
    if workspace_bytes is None:
        workspace_bytes = int(WORKSPACE_FRACTION * torch.cuda.mem_get_info(dev)[0])
        have = eng.handles.get((dev.index, L, bool(cyclical)))
        if have is not None:  # a cached workspace is not free memory, but it is ours to use
            workspace_bytes = max(workspace_bytes, have[1] * int(eng.fn(lib, "bytes")(L, *have[2:])))
    return max(1, min(N, int(workspace_bytes) // per))


def _release(eng) -> None:
    if not eng.handles:
        return
    lib = _lib.load()
    for h in eng.handles.values():
        eng.fn(lib, "destroy")(h[0])
    eng.handles.clear()


def release_workspaces() -> None:
    """Free the cached batch workspaces (the batched greedy, beam, value-guided greedy and MCTS searches' too)."""
    _release(_BFS)
    from . import _batch_beam, _batch_greedy, _batch_mcts, _batch_vgreedy
    _batch_greedy.release_workspaces()
    _batch_beam.release_workspaces()
    _batch_vgreedy.release_workspaces()
    _batch_mcts.release_workspaces()


def _validate(presentations, max_nodes_to_explore, on_error, name="bfs_many"):
    """(states (N, 2L) int32, budgets (N) int64) or ValueError; no GPU call (a tensor on a GPU is
    copied to the host to be checked)."""
    if on_error not in ("raise", "return"):
        raise ValueError(f"on_error must be 'raise' or 'return', not {on_error!r}")
    if isinstance(presentations, torch.Tensor):
        presentations = presentations.detach().cpu().numpy()
    try:
        p = np.asarray(presentations)
    except ValueError as e:  # rows of different lengths
        raise ValueError("presentations must be rows of equal length") from e
    if p.dtype == object or p.ndim != 2:
        raise ValueError("presentations must be rows of equal length")
    if not np.issubdtype(p.dtype, np.integer):
        raise ValueError("presentations must hold integer letters")
    N, W = p.shape
    if W == 0 or W % 2:
        raise ValueError(f"a presentation has an even, positive number of entries, not {W}")
    L = W // 2
    if L > _lib.MAX_L:
        raise ValueError(f"max_relator_length {L} exceeds {_lib.MAX_L}")
    for h in (p[:, :L], p[:, L:]):
        nz = h != 0
        n = nz.sum(1)
        bad = (n == 0) | (nz != (np.arange(L)[None, :] < n[:, None])).any(1)
        if bad.any():
            i = int(np.nonzero(bad)[0][0])
            raise ValueError(f"{p[i]} is not a valid presentation (row {i})")
    if np.any(np.abs(p) > 2):
        raise ValueError("acx presentations use letters +-1 (x) and +-2 (y) only")
    if np.ndim(max_nodes_to_explore) == 0:
        b = np.full(N, int(max_nodes_to_explore), np.int64)
    else:
        b = np.asarray(max_nodes_to_explore)
        if b.ndim != 1 or len(b) != N or not np.issubdtype(b.dtype, np.integer):
            raise ValueError(f"max_nodes_to_explore must be an integer or a sequence of {N} integers")
        b = b.astype(np.int64)
    b = np.maximum(b, 1)  # the reference still expands the root once
    if N and int(b.max()) > MAX_NODES_EACH:
        raise ValueError(f"{name} supports at most 2^24 nodes per search")
    return np.ascontiguousarray(p, dtype=np.int32), b


def bfs_many(presentations, max_nodes_to_explore=10000, cyclically_reduce_after_moves=False, device=None,
             on_error="raise", return_stats=False, workspace_bytes=None):
    """bfs of every row of `presentations` ((N, 2L) array, tensor or list of equal-length rows),
    all in one launch: a list of (True, path) | (False, None), entry i equal to the reference's
    bfs(presentations[i], budget_i, cyclically_reduce_after_moves=...).  Prints nothing.

    max_nodes_to_explore: one budget, or one per row.
    on_error: a search in which a move raises in the reference (a relator becomes empty) makes the
      call raise AssertionError naming the rows ("raise"), or puts None at their positions ("return").
    return_stats: also return a dict of (N) arrays -- status (ACX_BFS_* of include/acx.h), nodes
      (len(tree_nodes) at the end: the number in the reference's "Exiting search" line), parents
      expanded, min_length.
    workspace_bytes: the most device memory the searches' workspace may take (default: half of the
      free device memory); a larger batch runs as consecutive groups, one launch per group."""
    return _search_many(_BFS, presentations, max_nodes_to_explore, cyclically_reduce_after_moves, device, on_error,
                        return_stats, workspace_bytes)


def _search_many(eng, presentations, max_nodes_to_explore, cyclically_reduce_after_moves, device, on_error,
                 return_stats, workspace_bytes):
    states, budgets = _validate(presentations, max_nodes_to_explore, on_error, eng.name)
    N, L = states.shape[0], states.shape[1] // 2
    stats = dict(status=np.zeros(N, np.int32), nodes=np.zeros(N, np.int64), parents=np.zeros(N, np.int64),
                 min_length=np.zeros(N, np.int32))
    results = [eng.no_path] * N
    if N:
        dev, lib, cyc = _device(device), _lib.load(), bool(cyclically_reduce_after_moves)
        cap = int(budgets.max())
        group = _group_size(eng, lib, dev, L, cyc, N, cap, workspace_bytes)
        for g0 in range(0, N, group):
            g1 = min(N, g0 + group)
            _run_group(eng, lib, dev, L, cyc, states[g0:g1], budgets[g0:g1], group, cap, g0, stats, results)
    return _finish(eng, results, stats, on_error, return_stats)


def _finish(eng, results, stats, on_error, return_stats):
    """the searches in which a move raised, and the call's return value"""
    errs = np.nonzero(stats["status"] == _lib.BFS_MOVE_ERROR)[0]
    if len(errs):
        if on_error == "raise":
            raise AssertionError(f"{eng.name}: a move produced an invalid presentation (utils.py:264-266) in searches "
                                 f"{errs.tolist()}")
        for i in errs:
            results[int(i)] = None
    return (results, stats) if return_stats else results


def _check_status(what, status, g0=0):
    bad = np.nonzero(status < 0)[0]
    if len(bad):  # validated arguments cannot get here: a full table or a kernel fault
        raise _lib.ACXError(f"{what}: searches {(bad + g0).tolist()} ended with status {status[bad].tolist()}")


def _read_results(eng, lib, h, dev, stream, g0, status, plen, results):
    """status and path_len (device tensors) of the group's finished searches: the paths are read
    back and results[g0 + i] is set for every search whose status returns one -> status on the host"""
    n = len(status)
    offsets = torch.cumsum(plen, 0) - plen
    plen_h = plen.cpu().numpy()  # (waits for the searches)
    total = int(plen_h.sum())
    acts = torch.empty(max(total, 1), dtype=torch.int32, device=dev)
    tots = torch.empty(max(total, 1), dtype=torch.int32, device=dev)
    if total:
        _lib.check(eng.fn(lib, "paths")(h, n, offsets.data_ptr(), acts.data_ptr(), tots.data_ptr(), total, stream),
                   f"{eng.prefix}_paths")
    status_h = status.cpu().numpy()
    acts_h, tots_h = acts.cpu().tolist(), tots.cpu().tolist()
    off = 0
    for i in range(n):
        k = int(plen_h[i])
        if status_h[i] in eng.path_statuses:
            results[g0 + i] = (bool(status_h[i] == _lib.BFS_FOUND), list(zip(acts_h[off:off + k], tots_h[off:off + k])))
        off += k
    return status_h


def _run_group(eng, lib, dev, L, cyclical, states, budgets, n_cap, cap, g0, stats, results):
    n = len(states)
    h = _handle(eng, lib, dev, L, cyclical, n_cap, cap)
    stream = torch.cuda.current_stream(dev).cuda_stream
    with torch.cuda.device(dev):
        st = torch.from_numpy(states).to(dev)
        bd = torch.from_numpy(budgets).to(dev)
        status = torch.empty(n, dtype=torch.int32, device=dev)
        min_len = torch.empty(n, dtype=torch.int32, device=dev)
        nodes, parents, plen = (torch.empty(n, dtype=torch.int64, device=dev) for _ in range(3))
        _lib.check(eng.fn(lib, "run")(h, st.data_ptr(), bd.data_ptr(), n, status.data_ptr(), nodes.data_ptr(),
                                      parents.data_ptr(), min_len.data_ptr(), plen.data_ptr(), stream),
                   f"{eng.prefix}_run")
        status_h = _read_results(eng, lib, h, dev, stream, g0, status, plen, results)
        stats["status"][g0:g0 + n] = status_h
        stats["nodes"][g0:g0 + n] = nodes.cpu().numpy()
        stats["parents"][g0:g0 + n] = parents.cpu().numpy()
        stats["min_length"][g0:g0 + n] = min_len.cpu().numpy()
    _check_status(f"{eng.prefix}_run", status_h, g0)
