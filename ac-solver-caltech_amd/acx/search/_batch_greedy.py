"""greedy_search over a batch of presentations in one launch (csrc/acx_mgreedy.hip, C-ABI
acx_mgreedy_* in include/acx.h): one wave runs one search from root to verdict, its frontier a heap
in the search's own slice of device memory, so many small searches fill the GPU that a loop of
acx.greedy_search (one launch and one host round trip per pop round) leaves idle.  Each result
equals the reference's greedy_search(p_i, budget_i) (ac_solver/search/greedy.py:15-121), paths
included.  Arguments, validation and batching are those of bfs_many (_batch_bfs.py)."""

from __future__ import annotations

from .. import _lib
from . import _batch_bfs

_HANDLES = {}  # (device, L, cyclical) -> (handle, searches, max_nodes_each)
# greedy returns a path unless a move raised (greedy.py:100,121)
_GREEDY = _batch_bfs._Engine("greedy_search_many", "acx_mgreedy", _HANDLES,
                             (_lib.BFS_EXHAUSTED, _lib.BFS_FOUND, _lib.BFS_BUDGET), (False, None))


def release_workspaces() -> None:
    """Free the cached batch workspaces of the greedy search."""
    _batch_bfs._release(_GREEDY)


def greedy_search_many(presentations, max_nodes_to_explore=10000, cyclically_reduce_after_moves=False, device=None,
                       on_error="raise", return_stats=False, workspace_bytes=None):
    """greedy_search of every row of `presentations` ((N, 2L) array, tensor or list of equal-length
    rows), all in one launch: a list of (True, path) | (False, path), entry i equal to the
    reference's greedy_search(presentations[i], budget_i, cyclically_reduce_after_moves=...) -- on
    the budget exit or an exhausted frontier the path is the last popped node's plus (11, total of
    its last child), as the reference returns it.  Prints nothing.

    max_nodes_to_explore: one budget, or one per row.
    on_error: a search in which a move raises in the reference (a relator becomes empty) makes the
      call raise AssertionError naming the rows ("raise"), or puts None at their positions ("return").
    return_stats: also return a dict of (N) arrays -- status (ACX_BFS_* of include/acx.h), nodes
      (len(tree_nodes) at the end: the number in the reference's "Exiting search" line), parents
      (nodes popped), min_length.
    workspace_bytes: the most device memory the searches' workspace may take (default: half of the
      free device memory); a larger batch runs as consecutive groups, one launch per group."""
    return _batch_bfs._search_many(_GREEDY, presentations, max_nodes_to_explore, cyclically_reduce_after_moves,
                                   device, on_error, return_stats, workspace_bytes)
