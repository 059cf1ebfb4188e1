"""acx -- MI355X-native Andrews-Curtis environment (the ACEnv.step / 12-way expansion hot
path of Avi161/AC-Solver-Caltech), HIP kernels behind the C-ABI in include/acx.h.

Public names mirror the reference's ac_solver/__init__.py:1-6 (ACEnv, ACEnvConfig, bfs,
greedy_search); VecACEnv and acx.ops are the batched device API, bfs_many and greedy_search_many
are bfs and greedy_search over a batch of presentations in one launch, beam_search_many and
beam_search the reference's value-guided beam search (value_search/value_guided_search.py) over a
batch, scored by the caller's model, value_guided_greedy_search_many and value_guided_greedy_search
its value-guided greedy search, mcts_search_many and mcts_search its MCTS (value_search/mcts.py),
likewise; DeviceMLP is the reference's FeatureMLP as device code, which the value-guided greedy
search runs fused, with no Python between the pops.
"""

from .envs.ac_env import ACEnv, ACEnvConfig, VecACEnv
from .envs.ac_moves import ACMove
from .search.breadth_first import bfs
from .search._batch_bfs import bfs_many
from .search.greedy import greedy_search
from .search._batch_greedy import greedy_search_many
from .search._batch_beam import beam_search, beam_search_many
from .search._batch_vgreedy import value_guided_greedy_search, value_guided_greedy_search_many
from .search._batch_mcts import mcts_search, mcts_search_many
from .search._cache import SolutionCache
from ._mlp import DeviceMLP
from . import data  # noqa: F401

__all__ = ["ACEnv", "ACEnvConfig", "VecACEnv", "ACMove", "bfs", "bfs_many", "greedy_search",
           "greedy_search_many", "beam_search", "beam_search_many", "value_guided_greedy_search",
           "value_guided_greedy_search_many", "mcts_search", "mcts_search_many", "SolutionCache", "DeviceMLP"]
