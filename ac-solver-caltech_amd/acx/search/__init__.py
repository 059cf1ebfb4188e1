from ._batch_beam import beam_search, beam_search_many
from ._batch_bfs import bfs_many
from ._batch_greedy import greedy_search_many
from ._batch_mcts import mcts_search, mcts_search_many
from ._cache import SolutionCache
from ._batch_vgreedy import value_guided_greedy_search, value_guided_greedy_search_many
from .breadth_first import bfs
from .greedy import greedy_search

__all__ = ["bfs", "bfs_many", "greedy_search", "greedy_search_many", "beam_search", "beam_search_many",
           "value_guided_greedy_search", "value_guided_greedy_search_many", "mcts_search", "mcts_search_many",
           "SolutionCache"]
