"""Loader for libacx.so, the C-ABI declared in include/acx.h.

The library is loaded with ctypes *after* torch: its NEEDED libamdhip64.so.7 then binds to
the HIP runtime torch has already mapped (same soname), so torch's device pointers and
streams are valid in it.  There is no fallback: if the library (or a GPU) is missing, every
compute call raises.
"""

from __future__ import annotations

import ctypes
import os

import torch  # noqa: F401  (must be imported before libacx.so is loaded)

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("ACX_LIB", os.path.join(HERE, "libacx.so"))

OK, E_ARG, E_LAUNCH = 0, -1, -2
BFS_EXHAUSTED, BFS_FOUND, BFS_BUDGET, BFS_MOVE_ERROR = 0, 1, 2, 3
MBFS_DOMAIN, MBFS_OVERFLOW = -3, -4
ERR_NONE, ERR_INVALID, ERR_EMPTY_CONJ, ERR_DOMAIN, ERR_ACTION, ERR_PAD = 0, 1, 2, 3, 4, 9
MAX_L = 128
# acx_rollout_deal (include/acx.h ACX_DEAL_*, ACX_ROLLOUT_DEAL_WORDS)
DEAL_PLAIN, DEAL_XCC, DEAL_AUTO = 0, 1, 2
DEAL_PCT, DEAL_OVER_PCT, ROLLOUT_DEAL_WORDS = 80, 125, 256

# every entry point declared in include/acx.h, with its ctypes signature
_P = ctypes.c_void_p
_I32 = ctypes.c_int32
_I64 = ctypes.c_int64
SIGNATURES = {
    "acx_step": ([_P] * 12 + [_I64, _I32, _I32, _I32, _P], ctypes.c_int),
    "acx_step_lengths": ([_P] * 11 + [_I64, _I32, _I32, _I32, _P], ctypes.c_int),
    "acx_step_lengths_reduced": ([_P] * 12 + [_I64, _I32, _I32, _I32, _P], ctypes.c_int),
    "acx_step_plan_create": ([_I32] + [_P] * 12 + [_I64, _I32, _I32, _I32], ctypes.c_void_p),
    "acx_step_plan_launch": ([_P, _P, _P], ctypes.c_int),
    "acx_step_plan_destroy": ([_P], None),
    # ..., action_hist, hist_cap, hist_base, hist_t, episode_len, ...
    "acx_step_learner": ([_P] * 11 + [_I32, _P, _I64, _P, _P, _P, _P, _I64, _I32, _I32, _I32, _P], ctypes.c_int),
    "acx_step_record": ([_P] * 11 + [_I32, _P, _I64] + [_P] * 3 + [_I64, _I32, _I32, _I32, _P], ctypes.c_int),
    "acx_step_next": ([_P] * 11 + [_I32, _P, _I64] + [_P] * 3 + [_I64, _I32, _I32, _I32, _P], ctypes.c_int),
    "acx_curriculum_workspace": ([_I64], ctypes.c_int64),
    "acx_learner_failure_word": ([_I64], ctypes.c_int64),
    "acx_curriculum_assign": ([_P, _P, _P, _I64] + [_P] * 7 + [_I64, _I32, _P], ctypes.c_int),
    "acx_learner_step": ([_P] * 11 + [_I32, _P, _I64] + [_P] * 4 + [_I64] + [_P] * 4 + [_I64, _I32, _I32, _I32, _P],
                         ctypes.c_int),
    "acx_rollout": ([_P] * 10 + [_I32, _I64, _I32, _I32, _I32, _P], ctypes.c_int),
    "acx_packed_actions_words": ([_I32, _I64], ctypes.c_int64),
    "acx_pack_actions": ([_P, _P, _I32, _I64, _P], ctypes.c_int),
    "acx_rollout_packed": ([_P] * 10 + [_I32, _I64, _I32, _I32, _I32, _P], ctypes.c_int),
    "acx_rollout_obs8": ([_P] * 11 + [_I32, _I64, _I32, _I32, _I32, _P], ctypes.c_int),
    # ..., T, B, L, horizon, cyclical, deal, pct, over_pct, deal_ws, stream
    "acx_rollout_deal": ([_P] * 12 + [_I32, _I64, _I32, _I32, _I32, _I32, _I32, _I32, _P, _P], ctypes.c_int),
    "acx_rollout_deal_info": ([_I32, _I64, _I32, _I32, _I32, _I32, _I32, _P], ctypes.c_int),
    "acx_expand12": ([_P] * 6 + [_I64, _I32, _I32, _P], ctypes.c_int),
    "acx_canonicalize": ([_P] * 5 + [_I64, _I32, _I32, _P], ctypes.c_int),
    "acx_unpack_keys": ([_P] * 3 + [_I64, _I32, _P], ctypes.c_int),
    # exact word functions on arbitrary letters (ac-solver-caltech_amd/csrc/acx_words.hip)
    "acx_word_move": ([_P] * 7 + [_I64, _I32, _I32, _P], ctypes.c_int),
    "acx_concatenate": ([_P] * 4 + [_I64, _I32, _I32, _I32, _I32, _P], ctypes.c_int),
    "acx_conjugate": ([_P] * 6 + [_I64, _I32, _I32, _I32, _I32, _P], ctypes.c_int),
    "acx_word_simplify_presentation": ([_P] * 5 + [_I64, _I32, _I32, _P], ctypes.c_int),
    "acx_word_simplify_relator": ([_P, _I32] + [_P] * 5 + [_I64, _I32, _I32, _I32, _P], ctypes.c_int),
    "acx_key_words": ([_I32], ctypes.c_int32),
    "acx_version": ([], ctypes.c_char_p),
    "acx_features": ([_P] * 5 + [_I64, _I32, _P], ctypes.c_int),
    "acx_token_ids": ([_P] * 3 + [_I64, _I32, _I32, _P], ctypes.c_int),
    # the FeatureMLP scorer (csrc/acx_mlp.hip, acx_mlp_host.cpp) and the fused pops of acx_vgreedy.hip
    "acx_mlp_scores": ([_P, _P, _P, _I32, _P, _I64, _P], ctypes.c_int),
    "acx_mlp_scores_host": ([_P, _P, _P, _I32, _P, _I64], ctypes.c_int),
    "acx_vgreedy_run_mlp": ([_P, _P, _P, _I32, _P, _P, _I64, _P, _P], ctypes.c_int),
    # host-side search engine (ac-solver-caltech_amd/csrc/acx_search.cpp)
    "acx_search_create": ([_I32, _I32, _P, _I64], ctypes.c_void_p),
    "acx_search_destroy": ([_P], None),
    "acx_search_next_batch": ([_P, _P, _I64], ctypes.c_int64),
    "acx_search_feed": ([_P, _P, _I64], ctypes.c_int32),
    "acx_search_status": ([_P, _P, _P, _P], ctypes.c_int32),
    "acx_search_path": ([_P, _P, _P, _I64], ctypes.c_int64),
    "acx_search_node_keys": ([_P, _P, _I64], ctypes.c_int64),
    "acx_search_stats": ([_P, _P], None),
    "acx_search_min_trace": ([_P, _P, _I64], ctypes.c_int64),
    "acx_search_popped": ([_P, _P, _I64], ctypes.c_int64),
    "acx_search_found": ([_P, _P, _P], ctypes.c_int32),
    # greedy with the device visited set (ac-solver-caltech_amd/csrc/acx_greedy.hip)
    "acx_greedy_run": ([_P, _I32, _I64, _I32, _I32, _P], ctypes.c_int),
    "acx_greedy_destroy": ([_P], None),
    "acx_greedy_status": ([_P, _P, _P, _P], ctypes.c_int32),
    "acx_greedy_path": ([_P, _P, _P, _I64], ctypes.c_int64),
    "acx_greedy_stats": ([_P, _P], None),
    "acx_greedy_min_trace": ([_P, _P, _I64], ctypes.c_int64),
    "acx_greedy_popped": ([_P, _P, _I64], ctypes.c_int64),
    "acx_greedy_node_keys": ([_P, _P, _I64], ctypes.c_int64),
    "acx_greedy_found": ([_P, _P, _P], ctypes.c_int32),
    # device BFS (ac-solver-caltech_amd/csrc/acx_bfs.hip)
    "acx_bfs_create": ([_I32, _I64, _I64, _I32], ctypes.c_void_p),
    "acx_bfs_run": ([_P, _P, _I64, _P, _P, _I64, _P, _P], ctypes.c_int),
    "acx_bfs_destroy": ([_P], None),
    "acx_bfs_node_keys": ([_P, _P, _I64, _P], ctypes.c_int64),
    "acx_bfs_min_trace": ([_P, _P, _I64], ctypes.c_int64),
    # owner-partitioned multi-GPU BFS (ac-solver-caltech_amd/csrc/acx_sbfs.hip)
    "acx_sbfs_create": ([_I32, _I64, _I64, _I32, _I32, _I32], ctypes.c_void_p),
    "acx_sbfs_destroy": ([_P], None),
    "acx_sbfs_max_records": ([_P], ctypes.c_int64),
    "acx_sbfs_owner": ([_P, _I32, _I32], ctypes.c_int32),
    "acx_sbfs_reset": ([_P, _P, _P], ctypes.c_int),
    "acx_sbfs_expand": ([_P, _I64, _I32, _P, _I32, _P], ctypes.c_int),
    "acx_sbfs_pack": ([_P, _P, _P], ctypes.c_int),
    "acx_sbfs_insert": ([_P, _P, _I64, _I64, _P, _P], ctypes.c_int),
    "acx_sbfs_commit": ([_P, _P, _I64, _I64, _P, _P], ctypes.c_int),
    "acx_sbfs_min_len": ([_P, _I64, _P], ctypes.c_int64),
    "acx_sbfs_lookup": ([_P, _I64, _P, _P], ctypes.c_int),
    "acx_sbfs_trace": ([_P, _I64, _I64, _P, _I64, _P], ctypes.c_int64),
    "acx_sbfs_node_keys": ([_P, _P, _P, _I64, _P], ctypes.c_int64),
    # the solution cache (ac-solver-caltech_amd/csrc/acx_cache.hip)
    "acx_cache_bytes": ([_I32, _I64], ctypes.c_int64),
    "acx_cache_create": ([_I32, _I64], ctypes.c_void_p),
    "acx_cache_destroy": ([_P], None),
    "acx_cache_info": ([_P, _P, _P], ctypes.c_int),
    "acx_cache_count": ([_P, _P, _P, _P, _I64, _I32, _I32, _I32, _P, _P, _P], ctypes.c_int),
    "acx_cache_reserve": ([_P, _I64, _P], ctypes.c_int),
    "acx_cache_fill": ([_P, _P, _P, _P, _P, _I64, _I64, _I64, _I32, _I32, _I32, _P], ctypes.c_int),
    "acx_cache_lookup": ([_P, _P, _I64, _P, _P, _P, _P], ctypes.c_int),
    "acx_cache_rows": ([_P, _P, _I64, _P, _P, _P], ctypes.c_int),
    "acx_cache_entries": ([_P, _P, _I64, _P, _P], ctypes.c_int),
    # the hash seam of the search engines (csrc/acx_test_hash.h; tests only)
    "acx_internal_hash_classes": ([], ctypes.c_int32),
    "acx_internal_key_hash": ([_P, _I32], ctypes.c_uint64),
    # the MCTS kernels' score routine over arrays (csrc/acx_mcts.hip; tests only)
    "acx_internal_ucb": ([_P, _P, _P, ctypes.c_double, _P, _I64, _P], ctypes.c_int),
}

# the batched engines, one workgroup per search: BFS (ac-solver-caltech_amd/csrc/acx_mbfs.hip) and
# greedy (acx_mgreedy.hip) have the same five functions (the handle of csrc/acx_batch.h)
_BATCH = (("bytes", [_I32, _I64], ctypes.c_int64),
          ("create", [_I32, _I64, _I64, _I32], ctypes.c_void_p),
          ("run", [_P, _P, _P, _I64, _P, _P, _P, _P, _P, _P], ctypes.c_int),
          ("paths", [_P, _I64, _P, _P, _P, _I64, _P], ctypes.c_int),
          ("destroy", [_P], None))
for _prefix in ("acx_mbfs", "acx_mgreedy"):
    for _what, _args, _res in _BATCH:
        SIGNATURES[f"{_prefix}_{_what}"] = (_args, _res)

# the engines scored by the caller (the step frame of csrc/acx_scored.h): a step is the make call,
# gather, the scorer, the take call.  Beam search (acx_beam.hip): expand, select.  Value-guided greedy
# (acx_vgreedy.hip): pop, push; a NaN score ends a search with BEAM_NAN, as in the beam search.
# MCTS (acx_mcts.hip): select (with the host's log table, its length and the UCB1 constant), backup.
# Per engine: its make and take names, and its own arguments of the shape (bytes, create), of
# begin and of the make call
BEAM_NAN, BEAM_MAX_WIDTH = -5, 1024
MCTS_SPIN = 64
_SCORED = (("acx_beam", "expand", "select", [_I32], [_P], []),
           ("acx_vgreedy", "pop", "push", [], [], []),
           ("acx_mcts", "select", "backup", [], [], [_P, _I64, ctypes.c_double]))
for _prefix, _make, _take, _shape, _begin, _own in _SCORED:
    SIGNATURES.update({
        f"{_prefix}_bytes": ([_I32, _I64] + _shape, ctypes.c_int64),
        f"{_prefix}_create": ([_I32, _I64, _I64] + _shape + [_I32], ctypes.c_void_p),
        f"{_prefix}_begin": ([_P, _P, _P] + _begin + [_I64, _P], ctypes.c_int),
        f"{_prefix}_{_make}": ([_P] + _own + [_P, _P], ctypes.c_int),
        f"{_prefix}_gather": ([_P, _P, _I64, _P], ctypes.c_int),
        f"{_prefix}_{_take}": ([_P, _P, _I64, _P], ctypes.c_int),
        f"{_prefix}_finish": ([_P] * 7, ctypes.c_int),
        f"{_prefix}_paths": ([_P, _I64, _P, _P, _P, _I64, _P], ctypes.c_int),
        f"{_prefix}_destroy": ([_P], None),
    })
# an attached solution cache (csrc/acx_cache.h)
BFS_CACHED = 4
for _prefix in ("acx_beam", "acx_vgreedy", "acx_mcts"):
    SIGNATURES[f"{_prefix}_set_cache"] = ([_P, _P], ctypes.c_int)
    SIGNATURES[f"{_prefix}_cache_hits"] = ([_P, _I64, _P, _P, _P, _P], ctypes.c_int)

_lib = None


class ACXError(RuntimeError):
    pass


def load():
    """Return the loaded libacx.so (raises ACXError if it is missing)."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise ACXError(
                f"libacx.so not found at {LIB_PATH}; build it with `python ac-solver-caltech_amd/build.py` "
                "(there is no CPU fallback for the acx kernels)"
            )
        lib = ctypes.CDLL(LIB_PATH)
        for name, (argtypes, restype) in SIGNATURES.items():
            fn = getattr(lib, name)
            fn.argtypes = argtypes
            fn.restype = restype
        _lib = lib
    return _lib


def check(status: int, what: str) -> None:
    if status != OK:
        kind = {E_ARG: "bad argument", E_LAUNCH: "kernel launch failed"}.get(status, f"status {status}")
        raise ACXError(f"{what}: {kind}")


def key_words(L: int) -> int:
    return (4 * L + 16 + 63) // 64
