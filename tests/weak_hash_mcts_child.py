"""The process that runs the MCTS job of tests/test_gpu_weak_hash_mcts.py through libacx_weakhash.so
(ac-solver-caltech_amd/build.py; the key hash of csrc/acx_test_hash.h with 8 classes), beside
tests/weak_hash_child.py and with its conventions: the variant cannot share a process with
libacx.so, so the job gets a fresh one.

    ACX_LIB=<variant> python tests/weak_hash_mcts_child.py <dir>

<dir>/in.json holds {"calls": [...]}: every call is one acx.mcts_search_many call -- {pres, scorer (a
name of mcts_yardstick.MODELS or TOKEN_MODELS, taken as the value itself), budgets, c, cyc} --
with the arguments its test chose; nothing here knows an expected value.  The answers go to one JSON
line on stdout ({"results": [...]}): res, st, and per search the number of its final nodes (the
yardstick's, packed on the CPU) and of distinct acx_internal_key_hash values over them."""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
for _p in (HERE, REPO, os.path.join(REPO, "ac-solver-caltech_amd")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import numpy as np  # noqa: E402

CLASSES = 8


def mcts_many(lib, c):
    import torch

    import acx
    import mcts_yardstick as Y
    from weak_hash_child import key_hashes
    from weak_hash_common import pack_keys_np
    pres = np.array(c["pres"], np.int32)
    L = pres.shape[1] // 2
    tokens = c["scorer"] in Y.TOKEN_MODELS
    res, st = acx.mcts_search_many(pres, Y.model_t(c["scorer"]), max_nodes_to_explore=c["budgets"], c_explore=c["c"],
                                   cyclically_reduce_after_moves=c["cyc"],
                                   scorer_input="tokens" if tokens else "features", device=torch.device("cuda:0"),
                                   return_stats=True, on_error="return")
    out = {"res": [None if r is None else [bool(r[0]), [list(x) for x in r[1]]] for r in res],
           "st": {k: v.tolist() for k, v in st.items()}, "nodes": [], "classes": []}
    for j, p in enumerate(pres):
        y = Y.mcts(p, Y.model_np(c["scorer"]), c["budgets"][j], c["c"], c["cyc"], on_tokens=tokens)
        keys = pack_keys_np(np.stack(y["states"]), L)
        out["nodes"].append(int(len(keys)))
        out["classes"].append(int(len(np.unique(key_hashes(lib, keys, L)))))
    return out


def main():
    d = sys.argv[1]
    with open(os.path.join(d, "in.json")) as f:
        calls = json.load(f)["calls"]
    from acx import _lib
    lib = _lib.load()
    assert lib.acx_internal_hash_classes() == CLASSES, (_lib.LIB_PATH, lib.acx_internal_hash_classes())
    print(json.dumps({"results": [mcts_many(lib, c) for c in calls]}))


if __name__ == "__main__":
    main()
