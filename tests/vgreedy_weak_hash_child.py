"""The process that runs tests/test_gpu_vgreedy_many.py's call through libacx_weakhash.so
(ac-solver-caltech_amd/build.py; the key hash of csrc/acx_test_hash.h with 8 classes): the variant
cannot share a process with libacx.so.

    ACX_LIB=<variant> python tests/vgreedy_weak_hash_child.py <dir>

<dir>/in.json holds {"pres", "scorer", "budgets", "cyc"}: one acx.value_guided_greedy_search_many call.
Nothing here knows an expected value.  The answer is one JSON line on stdout: the call's results and
stats and, per search, the number of its nodes (the yardstick's, packed on the CPU) and of distinct
acx_internal_key_hash values over them."""
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


def main():
    with open(os.path.join(sys.argv[1], "in.json")) as f:
        c = json.load(f)
    import torch
    import acx
    import vgreedy_yardstick as Y
    from acx import _lib
    from weak_hash_child import key_hashes
    from weak_hash_common import pack_keys_np
    lib = _lib.load()
    assert lib.acx_internal_hash_classes() == CLASSES, (_lib.LIB_PATH, lib.acx_internal_hash_classes())
    pres = np.array(c["pres"], np.int32)
    L = pres.shape[1] // 2
    res, st = acx.value_guided_greedy_search_many(pres, Y.SCORERS[c["scorer"]][1], max_nodes_to_explore=c["budgets"],
                                                  cyclically_reduce_after_moves=c["cyc"], device=torch.device("cuda:0"),
                                                  return_stats=True, on_error="return")
    out = {"res": [None if r is None else [bool(r[0]), [list(x) for x in r[1]]] for r in res],
           "st": {k: v.tolist() for k, v in st.items()}, "nodes": [], "classes": []}
    for p, b in zip(pres, c["budgets"]):
        states = np.stack(Y.vgreedy(p, c["scorer"], b, c["cyc"], drop_twins=True)["states"])
        out["nodes"].append(int(len(states)))
        out["classes"].append(int(len(np.unique(key_hashes(lib, pack_keys_np(states, L), L)))))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
