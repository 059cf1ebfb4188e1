"""The process that runs the beam search's job of tests/test_gpu_beam_many.py through
libacx_weakhash.so (ac-solver-caltech_amd/build.py; the key hash of csrc/acx_test_hash.h with 8
classes): the variant cannot share a process with libacx.so, so the job gets a fresh one, started
as tests/weak_hash_common.run_child starts tests/weak_hash_child.py.

    ACX_LIB=<variant> python tests/beam_weak_hash_child.py <dir>

<dir>/in.json holds {pres, scorer, W, budget, cyc}; nothing here knows an expected value.  One JSON
line on stdout: the search's result and stats, and over its nodes (the yardstick's, packed on the
CPU) their count and the number of distinct acx_internal_key_hash values."""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
for _p in (HERE, REPO, os.path.join(REPO, "ac-solver-caltech_amd")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import numpy as np  # noqa: E402


def main():
    with open(os.path.join(sys.argv[1], "in.json")) as f:
        c = json.load(f)
    import torch
    import acx
    from acx import _lib
    import beam_yardstick as Y
    from weak_hash_child import CLASSES, key_hashes
    from weak_hash_common import pack_keys_np
    lib = _lib.load()
    assert lib.acx_internal_hash_classes() == CLASSES, (_lib.LIB_PATH, lib.acx_internal_hash_classes())
    pres = np.array(c["pres"], np.int32)
    L = pres.shape[1] // 2
    res, st = acx.beam_search_many(pres, Y.SCORERS[c["scorer"]][1], beam_width=c["W"], max_nodes_to_explore=c["budget"],
                                   cyclically_reduce_after_moves=c["cyc"], device=torch.device("cuda:0"),
                                   return_stats=True, on_error="return")
    out = {"res": [None if r is None else [bool(r[0]), [list(x) for x in r[1]]] for r in res],
           "st": {k: v.tolist() for k, v in st.items()}, "nodes": [], "classes": []}
    for p in pres:
        states = np.stack(Y.beam(p, c["scorer"], c["W"], c["budget"], c["cyc"])["states"])
        out["nodes"].append(int(len(states)))
        out["classes"].append(int(len(np.unique(key_hashes(lib, pack_keys_np(states, L), L)))))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
