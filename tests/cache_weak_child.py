"""The process that runs the solution cache through libacx_weakhash.so for tests/test_gpu_cache.py
(the variant cannot share a process with libacx.so; tests/weak_hash_child.py is the same idea for the
engines' own jobs):

    ACX_LIB=<variant> python tests/cache_weak_child.py <dir>

<dir>/in.json holds {"L", "presentations", "paths", "queries", "searches", "budget"}; nothing here
knows an expected value.  One JSON line on stdout: the classes of the variant's hash, the cache's
dict after the backfill (as lists), the paths_for of every query, and the value-guided greedy
searches with the cache attached."""
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
    import torch

    import acx
    from acx import _lib
    with open(os.path.join(sys.argv[1], "in.json")) as f:
        job = json.load(f)
    dev = torch.device("cuda:0")
    lib = _lib.load()
    c = acx.SolutionCache(job["L"], dev, capacity=64)
    paths = [[tuple(m) for m in p] for p in job["paths"]]
    half = len(paths) // 2
    c.backfill_many(np.array(job["presentations"][:half]), paths[:half])
    c.backfill_many(np.array(job["presentations"][half:]), paths[half:])
    d = c.to_dict()
    found = c.paths_for(np.array(job["queries"]))
    res, st = acx.value_guided_greedy_search_many(np.array(job["searches"]), lambda f: f[:, 0], job["budget"], device=dev,
                                                  solution_cache=c, return_stats=True)
    print(json.dumps(dict(classes=int(lib.acx_internal_hash_classes()), entries=len(c), capacity=c.capacity,
                          keys=[list(k) for k in d], values=[[list(m) for m in v] for v in d.values()],
                          found=[None if p is None else [list(m) for m in p] for p in found],
                          results=[[bool(ok), [list(m) for m in p]] for ok, p in res],
                          nodes=st["nodes"].tolist(), cache_hit=st["cache_hit"].tolist())))


if __name__ == "__main__":
    main()
