"""The process that runs a job of tests/test_gpu_weak_hash.py, tests/test_weak_hash_cpu.py,
tests/test_gpu_cache.py or tests/test_gpu_fused_vgreedy.py through libacx_weakhash.so (ac-solver-caltech_amd/build.py; the key hash of csrc/acx_test_hash.h with 8
classes): the variant cannot share a process with libacx.so, so each job gets a fresh one.

    ACX_LIB=<variant> python tests/weak_hash_child.py <dir>

<dir>/in.json holds {"calls": [...]}: every call is one API call (the `op`s below) with the
arguments its test chose; nothing here knows an expected value.  The answers go to one JSON line on
stdout ({"results": [...]}, answer i for call i) and the arrays a call returns (node keys) to
<dir>/out.npz under "a<i>_<name>".  A call that returns node keys also reports their count and the
number of distinct acx_internal_key_hash values over them."""
import contextlib
import ctypes
import io
import json
import os
import queue
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
for _p in (HERE, REPO, os.path.join(REPO, "ac-solver-caltech_amd")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import numpy as np  # noqa: E402

CLASSES = 8


def _path(p):
    return None if p is None else [list(x) for x in p]


def key_hashes(lib, keys, L):
    keys = np.ascontiguousarray(keys, dtype=np.uint64)
    return np.array([lib.acx_internal_key_hash(keys[i].ctypes.data, L) for i in range(len(keys))], np.uint64)


def _classes(lib, keys, L):
    return {"nodes": int(len(keys)), "classes": int(len(np.unique(key_hashes(lib, keys, L))))}


def _quiet(fn):
    """fn() -> its value or "raises" (a move of the reference raised); the lines it prints swallowed"""
    with contextlib.redirect_stdout(io.StringIO()):
        try:
            return fn()
        except AssertionError:
            return "raises"


class Ops:
    def __init__(self, lib, arrays):
        import torch
        self.lib, self.arrays, self.dev = lib, arrays, torch.device("cuda:0")

    # ---- CPU ----
    def hashes(self, i, c):
        """key hashes of (n, kw) keys read from c["keys"] (an .npy file)"""
        self.arrays[f"a{i}_hashes"] = key_hashes(self.lib, np.load(c["keys"]), c["L"])
        return {}

    def owners(self, i, c):
        st = np.ascontiguousarray(np.load(c["states"]), dtype=np.int32)
        self.arrays[f"a{i}_owners"] = np.array(
            [[self.lib.acx_sbfs_owner(st[j].ctypes.data, c["L"], w) for w in c["worlds"]] for j in range(len(st))], np.int32)
        return {}

    def symbols(self, i, c):
        from acx import _lib
        return {"missing": [n for n in _lib.SIGNATURES if not hasattr(self.lib, n)]}

    # ---- GPU: one answer per call ----
    def device_bfs(self, i, c):
        from acx.search import _device_bfs as D
        r = _quiet(lambda: D.device_bfs(np.array(c["pres"]), c["budget"], cyclically_reduce_after_moves=c["cyc"],
                                        device=self.dev, chunk=c["chunk"], keep_node_keys=c.get("keys", False)))
        if r == "raises":
            return {"raises": True}
        st = D.LAST_STATS
        out = {"ok": bool(r[0]), "path": _path(r[1]), "status": st["status"], "nodes": st["nodes"],
               "parents": st["parents"], "min_length": st["min_length"]}
        if c.get("keys"):
            nk = np.asarray(st["node_keys"])[:st["nodes"]]
            self.arrays[f"a{i}_keys"] = nk
            out.update(_classes(self.lib, nk, len(c["pres"]) // 2))
        return out

    def greedy_device(self, i, c):
        from acx.search import _engine as E
        r = _quiet(lambda: E.run_search(E.GREEDY, np.array(c["pres"]), c["budget"], False, c["cyc"], device=self.dev,
                                        keep_node_keys=c.get("keys", False), engine="device"))
        if r == "raises":
            return {"raises": True}
        st = E.LAST_STATS
        out = {"ok": bool(r[0]), "path": _path(r[1]), "status": st["status"], "nodes": st["nodes"],
               "min_length": st["min_length"]}
        if c.get("keys"):
            self.arrays[f"a{i}_keys"] = st["node_keys"]
            out.update(_classes(self.lib, st["node_keys"], len(c["pres"]) // 2))
        return out

    def _many(self, fn, c):
        res, st = fn(np.array(c["pres"], np.int32), c["budgets"], cyclically_reduce_after_moves=c["cyc"], device=self.dev,
                     return_stats=True, on_error="return")
        return {"res": [None if r is None else [bool(r[0]), _path(r[1])] for r in res],
                "st": {k: v.tolist() for k, v in st.items()}}

    def bfs_many(self, i, c):
        import acx
        return self._many(acx.bfs_many, c)

    def greedy_many(self, i, c):
        import acx
        return self._many(acx.greedy_search_many, c)

    def _scored_many(self, fn, c, nodes_of, **kw):
        """a scored search's results and stats, and over each search's nodes (the yardstick's:
        nodes_of(presentation, its index), packed on the CPU) their count and the number of
        distinct key hashes"""
        from weak_hash_common import pack_keys_np
        pres = np.array(c["pres"], np.int32)
        L = pres.shape[1] // 2
        res, st = fn(pres, cyclically_reduce_after_moves=c["cyc"], device=self.dev, return_stats=True, on_error="return",
                     **kw)
        out = {"res": [None if r is None else [bool(r[0]), _path(r[1])] for r in res],
               "st": {k: v.tolist() for k, v in st.items()}, "nodes": [], "classes": []}
        for j, p in enumerate(pres):
            states = np.stack(nodes_of(p, j)["states"])
            out["nodes"].append(int(len(states)))
            out["classes"].append(_classes(self.lib, pack_keys_np(states, L), L)["classes"])
        return out

    def beam_many(self, i, c):
        import acx
        import beam_yardstick as Y
        return self._scored_many(acx.beam_search_many, c, lambda p, j: Y.beam(p, c["scorer"], c["W"], c["budget"], c["cyc"]),
                                 scorer=Y.SCORERS[c["scorer"]][1], beam_width=c["W"], max_nodes_to_explore=c["budget"])

    def vgreedy_many(self, i, c):
        import acx
        import vgreedy_yardstick as Y
        return self._scored_many(acx.value_guided_greedy_search_many, c,
                                 lambda p, j: Y.vgreedy(p, c["scorer"], c["budgets"][j], c["cyc"], drop_twins=True),
                                 scorer=Y.SCORERS[c["scorer"]][1], max_nodes_to_explore=c["budgets"])

    def vgreedy_mlp_many(self, i, c):
        """acx.value_guided_greedy_search_many scored by the acx.DeviceMLP mlp_common.net(kind, hidden)
        with its normalisation, fused or stepped; the nodes whose key hashes are counted are the
        yardstick's, scored by mlp.host"""
        import acx
        import mlp_common as MC
        import vgreedy_yardstick as Y
        mlp, mean, std = MC.net(c["kind"], tuple(c["hidden"]))
        return self._scored_many(acx.value_guided_greedy_search_many, c,
                                 lambda p, j: Y.vgreedy(p, mlp.host, c["budgets"][j], c["cyc"], mean=mean, std=std,
                                                        drop_twins=True),
                                 scorer=mlp, max_nodes_to_explore=c["budgets"], feat_mean=mean, feat_std=std,
                                 fused=c["fused"])

    def mcts_many(self, i, c):
        """scorer: a name of mcts_yardstick.MODELS or TOKEN_MODELS, taken as the value itself"""
        import acx
        import mcts_yardstick as Y
        tokens = c["scorer"] in Y.TOKEN_MODELS
        return self._scored_many(acx.mcts_search_many, c,
                                 lambda p, j: Y.mcts(p, Y.model_np(c["scorer"]), c["budgets"][j], c["c"], c["cyc"],
                                                     on_tokens=tokens),
                                 scorer=Y.model_t(c["scorer"]), scorer_input="tokens" if tokens else "features",
                                 max_nodes_to_explore=c["budgets"], c_explore=c["c"])

    def cache(self, i, c):
        """the solution cache: {"L", "presentations", "paths", "queries", "searches", "budget"} -> the
        classes of the variant's hash, the cache's dict after a backfill in two calls from a capacity
        of 64 (as lists), the paths_for of every query, and the value-guided greedy searches with the
        cache attached"""
        import acx
        k = acx.SolutionCache(c["L"], self.dev, capacity=64)
        paths = [[tuple(m) for m in p] for p in c["paths"]]
        half = len(paths) // 2
        k.backfill_many(np.array(c["presentations"][:half]), paths[:half])
        k.backfill_many(np.array(c["presentations"][half:]), paths[half:])
        d = k.to_dict()
        found = k.paths_for(np.array(c["queries"]))
        res, st = acx.value_guided_greedy_search_many(np.array(c["searches"]), lambda f: f[:, 0], c["budget"],
                                                      device=self.dev, solution_cache=k, return_stats=True)
        return dict(classes=int(self.lib.acx_internal_hash_classes()), entries=len(k), capacity=k.capacity,
                    keys=[list(x) for x in d], values=[[list(m) for m in v] for v in d.values()],
                    found=[None if p is None else [list(m) for m in p] for p in found],
                    results=[[bool(ok), [list(m) for m in p]] for ok, p in res],
                    nodes=st["nodes"].tolist(), cache_hit=st["cache_hit"].tolist())

    def sbfs(self, i, c):
        """arena_log2_cap: on a fresh workspace whose key arena starts at 2^cap records (the
        regrowth hook of csrc/acx_sbfs.hip), which is reset whatever happens"""
        from acx.search import _sharded_bfs as S
        hook = self.lib.acx_internal_sbfs_arena_cap
        hook.argtypes, hook.restype = [ctypes.c_int32], None
        if c.get("arena_log2_cap"):
            S.release_workspaces()
            hook(c["arena_log2_cap"])
        try:
            r = _quiet(lambda: S.sharded_bfs(np.array(c["pres"]), c["budget"], cyclically_reduce_after_moves=c["cyc"],
                                             device=self.dev, chunk=c["chunk"], keep_node_keys=c.get("keys", False)))
        finally:
            if c.get("arena_log2_cap"):
                hook(0)
                S.release_workspaces()
        if r == "raises":
            return {"raises": True}
        st = S.LAST_STATS
        out = {"ok": bool(r[0]), "path": _path(r[1]), "status": st["status"], "nodes": st["nodes"],
               "parents": st["parents"], "chunks": st["chunks"], "min_length": st["min_length"]}
        if c.get("keys"):
            self.arrays[f"a{i}_keys"], self.arrays[f"a{i}_ids"] = st["node_keys"], st["node_ids"]
            out.update(_classes(self.lib, st["node_keys"][:st["nodes"]], len(c["pres"]) // 2))
        return out

    def release(self, i, c):
        from acx.search import _device_bfs as D
        from acx.search import _sharded_bfs as S
        D.release_workspaces()
        S.release_workspaces()
        return {}

    def sbfs_ranks(self, i, c):
        """test_gpu_sbfs.py's workers (gloo, sharing cuda:0), started from this process, which makes
        no GPU call of its own; they inherit ACX_LIB"""
        import torch.multiprocessing as mp
        from test_gpu_sbfs import _free_port, _worker
        world = c["world"]
        ctx = mp.get_context("spawn")
        q = ctx.Queue()
        port = _free_port()
        ps = [ctx.Process(target=_worker, args=(r, world, port, c["jobs"], q)) for r in range(world)]
        for p in ps:
            p.start()
        try:
            res = dict(q.get(timeout=c["timeout"]) for _ in range(world))
            for p in ps:
                p.join(timeout=60)
            died = [p.exitcode for p in ps if p.exitcode is None or p.exitcode < 0 or p.exitcode in (134, 139)]
        except queue.Empty:
            died = ["timeout"]
        if died:  # a rank that hung or ended on a signal: this process ends as one that did
            for p in ps:
                p.kill()
            print(f"sbfs_ranks: workers died: {died}", file=sys.stderr)
            sys.exit(124 if died == ["timeout"] else 139)
        out = {"exit": [p.exitcode for p in ps], "error": [res[r] if isinstance(res[r], str) else None for r in range(world)],
               "cases": [], "orders": {}}
        if any(out["error"]):
            return out
        for r in range(world):
            out["cases"].append([x if x == "raises" else [x[0], x[1], x[2]] for x in res[r]["cases"]])
        for name, (pres, _, _, _) in c["jobs"]["orders"].items():
            out["orders"][name] = []
            for r in range(world):
                rr, nodes, ids, keys, trace = res[r][name]
                self.arrays[f"a{i}_{name}_{r}_ids"], self.arrays[f"a{i}_{name}_{r}_keys"] = ids, keys
                out["orders"][name].append({"ok": bool(rr[0]), "path": _path(rr[1]), "nodes": int(nodes), "trace": [int(v) for v in trace],
                                            **{"store_" + k: v for k, v in _classes(self.lib, keys, len(pres) // 2).items()}})
        return out


def main():
    d = sys.argv[1]
    with open(os.path.join(d, "in.json")) as f:
        calls = json.load(f)["calls"]
    from acx import _lib
    lib = _lib.load()
    assert lib.acx_internal_hash_classes() == CLASSES, (_lib.LIB_PATH, lib.acx_internal_hash_classes())
    arrays = {}
    ops = Ops(lib, arrays)
    results = [getattr(ops, c["op"])(i, c) for i, c in enumerate(calls)]
    np.savez(os.path.join(d, "out.npz"), **arrays)
    print(json.dumps({"results": results}))


if __name__ == "__main__":
    main()
