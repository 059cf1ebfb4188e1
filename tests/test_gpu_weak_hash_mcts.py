"""The batched MCTS's visited set under a colliding hash (csrc/acx_mcts.hip through
libacx_weakhash.so; tests/test_gpu_weak_hash.py states what the variant library does to a table):
every probe starts in the table's last bucket and wraps, a search's nodes form one chain, and the
full key compare decides between states that share a fingerprint.  The searches must not change:
the expected values are the yardstick's (tests/mcts_yardstick.py), never the variant's.

The variant cannot share a process with libacx.so: the calls go to one fresh child
(tests/weak_hash_mcts_child.py) with one time limit."""
import json
import os
import subprocess
import sys
import time

import numpy as np
import pytest

import mcts_yardstick as Y
import vgreedy_yardstick as YV
from conftest import REPO
from many_common import _dataset_rows
from weak_hash_common import FATAL, check_classes, variant

pytestmark = pytest.mark.gpu

CHILD = os.path.join(REPO, "tests", "weak_hash_mcts_child.py")
AK3 = [1, 1, 1, -2, -2, -2, -2] + [0] * 11 + [1, 2, 1, -2, -1, -2] + [0] * 12


def _run_child(calls, workdir, timeout):
    with open(os.path.join(str(workdir), "in.json"), "w") as f:
        json.dump({"calls": calls}, f)
    t0 = time.perf_counter()
    r = subprocess.run([sys.executable, CHILD, str(workdir)], env=dict(os.environ, ACX_LIB=variant()),
                       capture_output=True, text=True, timeout=timeout)
    assert r.returncode >= 0 and r.returncode not in FATAL, (r.returncode, r.stderr[-2000:])
    assert r.returncode == 0, (r.returncode, r.stderr[-4000:])
    out = json.loads(r.stdout.strip().splitlines()[-1])["results"]
    assert len(out) == len(calls)
    return out, time.perf_counter() - t0


def test_mcts_many(tmp_path):
    """AK(3), an expansion with twins and Miller-Schupp rows at L = 18, at most 2,000 nodes per
    search, on features at c = 1.41 and on token ids at c = 0: the results are the yardstick's, and
    every large search's nodes fall in at most 8 hash classes"""
    twin = next(p for p, _, _, _ in YV.twin_cases() if len(p) == 36)
    rows = [np.array(AK3, np.int32), twin] + list(_dataset_rows()[::40])
    budgets = [1989, 600] + [1200] * (len(rows) - 2)
    calls = [dict(pres=[r.tolist() for r in rows], scorer=s, budgets=budgets, c=c, cyc=cyc)
             for s, c, cyc in (("M1", 1.41, False), ("TOK", 0.0, False))]
    out, dt = _run_child(calls, tmp_path, 240)
    print(f"weak-hash job mcts_many: {len(calls)} calls in {dt:.1f} s")
    large = 0
    for call, got in zip(calls, out):
        tokens = call["scorer"] in Y.TOKEN_MODELS
        ys = [Y.mcts(p, Y.model_np(call["scorer"]), b, call["c"], call["cyc"], on_tokens=tokens)
              for p, b in zip(rows, budgets)]
        assert got["res"] == [None if y["raises"] else [y["ok"], y["path"]] for y in ys], call["scorer"]
        for k in ("status", "nodes", "iterations"):
            assert got["st"][k] == [y[k] for y in ys], (call["scorer"], k)
        assert got["nodes"] == [len(y["states"]) for y in ys] and max(got["nodes"]) <= 2000
        assert any(y["twin_expansions"] for y in ys) and sum(y["ucb_sel"] for y in ys) >= 1000
        for n, c in zip(got["nodes"], got["classes"]):
            if n >= 512:
                check_classes(n, c, ("mcts_many", call["scorer"]))
                large += 1
    assert large >= 12
