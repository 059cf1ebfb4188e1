"""The hash seam of the search engines (csrc/acx_test_hash.h) and the variant library built with
it (build.py: libacx_weakhash.so, 8 hash classes), on the CPU:

* which library is which (acx_internal_hash_classes, the build stamp, every entry point resolves);
* the weak hash restated from its definition, weak(h) = (h % K) << 61 | 2^61 - 1, through
  acx_internal_key_hash: at most 8 values, every masked or range-reduced probe starts in the last
  bucket, the sbfs owners still spread -- what tests/test_gpu_weak_hash.py relies on for its
  claim that every insert there walks one chain from the table's last bucket;
* the host engine (csrc/acx_search.cpp) compiled with K = 1 and K = 8 behind
  tests/sanitize/search_harness.cpp, plain and under ASan + UBSan, on the 240 reference runs of
  tests/golden/kat_search_extra.json (breadth_first.py:15-97, greedy.py:15-121) at 1, 3 and 16
  threads: the results may depend on the keys alone."""
import importlib.util
import json
import os
import subprocess

import numpy as np
import pytest

from conftest import GOLDEN, PKG_ROOT, REPO
from oracle import oracle as O
from weak_hash_common import CLASSES, VARIANT, pack_keys_np, run_child, variant

CSRC = os.path.join(PKG_ROOT, "csrc")
WORLDS = [2, 3, 4]
BUDGETS = [1, 300, 2000]


def _ak3(L):
    from acx.envs.utils import convert_relators_to_presentation
    return convert_relators_to_presentation([1, 1, 1, -2, -2, -2, -2], [1, 2, 1, -2, -1, -2], L)


def _bfs_levels(start, levels):
    """the distinct states of the first `levels` BFS levels below `start` (oracle expansions)"""
    L = len(start) // 2
    seen = {np.asarray(start, np.int32).tobytes(): None}
    level = [np.asarray(start, np.int32)]
    for _ in range(levels):
        ch, _, err = O.expand12(np.stack(level), L, False)
        level = []
        for c, e in zip(ch.reshape(-1, 2 * L), err.reshape(-1)):
            if not e and c.tobytes() not in seen:
                seen[c.tobytes()] = None
                level.append(c.astype(np.int32))
    return np.stack([np.frombuffer(b, np.int32) for b in seen])


@pytest.fixture(scope="module")
def state_sets():
    """{name: (L, distinct (n, 2L) int32 states)}"""
    sets = {}
    with np.load(os.path.join(GOLDEN, "features.npz")) as z:
        for L in (7, 18, 36):
            sets[f"features_L{L}"] = (L, np.unique(z[f"L{L}_states"].astype(np.int32), axis=0))
    sets["ak3_128"] = (128, _bfs_levels(_ak3(128), 3))
    assert all(len(s) >= 1000 for _, s in sets.values())
    return sets


@pytest.fixture(scope="module")
def weak(state_sets, tmp_path_factory):
    """the variant's answers, from one child process: (symbols missing, {name: hashes}, {name: owners})"""
    d = tmp_path_factory.mktemp("weak_hash")
    calls = [{"op": "symbols"}]
    for name, (L, st) in state_sets.items():
        np.save(d / f"{name}_keys.npy", pack_keys_np(st, L))
        np.save(d / f"{name}_states.npy", st)
        calls.append({"op": "hashes", "keys": str(d / f"{name}_keys.npy"), "L": L})
        calls.append({"op": "owners", "states": str(d / f"{name}_states.npy"), "L": L, "worlds": WORLDS})
    out, arrays, _ = run_child(calls, d, timeout=120)
    names = list(state_sets)
    return (out[0]["missing"], {n: arrays[f"a{1 + 2 * i}_hashes"] for i, n in enumerate(names)},
            {n: arrays[f"a{2 + 2 * i}_owners"] for i, n in enumerate(names)})


def _build_module():
    spec = importlib.util.spec_from_file_location("acx_build", os.path.join(PKG_ROOT, "build.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_which_library_is_which(weak):
    from acx import _lib
    assert _lib.load().acx_internal_hash_classes() == 0  # the shipped hash is untouched
    assert weak[0] == []  # (the child has asserted 8 classes) every SIGNATURES name resolves
    build = _build_module()
    assert build.WEAK_OUT == variant() and build.WEAK_CLASSES == CLASSES
    with open(VARIANT + ".stamp") as f:
        assert f.read().strip() == build.source_hash()
    assert build.built_hash(VARIANT) == build.source_hash()


def test_key_packer_is_the_engines(state_sets):
    from acx.search import _engine as E
    for L, st in state_sets.values():
        keys = pack_keys_np(st[:50], L)
        for s, k in zip(st[:50], keys):
            assert np.array_equal(E._pack_key(s.astype(np.int64), L), k)


def test_shipped_hash_separates_the_keys(state_sets):
    from acx import _lib
    lib = _lib.load()
    for name, (L, st) in state_sets.items():
        keys = pack_keys_np(st, L)
        h = {lib.acx_internal_key_hash(k.ctypes.data, L) for k in keys}
        assert len(h) == len(keys), name
    assert lib.acx_internal_key_hash(None, 36) == 0 and lib.acx_internal_key_hash(keys[0].ctypes.data, 129) == 0


def test_weak_hash_is_its_definition(state_sets, weak):
    _, hashes, owners = weak
    low = (1 << 61) - 1
    # bucket counts of the batched engines at these budgets (csrc/acx_mbfs.hip, acx_mgreedy.hip
    # buckets_for: 2 (B + 11 + 768) and 2 (B + 11 + 12) slots in buckets of 8), and every small one
    nbs = {(2 * (B + 11 + 768) + 7) // 8 for B in BUDGETS} | {(2 * (B + 11 + 12) + 7) // 8 for B in BUDGETS}
    nbs |= set(range(1, 300))
    for name, (L, st) in state_sets.items():
        h = [int(x) for x in hashes[name]]
        assert len(h) == len(st)
        values = set(h)
        assert 2 <= len(values) <= CLASSES, name
        for v in values:
            assert v & low == low and (v >> 61) < CLASSES, (name, hex(v))
            for k in range(41):  # a masked table of 2^k buckets: the last one
                m = (1 << k) - 1
                assert v & m == m
            for nb in nbs:  # a range-reduced table of nb buckets (__umulhi((uint32_t)h, nb)): the last one
                assert ((v & 0xffffffff) * nb) >> 32 == nb - 1, (name, nb)
            assert (v >> 32) & 0xffffff == 0xffffff  # sbfs's fingerprint: one value
        assert len({(v >> 40) & 0xffffff for v in values}) == len(values)  # visited's: one per class
        for j, world in enumerate(WORLDS):  # owner = (h >> 32) * world >> 32 (acx_sbfs_owner)
            assert [int(o) for o in owners[name][:, j]] == [((v >> 32) * world) >> 32 for v in h], (name, world)
            assert set(owners[name][:, j].tolist()) == set(range(world)), (name, world)


# ---------------------------------------------------------------------------------------------
# the host engine under K = 1 and K = 8
# ---------------------------------------------------------------------------------------------
@pytest.fixture(scope="module", params=[(1, "plain"), (8, "plain"), (1, "asan"), (8, "asan")],
                ids=lambda p: f"K{p[0]}-{p[1]}")
def weak_harness(request, tmp_path_factory):
    from test_sanitizers import SAN_FLAGS
    K, kind = request.param
    exe = str(tmp_path_factory.mktemp(f"weak_search_K{K}_{kind}") / "search_harness")
    cmd = (["g++", "-O1", "-g", "-std=c++17", "-pthread", f"-DACX_TEST_HASH_CLASSES={K}"] +
           (SAN_FLAGS["asan"] if kind == "asan" else []) +
           ["-I" + os.path.join(REPO, "include"), os.path.join(REPO, "tests", "sanitize", "search_harness.cpp"),
            os.path.join(CSRC, "acx_search.cpp"), "-x", "c", os.path.join(REPO, "oracle", "acx_oracle.c"), "-o", exe])
    subprocess.run(cmd, check=True, capture_output=True, text=True)
    return exe


@pytest.mark.slow
@pytest.mark.parametrize("threads", ["1", "3", "16"])
def test_host_engine_gives_the_reference_runs_under_a_colliding_hash(weak_harness, threads):
    from test_sanitizers import _run
    with open(os.path.join(GOLDEN, "kat_search_extra.json")) as f:
        cases = json.load(f)
    assert len(cases) == 240
    lines = []
    for c in cases:
        p = c["presentation"]
        mode = 0 if c["search_fn"] == "bfs" else 1
        lines.append(f"{mode} {len(p) // 2} {int(c['cyclical'])} {c['budget']} " + " ".join(map(str, p)))
    out = _run(weak_harness, stdin="\n".join(lines) + "\n", threads=threads).strip().split("\n")
    assert len(out) == len(cases)
    for c, line in zip(cases, out):  # as test_sanitizers.py checks the sanitized engine's runs
        v = [int(x) for x in line.split()]
        status, n_nodes, m = v[0], v[1], v[2]
        path = [(v[3 + 2 * i], v[4 + 2 * i]) for i in range(m)]
        if c["raises"]:
            assert status == 3, c
            continue
        assert status in (1, 2), c
        assert (status == 1) == c["ok"], c
        if c["search_fn"] == "bfs":
            assert (path if status == 1 else None) == (None if c["path"] is None else [tuple(x) for x in c["path"]]), c
        else:
            assert path == [tuple(x) for x in c["path"]], c
        if c["budget_nodes"] is not None:
            assert n_nodes == c["budget_nodes"], c
