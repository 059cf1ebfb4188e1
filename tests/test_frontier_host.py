"""CPU: the host code both greedy engines share (ac-solver-caltech_amd/csrc/acx_key.h and
acx_frontier.h), built stand-alone with the host compiler (tests/frontier_check.cpp; no libacx, no
GPU): the packed-key fields at the word-boundary relator lengths, the priority key's fast path
against its generic path and the definition (greedy.py:55-64,104-113), the BucketHeap's pop order
with first-word ties, the two-generation in-flight table at age 4, and the per-child replay of a
popped node (what it records at a success, a move error and the budget)."""
import os
import subprocess

import pytest

from conftest import PKG_ROOT, REPO


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("frontier") / "frontier_check")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-I", os.path.join(REPO, "include"), "-I",
                           os.path.join(PKG_ROOT, "csrc"), os.path.join(REPO, "tests", "frontier_check.cpp"), "-o", exe])
    return exe


@pytest.mark.parametrize("seed", [1, 2])
def test_frontier_host_code(checker, seed):
    r = subprocess.run([checker, str(seed)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.startswith("ok"), r.stdout[-2000:]
