"""CPU: the chunk verdict the BFS engines share (ac-solver-caltech_amd/csrc/acx_bfs_verdict.h), built
stand-alone with the host compiler (tests/verdict_check.cpp; no libacx, no GPU) and compared, over
every first-success seq, first-raising seq and cut parent of chunks of 1, 2 and 3 parents, with a
child-by-child restatement of the reference's loop (breadth_first.py:84-95).  The program prints
that restatement's table; the sharded BFS's Python copy of the rule (_sharded_bfs._chunk_verdict)
is held to it on every row."""
import os
import subprocess

import pytest

from conftest import PKG_ROOT, REPO


@pytest.fixture(scope="module")
def table(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("verdict") / "verdict_check")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(REPO, "include"), "-I",
                           os.path.join(PKG_ROOT, "csrc"), os.path.join(REPO, "tests", "verdict_check.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    lines = r.stdout.splitlines()
    assert r.returncode == 0 and lines and lines[-1].startswith("ok"), r.stdout[-2000:]
    rows = [tuple(int(x) for x in ln.split()) for ln in lines[:-1]]
    assert len(rows) == int(lines[-1].split()[1])
    return rows


def test_header_matches_the_sequential_reference(table):
    # every case of the enumeration: sum over P of (12 P + 1)^2 (P + 1)
    assert len(table) == sum((12 * P + 1) ** 2 * (P + 1) for P in (1, 2, 3))
    assert len(set(r[:4] for r in table)) == len(table)
    assert {r[4] for r in table} == {0, 1, 2, 3}  # go on, FOUND, BUDGET, MOVE_ERROR all occur


def test_sharded_bfs_python_rule_matches_the_table(table):
    from acx import _lib
    from acx.search._sharded_bfs import NONE, _chunk_verdict

    assert (_lib.BFS_FOUND, _lib.BFS_BUDGET, _lib.BFS_MOVE_ERROR) == (1, 2, 3)
    none = lambda v: NONE if v < 0 else v
    bad = [(r, got) for r in table
           for got in [_chunk_verdict(none(r[1]), none(r[2]), none(r[3]), r[0])] if tuple(got) != r[4:]]
    assert not bad, bad[:10]
