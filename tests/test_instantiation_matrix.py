"""CPU: the pieces of tests/test_gpu_instantiations.py that can be wrong without a GPU noticing.

The comparison of a kernel's walk with the oracle's (assert_walk_equal) must raise on every kind of
single corruption, and the list of relator lengths (MATRIX_L) must still cover every instantiation
class that the sources' dispatch defines: someone who adds a class or moves a threshold gets a
failing test, not a silent hole."""
import os
import re

import numpy as np
import pytest

from conftest import PKG_ROOT, REPO
from test_gpu_instantiations import (B_MATRIX, H_MATRIX, MATRIX_L, T_ROLLOUT, T_STEP, assert_not_vacuous,
                                     assert_walk_equal, matrix_case, oracle_walk)

WALK_KEYS = ("state", "reward", "done", "trunc", "count", "err", "err_count", "final_obs", "lengths")


def _walk(L, cyc):
    starts, count0, acts = matrix_case(L, cyc, T_STEP)
    return oracle_walk(starts, count0, acts, L, H_MATRIX, cyc)


@pytest.mark.parametrize("L", [16, 33])
def test_walk_comparison_raises_on_each_corruption(L):
    want = _walk(L, 1)
    assert_not_vacuous(want, L)
    clean = {k: want[k].copy() for k in WALK_KEYS}
    assert_walk_equal(clean, want, L)  # the oracle's own output passes
    n = want["lengths"]
    # a (step, row) that holds a relator r0 of exactly L letters, and one that reset
    t_full, b_full = (int(x[0]) for x in np.nonzero(n[:, :, 0] == L))
    t_rs, b_rs = (int(x[0]) for x in np.nonzero(want["done"] | want["trunc"]))
    t_keep, b_keep = (int(x[0]) for x in np.nonzero((want["done"] | want["trunc"]) == 0))

    def corrupt(key, index, value=None):
        bad = {k: v.copy() for k, v in clean.items()}
        old = bad[key][index]
        bad[key][index] = (-old if key == "state" else old + 1) if value is None else value
        assert not np.array_equal(bad[key], clean[key])
        return bad

    cases = {
        "last letter of a full-length relator": corrupt("state", (t_full, b_full, L - 1)),
        "length": corrupt("lengths", (T_STEP - 1, B_MATRIX - 1, 1)),
        "reward": corrupt("reward", (3, 200)),
        "done": corrupt("done", (t_rs, b_rs), 1 - int(want["done"][t_rs, b_rs])),
        "err byte": corrupt("err", (T_STEP - 1, 64)),
        "final_obs row": corrupt("final_obs", (t_rs, b_rs, 0)),
        "truncated": corrupt("trunc", (0, 4), 1 - int(want["trunc"][0, 4])),
        "step count": corrupt("count", (5, 321)),
        "err_count": corrupt("err_count", (T_STEP - 1,)),
    }
    for name, bad in cases.items():
        with pytest.raises(AssertionError):
            assert_walk_equal(bad, want, L, where=name)
    # final_obs is held to the oracle only on the rows that reset (the kernels leave the others untouched)
    assert_walk_equal(corrupt("final_obs", (t_keep, b_keep, 0)), want, L)
    # a missing output is not compared, a wrongly shaped one raises
    assert_walk_equal({"reward": clean["reward"]}, want, L)
    with pytest.raises(AssertionError):
        assert_walk_equal({"reward": clean["reward"][:-1]}, want, L)


@pytest.mark.slow
@pytest.mark.parametrize("cyc", [1, 0])
def test_matrix_walks_are_not_vacuous(cyc):
    """every (L, cyclical) walk of the GPU module clears its conditions on the oracle's replay"""
    for L in MATRIX_L:
        for T, seed in ((T_STEP, 0), (T_ROLLOUT, 1)):
            starts, count0, acts = matrix_case(L, cyc, T, seed)
            assert_not_vacuous(oracle_walk(starts, count0, acts, L, H_MATRIX, cyc), L)


def _read(*parts):
    with open(os.path.join(*parts)) as f:
        return f.read()


def _nw_classes(src):
    """[(last L of the class, NW), ...] and the NW of every longer L, from nw_for's return line"""
    m = re.search(r"int nw_for\(int L\)\s*\{\s*return\s+([^;]+);", src)
    assert m, "nw_for not found"
    steps = [(int(a), int(b)) for a, b in re.findall(r"L\s*<=\s*(\d+)\s*\?\s*(\d+)", m.group(1))]
    last = re.search(r":\s*(\d+)\s*$", m.group(1).strip())
    assert steps and last, m.group(1)
    return steps, int(last.group(1))


def test_matrix_lengths_cover_every_instantiation_class():
    launch = _read(PKG_ROOT, "csrc", "acx_launch.h")
    steps, nw_rest = _nw_classes(launch)
    assert (steps, nw_rest) == _nw_classes(_read(PKG_ROOT, "csrc", "acx_features.hip"))  # one class table
    max_l = int(re.search(r"#define\s+ACX_MAX_L\s+(\d+)", _read(REPO, "include", "acx.h")).group(1))
    special = sorted(int(x) for x in re.findall(r"if \(L == (\d+)\) return f\.template go<", launch))
    assert special and max_l in special  # the compile-time tiles, suites of their own
    assert not set(special) & set(MATRIX_L)
    # dispatch's switch handles every NW that nw_for returns, the last one as its default
    cases = [int(x) for x in re.findall(r"case (\d+): return v4 \? f\.template go<\1, 0, 4>\(\) : f\.template go<\1, 0, 2>",
                                        launch)]
    assert cases == [nw for _, nw in steps]
    assert re.search(rf"default: return v4 \? f\.template go<{nw_rest}, 0, 4>\(\) : f\.template go<{nw_rest}, 0, 2>", launch)
    assert re.search(r"const bool v4 = \(2 \* L\) % 4 == 0;", launch)  # VEC = 4 for even L, 2 for odd L
    bounds = [t for t, _ in steps]
    assert bounds == sorted(bounds) and bounds[-1] < max_l - 1
    lo = 1
    for hi, nw in steps + [(max_l - 1, nw_rest)]:
        in_class = [x for x in MATRIX_L if lo <= x <= hi]
        assert any(x % 2 == 0 for x in in_class), f"no even L of class NW={nw} ({lo}..{hi}) in MATRIX_L"
        assert any(x % 2 == 1 for x in in_class), f"no odd L of class NW={nw} ({lo}..{hi}) in MATRIX_L"
        assert lo in MATRIX_L, f"first L of class NW={nw} ({lo}) not in MATRIX_L"
        if (hi, nw) in steps:
            assert hi == 16 * nw, (hi, nw)  # a class ends on a full tile of 16 NW letters
            assert hi in MATRIX_L, f"full tile L={hi} of class NW={nw} not in MATRIX_L"
        lo = hi + 1
    assert max_l - 1 in MATRIX_L
