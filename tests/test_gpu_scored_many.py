"""The step frame the two searches scored by the caller share (csrc/acx_scored.h,
acx/search/_scored.py) at the edges of its offsets scan, which takes the per-search candidate counts
1,024 at a time: one search, 1,023 (the last thread of the only chunk idle) and 1,025 (a second
chunk of one search).  The other tests of the two engines run 4,096 searches or a few.  Dataset rows
cycled, budget 20, scorer S0 (beam: W = 2): every search must give what its row gives in a batch of
the 238 distinct rows alone, and the first 8 rows what the yardsticks give."""
import functools

import numpy as np
import pytest

import beam_yardstick as YB
import test_gpu_beam_many as TBM
import test_gpu_vgreedy_many as TVM
import vgreedy_yardstick as YV
from many_common import _dataset_rows

pytestmark = pytest.mark.gpu

BUDGET, W = 20, 2
ENGINES = {
    "beam": (lambda rows: TBM._many(rows, "S0", W, BUDGET), TBM._check_yardstick,
             lambda p: YB.beam(p, "S0", W, BUDGET)),
    "vgreedy": (lambda rows: TVM._many(rows, "S0", BUDGET), TVM._check_yardstick,
                lambda p: YV.vgreedy(p, "S0", BUDGET, False, drop_twins=True)),
}


@functools.lru_cache(maxsize=None)
def _distinct(engine):
    """the batch of the distinct rows alone, checked against the yardstick on its first 8 rows"""
    many, check, yard = ENGINES[engine]
    rows = _dataset_rows()
    res, st = many(rows)
    for i in range(8):
        check(res, st, i, yard(rows[i]), (engine, i))
    return res, st


@pytest.mark.parametrize("n", [1, 1023, 1025])
@pytest.mark.parametrize("engine", sorted(ENGINES))
def test_search_counts_around_the_offsets_chunk(engine, n):
    many, check, yard = ENGINES[engine]
    rows = _dataset_rows()
    want_res, want_st = _distinct(engine)
    res, st = many(rows[np.arange(n) % len(rows)])
    assert len(res) == n
    for i in range(n):
        j = i % len(rows)
        assert res[i] == want_res[j] and all(st[k][i] == want_st[k][j] for k in st), (engine, n, i)
    for i in range(min(n, 8)):
        check(res, st, i, yard(rows[i]), (engine, n, i))
