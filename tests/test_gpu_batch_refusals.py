"""The refusal statuses of the batched engines through the C-ABI (include/acx.h: acx_mbfs_* and
acx_mgreedy_*, the root routine of csrc/acx_batch.h).  acx.bfs_many / acx.greedy_search_many check
rows and budgets on the host, so only a caller of the C functions can meet ACX_MBFS_DOMAIN and
ACX_MBFS_OVERFLOW: a refused search has all-zero outputs, writes no path, does not disturb the
other searches of its batch and leaves nothing behind for the handle's next run."""
import numpy as np
import pytest
import torch

from many_common import _norm, _scrambled

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
CAP = 64                                  # max_nodes_each of the handle
BUDGETS = [20, 20, 20, 20, 20, 65, 20]    # row 5 asks for more than the handle holds
SENTINEL = -77


def _rows(L):
    """(the batch of 7 with its refused rows, 7 valid rows)"""
    rng = np.random.default_rng(300 + L)
    valid = np.stack([_scrambled(L, rng, 1 + i % 3) for i in range(7)])
    batch = np.zeros((7, 2 * L), np.int32)
    batch[[0, 5, 6]] = valid[0]
    batch[1, :L] = valid[0][:L]
    batch[1, L:2 * L - 1] = np.tile([1, 2], L)[:L - 1]
    batch[1, 2 * L - 1] = 3               # the row's last entry: nothing else is wrong with it
    batch[2, [0, 2, L]] = [1, 2, 2]       # a zero before a letter inside relator 0
    batch[3, 0] = 1                       # relator 1 empty
    batch[4, [0, L]] = [-3, 2]
    return batch, valid


def _alone(prefix, row, cyc=False):
    """what the wrapper returns for the row alone at budget 20"""
    import acx
    fn = acx.bfs_many if prefix == "acx_mbfs" else acx.greedy_search_many
    res, st = fn(row[None], 20, cyclically_reduce_after_moves=cyc, device=DEV, return_stats=True)
    path = _norm(res[0])[1] or []
    return dict(status=int(st["status"][0]), nodes=int(st["nodes"][0]), parents=int(st["parents"][0]),
                min_length=int(st["min_length"][0]), path=path)


def _run(lib, prefix, h, states, budgets):
    """_run and _paths on the handle: the five outputs and, per search, the region of the path
    arrays that its offset names (offsets `stride` apart, the arrays filled with SENTINEL before)"""
    n = len(states)
    stream = torch.cuda.current_stream(DEV).cuda_stream
    fn = lambda what: getattr(lib, f"{prefix}_{what}")  # noqa: E731
    with torch.cuda.device(DEV):
        st = torch.from_numpy(np.ascontiguousarray(states, np.int32)).to(DEV)
        bd = torch.tensor(budgets, dtype=torch.int64, device=DEV)
        status, min_len = (torch.full((n,), SENTINEL, dtype=torch.int32, device=DEV) for _ in range(2))
        nodes, parents, plen = (torch.full((n,), SENTINEL, dtype=torch.int64, device=DEV) for _ in range(3))
        assert fn("run")(h, st.data_ptr(), bd.data_ptr(), n, status.data_ptr(), nodes.data_ptr(), parents.data_ptr(),
                         min_len.data_ptr(), plen.data_ptr(), stream) == 0
        out = dict(status=status.cpu().numpy(), nodes=nodes.cpu().numpy(), parents=parents.cpu().numpy(),
                   min_length=min_len.cpu().numpy(), path_len=plen.cpu().numpy())
        assert out["path_len"].min() >= 0 and out["path_len"].max() <= CAP + 2
        stride = int(out["path_len"].max()) + 3
        offsets = torch.arange(n, dtype=torch.int64, device=DEV) * stride
        acts, tots = (torch.full((n * stride,), SENTINEL, dtype=torch.int32, device=DEV) for _ in range(2))
        assert fn("paths")(h, n, offsets.data_ptr(), acts.data_ptr(), tots.data_ptr(), n * stride, stream) == 0
        out["acts"] = acts.cpu().numpy().reshape(n, stride)
        out["tots"] = tots.cpu().numpy().reshape(n, stride)
    return out


def _check_search(out, i, want, keys=("status", "nodes", "parents", "min_length")):
    """search i of _run's (or test_gpu_beam_many._drive's) output against a yardstick's result"""
    got = {k: int(out[k][i]) for k in keys}
    assert got == {k: want[k] for k in got}, (i, got, want)
    k = len(want["path"])
    assert out["path_len"][i] == k, (i, want)
    assert [list(e) for e in zip(out["acts"][i][:k].tolist(), out["tots"][i][:k].tolist())] == want["path"], i
    assert (out["acts"][i][k:] == SENTINEL).all() and (out["tots"][i][k:] == SENTINEL).all(), i


@pytest.mark.parametrize("L", [13, 36])
@pytest.mark.parametrize("prefix", ["acx_mbfs", "acx_mgreedy"])
def test_refused_searches_through_the_c_abi(prefix, L):
    from acx import _lib
    from acx.search import _batch_bfs
    lib = _lib.load()
    batch, valid = _rows(L)
    alone = [_alone(prefix, r) for r in valid]
    assert alone[0]["path"] and any(len(a["path"]) >= 3 for a in alone)  # paths are written and walked
    refused = dict(nodes=0, parents=0, min_length=0, path=[])
    want = [alone[0]] + [dict(refused, status=_lib.MBFS_DOMAIN)] * 4 + [dict(refused, status=_lib.MBFS_OVERFLOW),
                                                                        alone[0]]
    with torch.cuda.device(DEV):
        h = getattr(lib, f"{prefix}_create")(L, 7, CAP, 0)
    assert h
    try:
        out = _run(lib, prefix, h, batch, BUDGETS)
        assert out["status"].tolist() == [w["status"] for w in want]
        for i, w in enumerate(want):
            _check_search(out, i, w)
        for k in out:  # rows 0 and 6 are the same search
            assert np.array_equal(out[k][0], out[k][6]), k
        # the epoch: the same handle, seven valid rows -- a refused search left nothing behind
        out = _run(lib, prefix, h, valid, [20] * 7)
        for i, w in enumerate(alone):
            _check_search(out, i, w)
    finally:
        getattr(lib, f"{prefix}_destroy")(h)
        _batch_bfs.release_workspaces()  # the wrappers' own handles (_alone)
