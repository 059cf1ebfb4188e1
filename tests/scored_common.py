"""What the GPU tests of the three searches scored by the caller (test_gpu_beam_many.py,
test_gpu_vgreedy_many.py, test_gpu_mcts_many.py; the step frame of csrc/acx_scored.h) share: the rows
they search, the module that turns a scorer into the single-search wrappers' model, and the driver
of the C-ABI's calls one by one with the checks of what it leaves for a refused search."""
import numpy as np
import torch

from many_common import _load, _scrambled
from test_gpu_batch_refusals import SENTINEL, _rows

DEV = torch.device("cuda:0")
AK3 = [1, 1, 1, -2, -2, -2, -2, 1, 2, 1, -2, -1, -2]


def _pad(letters, L, n0=7):
    s = np.zeros(2 * L, np.int32)
    s[:n0], s[L:L + len(letters) - n0] = letters[:n0], letters[n0:]
    return s


def _key(p):
    return np.ascontiguousarray(p, np.int32).tobytes()


class _FnModel(torch.nn.Module):
    def __init__(self, fn):
        super().__init__()
        self.fn = fn

    def forward(self, x):
        return self.fn(x)[:, None]


def _solvable():
    recs = [c for c in _load("greedy_many.json")["solvable"] if not c["cyclical"]][:40]
    return np.array([c["presentation"] for c in recs]), [200 + 20 * (i % 7) for i in range(len(recs))]


def _thirteen():
    _, valid = _rows(13)
    rng = np.random.default_rng(77)
    return np.concatenate([valid, np.stack([_scrambled(13, rng, 7 + i) for i in range(3)])])


class Engine:
    """How drive() steps an engine, as _scored._Steps says it on the library's side: the prefix of
    its calls, the names of its make and take call, the loop's bound as a function of the largest
    budget, the name under which its steps come back, and what the two numbers make wrote mean, as
    (M rows to score, live searches)"""

    def __init__(self, prefix, make, take, bound, steps="steps", report=lambda M, live: (M, live)):
        self.prefix, self.make, self.take, self.bound = prefix, make, take, bound
        self.steps, self.report = steps, report


def drive(lib, h, eng, states, budgets, L, fn, begin=(), make=(), short_take_at=None):
    """The C-ABI's calls of a run one by one, every status asserted 0: begin, steps of make /
    gather / fn on the features / take until no search is live, finish and paths into
    sentinel-filled outputs -> a dict of the arrays.  begin: the engine's own per-search tensors of
    its begin call (beam: the widths), make: its own arguments of the make call (mcts: the log
    table, its length, the constant), short_take_at: the step (0-based) whose take is told M - 1
    instead of M."""
    from acx import _lib, ops
    call = lambda what: getattr(lib, f"{eng.prefix}_{what}")  # noqa: E731
    n, kw = len(states), _lib.key_words(L)
    stream = torch.cuda.current_stream(DEV).cuda_stream
    with torch.cuda.device(DEV):
        st = torch.from_numpy(np.ascontiguousarray(states, np.int32)).to(DEV)
        bd = torch.tensor(budgets, dtype=torch.int64, device=DEV)
        pair = torch.zeros(2, dtype=torch.int64, device=DEV)
        assert call("begin")(h, st.data_ptr(), bd.data_ptr(), *(x.data_ptr() for x in begin), n, stream) == 0
        for step in range(eng.bound(max(budgets))):
            assert call(eng.make)(h, *make, pair.data_ptr(), stream) == 0
            M, live = eng.report(*pair.tolist())
            if live == 0:
                assert M == 0
                break
            if M == 0:
                continue
            keys = torch.empty((M, kw), dtype=torch.int64, device=DEV)
            assert call("gather")(h, keys.data_ptr(), M, stream) == 0
            y = fn(ops.features(keys=keys, L=L)).to(torch.float32).contiguous()
            assert call(eng.take)(h, y.data_ptr(), M - (step == short_take_at), stream) == 0
        else:
            raise AssertionError("the searches did not end")
        status, min_len = (torch.full((n,), SENTINEL, dtype=torch.int32, device=DEV) for _ in range(2))
        nodes, steps, plen = (torch.full((n,), SENTINEL, dtype=torch.int64, device=DEV) for _ in range(3))
        assert call("finish")(h, status.data_ptr(), nodes.data_ptr(), steps.data_ptr(), min_len.data_ptr(),
                              plen.data_ptr(), stream) == 0
        out = {"status": status.cpu().numpy(), "nodes": nodes.cpu().numpy(), eng.steps: steps.cpu().numpy(),
               "min_length": min_len.cpu().numpy(), "path_len": plen.cpu().numpy()}
        stride = int(out["path_len"].max()) + 3
        offsets = torch.arange(n, dtype=torch.int64, device=DEV) * stride
        acts, tots = (torch.full((n * stride,), SENTINEL, dtype=torch.int32, device=DEV) for _ in range(2))
        assert call("paths")(h, n, offsets.data_ptr(), acts.data_ptr(), tots.data_ptr(), n * stride, stream) == 0
        out["acts"], out["tots"] = acts.cpu().numpy().reshape(n, stride), tots.cpu().numpy().reshape(n, stride)
    return out


def _refused(out, i, status):
    """search i of drive()'s `out` was refused with `status`: no path written, every other output 0"""
    assert out["status"][i] == status and (out["acts"][i] == SENTINEL).all() and (out["tots"][i] == SENTINEL).all(), i
    assert all(out[k][i] == 0 for k in out if k not in ("status", "acts", "tots")), i
