"""acx.DeviceMLP on the host (acx_mlp_scores_host, csrc/acx_mlp_host.cpp; no GPU): its float32
arithmetic against a float64 evaluation within a derived bound, the corners of the contract, what
the constructor and from_module refuse, and that the searches of test_gpu_fused_vgreedy.py are not
vacuous (by the yardstick, tests/vgreedy_yardstick.py, scored by mlp.host)."""
import ctypes
import os

import numpy as np
import pytest
import torch

import mlp_common as MC
import vgreedy_yardstick as Y
from beam_yardstick import features_np, normalise_np
from conftest import GOLDEN
from many_common import _scrambled


def _inputs():
    """normalised features of the edge rows of tests/golden/features_edges.npz and of random presentations"""
    d = np.load(os.path.join(GOLDEN, "features_edges.npz"))
    f = [normalise_np(d[f"L{L}_features"], Y.NORM_MEAN, Y.NORM_STD) for L in (4, 19, 64)]
    rng = np.random.default_rng(3)
    rows = np.stack([_scrambled(24, rng, 3 + i % 20) for i in range(60)])
    f.append(normalise_np(features_np(rows, 24), Y.NORM_MEAN, Y.NORM_STD))
    f.append(features_np(rows, 24))
    return np.concatenate(f).astype(np.float32)


@pytest.mark.parametrize("hidden", MC.WIDTHS)
def test_host_mlp_against_float64_within_the_derived_bound(hidden):
    import acx
    ws, bs = MC.random_layers(hidden, 11 + len(hidden))
    x = _inputs()
    assert len(x) >= 1000 and np.isfinite(x).all()
    y32 = acx.DeviceMLP(ws, bs).host(x)
    y64, bound = MC.float64_with_bound(ws, bs, x)
    err = np.abs(y32.astype(np.float64) - y64)
    print("widths", hidden, "max error", err.max(), "its bound", bound[err.argmax()], "max |y|", np.abs(y64).max())
    assert y32.dtype == np.float32 and y32.shape == (len(x),)
    assert (err <= bound).all(), (err.max(), bound[err.argmax()])
    assert err.max() > 0  # float32 at work


def test_a_nan_weight_gives_nan_and_negative_preactivations_give_the_last_bias():
    import acx
    ws, bs = MC.random_layers((128, 64), 5)
    x = _inputs()[:40]
    ws[0][7, 3] = np.nan  # one unit of the first layer: the ReLU does not wash it out
    assert np.isnan(acx.DeviceMLP(ws, bs).host(x)).all()
    ws, bs = MC.random_layers((128, 64), 5)
    ws[1][:] = -np.abs(ws[1])  # layer 2 of non-negative inputs with non-positive weights and biases:
    bs[1][:] = -np.abs(bs[1])  # every pre-activation is negative, so the last layer sees zeros
    y = acx.DeviceMLP(ws, bs).host(x)
    assert np.array_equal(y.view(np.uint32), np.full(len(x), bs[2][0], np.float32).view(np.uint32))


def test_minus_zero_passes_the_relu():
    """v < 0 ? 0 : v keeps -0.0: every chain of the first layer is fmaf(-0.0, +0.0, -0.0) = -0.0, and
    the last layer's fmaf(w, -0.0, -0.0) with w >= 0 stays -0.0; a ReLU that returned +0.0 would give
    fmaf(1, +0.0, -0.0) = +0.0"""
    import acx
    ws = [np.full((64, 14), -0.0, np.float32), np.zeros((1, 64), np.float32)]
    bs = [np.full(64, -0.0, np.float32), np.full(1, -0.0, np.float32)]
    ws[1][0, 0] = 1.0
    y = acx.DeviceMLP(ws, bs).host(np.zeros((1, 14), np.float32))
    assert y.view(np.uint32)[0] == 0x80000000


BAD = {"width 63": (14, 63, 1), "width 320": (14, 320, 1), "no hidden layer": (14, 1),
       "five hidden layers": (14, 64, 64, 64, 64, 64, 1), "input width 13": (13, 64, 1),
       "two outputs": (14, 64, 2)}


@pytest.mark.parametrize("name", BAD)
def test_widths_outside_the_limits_are_refused(name):
    import acx
    from acx import _lib
    dims = BAD[name]
    ws = [np.zeros((dims[i + 1], dims[i]), np.float32) for i in range(len(dims) - 1)]
    bs = [np.zeros(dims[i + 1], np.float32) for i in range(len(dims) - 1)]
    with pytest.raises(ValueError, match="hidden|input width|one output"):
        acx.DeviceMLP(ws, bs)
    lib = _lib.load()
    params = np.zeros(sum((dims[i] + 1) * dims[i + 1] for i in range(len(dims) - 1)), np.float32)
    x, out = np.zeros((2, 14), np.float32), np.zeros(2, np.float32)
    d = (ctypes.c_int32 * len(dims))(*dims)
    assert lib.acx_mlp_scores_host(x.ctypes.data, params.ctypes.data, d, len(dims) - 1, out.ctypes.data, 2) == _lib.E_ARG
    # (the device entry checks its arguments before any GPU call)
    assert lib.acx_mlp_scores(x.ctypes.data, params.ctypes.data, d, len(dims) - 1, out.ctypes.data, 2, None) == _lib.E_ARG
    assert lib.acx_vgreedy_run_mlp(None, params.ctypes.data, d, len(dims) - 1, None, None, 1, out.ctypes.data,
                                   None) == _lib.E_ARG


def test_from_module():
    import acx
    nn = torch.nn
    torch.manual_seed(4)
    seq = nn.Sequential(nn.Linear(14, 128), nn.ReLU(), nn.Dropout(0.1), nn.Linear(128, 64), nn.ReLU(), nn.Linear(64, 1))
    lin = [m for m in seq if isinstance(m, nn.Linear)]
    a = acx.DeviceMLP.from_module(seq)
    b = acx.DeviceMLP([m.weight for m in lin], [m.bias for m in lin])
    assert a.widths == b.widths == (14, 128, 64, 1) and np.array_equal(a.params, b.params)
    x = _inputs()[:50]
    assert np.array_equal(a.host(x).view(np.uint32), b.host(x).view(np.uint32))
    assert np.allclose(a.host(x), seq.eval()(torch.from_numpy(x)).detach().numpy()[:, 0], rtol=1e-4, atol=1e-4)

    class Wrapped(nn.Module):  # the reference's FeatureMLP keeps its layers in .net
        def __init__(self):
            super().__init__()
            self.net = seq

    assert np.array_equal(acx.DeviceMLP.from_module(Wrapped()).params, a.params)
    for bad in (nn.Sequential(nn.Linear(14, 64), nn.Tanh(), nn.Linear(64, 1)),
                nn.Sequential(nn.Linear(14, 64), nn.ReLU()), nn.Linear(14, 1)):
        with pytest.raises(ValueError, match="ReLU|end with|Sequential"):
            acx.DeviceMLP.from_module(bad)


def test_fused_arguments_are_checked_before_any_gpu_call():
    import acx
    mlp, mean, std = MC.net("random", (64,))
    pres, budgets = MC.search_case(16)
    with pytest.raises(ValueError, match="fused=True needs"):
        acx.value_guided_greedy_search_many(pres, lambda f: f[:, 0], budgets, fused=True)
    with pytest.raises(ValueError, match="fused=True needs"):
        acx.value_guided_greedy_search_many(pres, mlp, budgets, scorer_input="tokens", fused=True)
    with pytest.raises(ValueError, match="pops_per_launch"):
        acx.value_guided_greedy_search_many(pres, mlp, budgets, pops_per_launch=0)
    with pytest.raises(ValueError, match="architecture='mlp'"):
        acx.value_guided_greedy_search(pres[0], torch.nn.Sequential(), "cnn", mean, std, fused=True)


def test_the_fused_searches_are_not_vacuous():
    """over the searches test_gpu_fused_vgreedy.py runs: a pop with 12 candidates, a pop without a
    candidate after which the search went on, a pop whose entry tied on score and depth, every
    ending, and pops from levels 1 and 2 of the heap"""
    ys = [y for L in MC.LS for cyc in (False, True) for kind in ("random", "length")
          for y in MC.yards(L, kind, (64,), cyc)]
    ys += [y for kind in ("random", "length") for y in MC.yards(MC.WIDE_L, kind, (256, 256, 128), False)]
    assert any(12 in y["cands"] for y in ys)
    assert any(y["empty_pops"] for y in ys)
    assert any(y["id_ties"] > 0 for y in ys)
    assert {y["status"] for y in ys} >= {Y.FOUND, Y.BUDGET, Y.MOVE_ERROR}
    assert any(y["level_pops"][1] > 0 for y in ys) and any(y["level_pops"][2] > 0 for y in ys)
    assert any(y["status"] == Y.BUDGET and y["steps"] == 1 for y in ys)  # budget 1: one pop
    assert max(y["nodes"] for y in ys) <= 611
