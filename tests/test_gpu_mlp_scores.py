"""acx.ops.mlp_scores (acx_mlp_scores, csrc/acx_mlp.hip) against mlp.host (acx_mlp_scores_host): the
two follow one float32 arithmetic (csrc/acx_mlp.h), so they agree bit for bit -- every width class
of a hidden layer (64, 128, 256; 192 in its own case), row counts on both sides of the 4 rows a wave
evaluates together and of a wave's 64 lanes, NaN and -0.0 through the ReLU."""
import numpy as np
import pytest
import torch

import mlp_common as MC

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
MS = (1, 12, 13, 64, 65, 1000)


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _x(M, seed):
    rng = np.random.default_rng(seed)
    x = rng.normal(0, 2, (M, 14)).astype(np.float32)
    x[::7, 3] = 0.0
    x[::5] *= 40  # magnitudes of the raw features
    return x


@pytest.mark.parametrize("hidden", MC.WIDTHS + ((192, 64),))
def test_device_scores_equal_host_scores_bit_for_bit(hidden):
    import acx
    mlp = acx.DeviceMLP(*MC.random_layers(hidden, 21 + len(hidden)))
    for M in MS:
        x = _x(M, M)
        y = acx.ops.mlp_scores(torch.from_numpy(x).to(DEV), mlp)
        assert y.dtype == torch.float32 and y.shape == (M,) and y.device == DEV
        want = mlp.host(x)
        assert np.array_equal(_bits(y.cpu().numpy()), _bits(want)), (hidden, M)
        assert np.array_equal(_bits(mlp(torch.from_numpy(x).to(DEV)).cpu().numpy()), _bits(want))  # the scorer form
    assert acx.ops.mlp_scores(torch.empty((0, 14), device=DEV), mlp).shape == (0,)


def test_expm1_is_torch_expm1_of_the_same_bits():
    import acx
    mlp = acx.DeviceMLP(*MC.random_layers((128, 64), 2, 0.1))
    x = torch.from_numpy(_x(65, 9)).to(DEV)
    y = acx.ops.mlp_scores(x, mlp)
    e = acx.ops.mlp_scores(x, mlp, expm1=True)
    assert np.array_equal(_bits(y.cpu().numpy()), _bits(mlp.host(x.cpu().numpy())))
    assert np.array_equal(_bits(e.cpu().numpy()), _bits(torch.expm1(y).cpu().numpy()))
    assert not np.array_equal(_bits(e.cpu().numpy()), _bits(y.cpu().numpy()))


def test_nan_and_minus_zero_pass_the_relu_on_the_device():
    import acx
    ws, bs = MC.random_layers((128, 64), 5)
    ws[0][7, 3] = np.nan
    x = _x(13, 1)
    y = acx.ops.mlp_scores(torch.from_numpy(x).to(DEV), acx.DeviceMLP(ws, bs)).cpu().numpy()
    assert np.isnan(y).all() and np.isnan(acx.DeviceMLP(ws, bs).host(x)).all()
    ws = [np.full((64, 14), -0.0, np.float32), np.zeros((1, 64), np.float32)]
    bs = [np.full(64, -0.0, np.float32), np.full(1, -0.0, np.float32)]
    ws[1][0, 0] = 1.0  # (test_mlp_host.py: -0.0 only if the ReLU keeps -0.0)
    y = acx.ops.mlp_scores(torch.zeros((5, 14), device=DEV), acx.DeviceMLP(ws, bs)).cpu().numpy()
    assert (_bits(y) == 0x80000000).all()


def test_arguments():
    import acx
    mlp = acx.DeviceMLP(*MC.random_layers((64,), 1))
    with pytest.raises(acx._lib.ACXError, match="device tensor"):
        acx.ops.mlp_scores(torch.zeros((3, 14)), mlp)
    with pytest.raises(ValueError, match="shape"):
        acx.ops.mlp_scores(torch.zeros((3, 13), device=DEV), mlp)
    with pytest.raises(TypeError):
        acx.ops.mlp_scores(torch.zeros((3, 14), device=DEV, dtype=torch.float64), mlp)
