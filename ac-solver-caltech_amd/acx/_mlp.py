"""acx.DeviceMLP: the reference's FeatureMLP (value_search/value_network.py) as the library's own
float32 arithmetic (csrc/acx_mlp.h; C-ABI acx_mlp_scores / acx_mlp_scores_host in include/acx.h):
every output of every layer is acc = bias, then acc = fmaf(W[j][k], x[k], acc) for ascending k,
ReLU after a hidden layer, and the result is the last layer's output y -- on the device and on the
host bit for bit.  The reference scores with expm1(y); y orders the same and has neither float32
expm1's ties between neighbouring values nor its +inf above about 88.7 (ops.mlp_scores(...,
expm1=True) applies it where magnitudes matter)."""

from __future__ import annotations

import ctypes

import numpy as np
import torch

from . import _lib

IN, MAX_HIDDEN, MAX_WIDTH, WIDTH_STEP = 14, 4, 256, 64


class DeviceMLP:
    """DeviceMLP(weights, biases, device=None): the layers' torch-layout (H, K) weights and (H)
    biases, first layer first.  The limits -- input width 14, 1 to 4 hidden layers, every hidden
    width a multiple of 64 up to 256, one output -- are checked here, before any GPU call
    (ValueError).  The parameters are uploaded to `device` here, and to any other device when they are
    first used there.

    mlp(x): ops.mlp_scores(x, mlp) -- (M, 14) float32 device features -> (M,) float32 y, so an
    instance is a scorer= of beam_search_many, value_guided_greedy_search_many and mcts_search_many;
    value_guided_greedy_search_many also runs it fused, with no Python between the pops.
    mlp.host(x): the same values from a numpy array, on the host."""

    def __init__(self, weights, biases, device=None):
        ws = [np.ascontiguousarray(torch.as_tensor(w).detach().cpu().numpy(), dtype=np.float32) for w in weights]
        bs = [np.ascontiguousarray(torch.as_tensor(b).detach().cpu().numpy(), dtype=np.float32) for b in biases]
        if len(ws) != len(bs):
            raise ValueError(f"{len(ws)} weights but {len(bs)} biases")
        if not 1 <= len(ws) - 1 <= MAX_HIDDEN:
            raise ValueError(f"a DeviceMLP has 1 to {MAX_HIDDEN} hidden layers, not {len(ws) - 1}")
        dims = [IN]
        for l, (w, b) in enumerate(zip(ws, bs)):
            if w.ndim != 2 or b.shape != (w.shape[0],):
                raise ValueError(f"layer {l}: weights (H, K) and a bias (H), not {w.shape} and {b.shape}")
            if w.shape[1] != dims[-1]:
                raise ValueError(f"layer {l}: input width {w.shape[1]}, but " +
                                 (f"the input width must be {IN}" if l == 0 else f"the layer before has {dims[-1]} outputs"))
            H, last = w.shape[0], l == len(ws) - 1
            if last and H != 1:
                raise ValueError(f"the last layer must have one output, not {H}")
            if not last and (H % WIDTH_STEP or not WIDTH_STEP <= H <= MAX_WIDTH):
                raise ValueError(f"layer {l}: a hidden width must be a multiple of {WIDTH_STEP} and at most "
                                 f"{MAX_WIDTH}, not {H}")
            dims.append(H)
        self.widths = tuple(dims)
        self.n_layers = len(ws)
        self.dims = (ctypes.c_int32 * len(dims))(*dims)
        # per layer W transposed (k-major, K x H), then the bias
        self.params = np.concatenate([x for w, b in zip(ws, bs) for x in (w.T.ravel(), b)]).astype(np.float32)
        self._on = {}  # (device type, index) -> the parameters there
        if device is not None:
            self.params_on(torch.device(device))

    @classmethod
    def from_module(cls, model, device=None):
        """from the reference's FeatureMLP (its .net), or any nn.Sequential of Linear, ReLU and Dropout
        in that pattern: Linear, ReLU[, Dropout], ..., Linear.  Dropout is the identity (eval)."""
        nn = torch.nn
        seq = getattr(model, "net", model)
        if not isinstance(seq, nn.Sequential):
            raise ValueError("from_module takes a FeatureMLP or an nn.Sequential of Linear / ReLU / Dropout")
        mods = [m for m in seq if not isinstance(m, nn.Dropout)]
        ws, bs = [], []
        for i, m in enumerate(mods):
            if i % 2 == 0:
                if not isinstance(m, nn.Linear):
                    raise ValueError(f"expected a Linear layer, found {type(m).__name__}")
                ws.append(m.weight)
                bs.append(m.bias if m.bias is not None else torch.zeros(m.out_features))
            elif not isinstance(m, nn.ReLU):
                raise ValueError(f"the activation after a hidden layer must be ReLU, not {type(m).__name__}")
        if len(mods) % 2 == 0:
            raise ValueError("the network must end with a Linear layer")
        return cls(ws, bs, device)

    def params_on(self, dev: torch.device) -> torch.Tensor:
        key = (dev.type, dev.index)
        if key not in self._on:
            self._on[key] = torch.from_numpy(self.params).to(dev)
        return self._on[key]

    def __call__(self, x):
        from . import ops
        return ops.mlp_scores(x, self)

    def host(self, x):
        x = np.ascontiguousarray(x, dtype=np.float32)
        if x.ndim != 2 or x.shape[1] != IN:
            raise ValueError(f"x must be (M, {IN}), got {x.shape}")
        out = np.empty(len(x), np.float32)
        st = _lib.load().acx_mlp_scores_host(x.ctypes.data, self.params.ctypes.data, self.dims, self.n_layers,
                                             out.ctypes.data, len(x))
        _lib.check(st, "acx_mlp_scores_host")
        return out
