"""What the tests of acx.DeviceMLP share (test_mlp_host.py, test_gpu_mlp_scores.py,
test_gpu_fused_vgreedy.py, weak_hash_child.py): the seeded networks, a float64 evaluation with its
error bound, and the searches of the fused value-guided greedy search with the yardstick's answers."""
import functools

import numpy as np

import vgreedy_yardstick as Y
from many_common import _scrambled
from scored_common import AK3, _key, _pad

WIDTHS = ((64,), (128, 64), (256, 256, 128), (64, 64, 64, 64))
LS = (16, 17, 33, 49, 65)  # one relator length per instantiation of the kernels (1, 2, 3, 4, 8 words)
WIDE_L = 33  # where the searches also run with the reference's default widths
ZERO, ONE = np.zeros(14, np.float32), np.ones(14, np.float32)


def random_layers(hidden, seed, scale=0.3):
    """(weights, biases) in torch layout (H, K), every entry N(0, scale^2)"""
    rng = np.random.default_rng(seed)
    dims = [14] + list(hidden) + [1]
    ws = [rng.normal(0, scale, (dims[i + 1], dims[i])).astype(np.float32) for i in range(len(dims) - 1)]
    bs = [rng.normal(0, scale, dims[i + 1]).astype(np.float32) for i in range(len(dims) - 1)]
    return ws, bs


def length_led_layers(hidden, seed):
    """unit 0 of every hidden layer carries feature 0 (the total length) through with weight 1 and
    the last layer reads it with weight 1; every other weight and bias is N(0, 0.05^2): an order
    close to greedy's, for mean 0 and std 1"""
    ws, bs = random_layers(hidden, seed, 0.05)
    for w in ws:
        w[0, 0] = 1.0
    return ws, bs


@functools.lru_cache(maxsize=None)
def net(kind, hidden, seed=0):
    """an acx.DeviceMLP and its normalisation: kind "random" (NORM_MEAN / NORM_STD) or "length"
    (mean 0, std 1)"""
    import acx
    if kind == "length":
        return acx.DeviceMLP(*length_led_layers(hidden, seed)), ZERO, ONE
    return acx.DeviceMLP(*random_layers(hidden, seed)), Y.NORM_MEAN, Y.NORM_STD


def float64_with_bound(ws, bs, x):
    """the network in float64, and the bound e_n on |y32 - y64| of a float32 evaluation whose every
    output is one chain of K fused multiply-adds from the bias: with u = 2^-24 and gamma_K = K u /
    (1 - K u), a chain over computed inputs a~ (|a~ - a| <= e) has error at most |W| e + gamma_K (|b| +
    |W| (|a| + e)); ReLU is 1-Lipschitz and |relu(a)| <= |a|, so over the absolute network
    a_l = |b_l| + |W_l| a_{l-1}:  e_l = |W_l| e_{l-1} + gamma_{K_l} (|b_l| + |W_l| (a_{l-1} + e_{l-1}))"""
    u = 2.0 ** -24
    h = np.asarray(x, np.float64)
    a, e = np.abs(h), np.zeros_like(h)
    for l, (w, b) in enumerate(zip(ws, bs)):
        w64, b64 = np.asarray(w, np.float64), np.asarray(b, np.float64)
        K = w64.shape[1]
        g = K * u / (1 - K * u)
        h = h @ w64.T + b64
        if l + 1 < len(ws):
            h = np.maximum(h, 0)
        aw = np.abs(w64).T
        e = e @ aw + g * (np.abs(b64) + (a + e) @ aw)
        a = np.abs(b64) + a @ aw
    return h[:, 0], e[:, 0]


def _raising(L):
    """r0 = r1: the root's move r1 -> r1 r0^-1 leaves an empty relator, which raises in the reference"""
    s = np.zeros(2 * L, np.int32)
    s[:3], s[L:L + 3] = [1, 2, 1], [1, 2, 1]
    return s


@functools.lru_cache(maxsize=None)
def search_case(L):
    """(presentations, budgets) of relator length L: AK(3) twice (a budget ending and budget 1),
    trivial presentations after 6, 9 and 4 moves, AK(3) reversed, and a root at which a move raises"""
    rng = np.random.default_rng(900 + L)
    pres = np.stack([_pad(AK3, L), _scrambled(L, rng, 6), _scrambled(L, rng, 9), _pad(AK3, L), _raising(L),
                     _pad(AK3[::-1], L, 6), _scrambled(L, rng, 4)])
    return pres, (600, 400, 333, 1, 50, 257, 120)


@functools.lru_cache(maxsize=None)
def yard(key, kind, hidden, budget, cyc):
    mlp, mean, std = net(kind, hidden)
    return Y.vgreedy(np.frombuffer(key, np.int32), mlp.host, budget, cyc, mean=mean, std=std, drop_twins=True)


def yards(L, kind, hidden, cyc):
    pres, budgets = search_case(L)
    return [yard(_key(p), kind, hidden, b, cyc) for p, b in zip(pres, budgets)]
