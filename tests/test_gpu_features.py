"""GPU parity of the value-search scoring inputs (csrc/acx_features.hip): features and token
ids from int32 presentations and from packed keys, bit-exact against the reference's own
compute_features outputs (tests/golden/features.npz, features_edges.npz) and the oracle
restatement; every pair of relator lengths, a normalisation that tells the columns apart, and row
counts around a block."""
import functools
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN
from oracle import features as F

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")


def _bits(a):
    return np.asarray(a, np.float32).view(np.uint32)


@pytest.mark.parametrize("L", [18, 36, 7])
def test_features_states_and_keys_vs_reference(L):
    import acx
    from acx.search._engine import _pack_key
    d = np.load(os.path.join(GOLDEN, "features.npz"))
    st, exp = d[f"L{L}_states"].astype(np.int32), d[f"L{L}_features"]
    f = acx.ops.features(states=torch.as_tensor(st).to(DEV)).cpu().numpy()
    assert np.array_equal(_bits(f), _bits(exp))
    keys = np.stack([_pack_key(s.astype(np.int64), L) for s in st]).view(np.int64)
    fk = acx.ops.features(keys=torch.as_tensor(keys).to(DEV), L=L).cpu().numpy()
    assert np.array_equal(_bits(fk), _bits(exp))
    rng = np.random.default_rng(L)
    mean = rng.normal(size=14).astype(np.float32)
    std = rng.uniform(0.1, 5, size=14).astype(np.float32)
    fn = acx.ops.features(states=torch.as_tensor(st).to(DEV), mean=torch.as_tensor(mean).to(DEV),
                          std=torch.as_tensor(std).to(DEV)).cpu().numpy()
    assert np.array_equal(_bits(fn), _bits(F.normalise(exp, mean, std)))
    for D in (2 * L, 2 * L + 5, 72 if 72 >= 2 * L else 2 * L):
        t = acx.ops.token_ids(states=torch.as_tensor(st).to(DEV), max_state_dim=D).cpu().numpy()
        assert np.array_equal(t, F.token_ids(st, D))
        tk = acx.ops.token_ids(keys=torch.as_tensor(keys).to(DEV), L=L, max_state_dim=D).cpu().numpy()
        assert np.array_equal(tk, F.token_ids(st, D))


@pytest.mark.parametrize("L,cyc", [(36, False), (36, True), (128, False)])
def test_features_of_expand12_keys_equal_features_of_children(L, cyc):
    """The fused scoring path: expand12 packed keys -> features/tokens, without int32 children."""
    import acx
    from oracle import oracle as O
    ms = np.load(os.path.join(os.path.dirname(acx.__file__), "data", "all_presentations.npy"))
    P = np.zeros((700, 2 * L), np.int32)
    for i in range(700):
        p = ms[i % len(ms)]
        P[i, :18], P[i, L : L + 18] = p[:18], p[18:]
    res = acx.ops.expand12(torch.as_tensor(P).to(DEV), cyclical=cyc, keys=True)
    ch, _, err = O.expand12(P, L, cyc)
    ok = err.reshape(-1) == 0
    f = acx.ops.features(keys=res["keys"], L=L).cpu().numpy()[ok]
    exp = F.compute_features_batch(ch.reshape(-1, 2 * L)[ok], L)
    assert np.array_equal(_bits(f), _bits(exp))
    t = acx.ops.token_ids(keys=res["keys"], L=L).cpu().numpy()[ok]
    assert np.array_equal(t, F.token_ids(ch.reshape(-1, 2 * L)[ok], 2 * L))


# ---------------------------------------------------------------------------------------------
# the edges: letters outside the packed domain, every length pair, normalisation, row counts
# ---------------------------------------------------------------------------------------------
def _dev(a):
    return torch.from_numpy(np.array(a, order="C")).to(DEV)  # (a copy: the shared tables are read-only)


def _mismatch(got, exp):
    """the rows at which two float32 tables differ bit for bit (the first few, for the message)"""
    bad = np.nonzero((_bits(got) != _bits(exp)).any(1))[0]
    return [(int(i), got[i].tolist(), exp[i].tolist()) for i in bad[:3]], len(bad)


@pytest.mark.parametrize("L", [4, 19, 64])
def test_features_and_tokens_at_the_edges_of_the_input_domain(L):
    """tests/golden/features_edges.npz: the reference's compute_features on int32 rows with empty
    relators, zeros inside a relator, letters 3 .. 127 and -3 .. -128, and letters that are 0, +-1,
    +-2 only mod 256 -- compute_features casts to int8 first, so 257 is x and 256 is padding; the
    token ids are the raw letter + 2 in int64 (_score_states_seq does not cast).
    Before features_states_kernel truncated its letters to int8 it compared the raw int32: the
    L = 4 row [257, 256, 1, 0 | 2, 0, 0, 0] gave total = 4, len_r1 = 3 where the reference gives 3, 2."""
    import acx
    d = np.load(os.path.join(GOLDEN, "features_edges.npz"))
    st, exp = d[f"L{L}_states"], d[f"L{L}_features"]
    assert st.dtype == np.int32
    f = acx.ops.features(states=_dev(st)).cpu().numpy()
    assert np.array_equal(_bits(f), _bits(exp)), _mismatch(f, exp)
    for D in (2 * L, 2 * L + 5):
        t = acx.ops.token_ids(states=_dev(st), max_state_dim=D).cpu().numpy()
        assert t.dtype == np.int64 and np.array_equal(t, F.token_ids(st, D))
    assert F.token_ids(st, 2 * L).max() == 2 ** 31 + 1 and F.token_ids(st, 2 * L).min() == -2 ** 31 + 2


@functools.lru_cache(maxsize=None)
def _pair_table(L):
    """every pair of relator lengths 0 .. L with random letters: ((L + 1)^2, 2L) int32 states and
    their 14 features -- lengths and ratios from Python's own int / int rounded to float32 (the
    correctly rounded quotient: float32(a / b) == float32(a) / float32(b) at every pair up to 128,
    so the table fixes correct rounding, and an approximate division misses it), counts by counting"""
    rng = np.random.default_rng(1000 + L)
    n0, n1 = (x.reshape(-1) for x in np.meshgrid(np.arange(L + 1), np.arange(L + 1), indexing="ij"))
    letters = rng.choice(np.array([1, -1, 2, -2], np.int32), (len(n0), 2 * L))
    live = np.concatenate([np.arange(L)[None, :] < n0[:, None], np.arange(L)[None, :] < n1[:, None]], 1)
    st = np.where(live, letters, 0).astype(np.int32)
    exp = np.zeros((len(n0), 14), np.float32)
    for i, (a, b) in enumerate(zip(n0.tolist(), n1.tolist())):
        mn, mx = min(a, b), max(a, b)
        exp[i, [0, 1, 2, 12, 13]] = [np.float32(a + b), np.float32(a), np.float32(b),
                                     np.float32(a / (a + b) if a + b else 0.5), np.float32(mx / mn if mn else mx)]
    for h in range(2):
        for c, v in enumerate((1, -1, 2, -2)):
            exp[:, 3 + 4 * h + c] = (st[:, h * L:(h + 1) * L] == v).sum(1)
    exp[:, 11] = (exp[:, 3] - exp[:, 4]) + (exp[:, 7] - exp[:, 8])
    st.setflags(write=False)
    exp.setflags(write=False)
    return st, exp


@pytest.mark.parametrize("path,L", [("states", 128), ("keys", 128), ("keys", 64), ("keys", 48), ("keys", 32),
                                    ("keys", 16)])
def test_features_at_every_length_pair(path, L):
    """all (L + 1)^2 pairs (n0, n1), the empty relators' branches (ratio 0.5, max_min_ratio = max)
    included: L = 128 on both paths, and on the key path the full tiles of every instantiation
    (<8> 128, <4> 64, <3> 48, <2> 32, <1> 16)"""
    import acx
    from weak_hash_common import pack_keys_np
    st, exp = _pair_table(L)
    assert len(st) == (L + 1) ** 2 and exp[0].tolist() == [0] * 12 + [0.5, 0] and exp[1, 13] == 1 and exp[L + 1, 13] == 1
    if path == "states":
        f = acx.ops.features(states=_dev(st)).cpu().numpy()
    else:
        f = acx.ops.features(keys=_dev(pack_keys_np(st, L).view(np.int64)), L=L).cpu().numpy()
    assert np.array_equal(_bits(f), _bits(exp)), _mismatch(f, exp)


def test_pair_table_is_the_oracle_s():
    """the table's counting against oracle.features.compute_features (pinned to the reference on the
    CPU), at the smallest L of the pair tests"""
    st, exp = _pair_table(16)
    assert np.array_equal(_bits(F.compute_features_batch(st, 16)), _bits(exp))


# 14 distinct means and 14 distinct stds, some negative.  std[0] (itself a denormal) is so small
# that column 0's quotients overflow once |f - mean| passes 3.4 (to +inf and, below the mean, to
# -inf); std[1] so large that column 1's quotients are float32 denormals or the smallest normals;
# no std is 0 (NaN payloads differ between hosts)
NORM_MEAN = np.float32([7.5, 3.25, -1.0, 0.1, 2.0, -0.3, 1.7, 4.0, -2.5, 0.9, 3.0, -1.5, 0.3, 1.3])
NORM_STD = np.float32([1e-38, -2.5e38, 3.0, -0.7, 1.9, 2.3, -5.0, 0.11, 7.0, -1.3, 0.6, 2.9, 0.37, -4.1])


@pytest.mark.parametrize("path", ["states", "keys"])
def test_normalisation_tells_every_column_apart(path):
    """(f - mean) / std as numpy's float32 arrays compute it (oracle.features.normalise, the
    reference's value_guided_search.py:59), bit for bit on both paths: a dropped, swapped or shifted
    mean / std changes some column, and the quotients that overflow to +-inf and the denormal ones
    are IEEE's"""
    import acx
    from weak_hash_common import pack_keys_np
    assert len(set(NORM_MEAN.tolist())) == 14 and len(set(NORM_STD.tolist())) == 14 and (NORM_STD != 0).all()
    L = 16
    st, raw = _pair_table(L)
    with np.errstate(all="ignore"):
        exp = F.normalise(raw, NORM_MEAN, NORM_STD)
        assert exp.dtype == np.float32 and not np.isnan(exp).any()
        tiny = np.float32(2.0) ** -126
        assert (exp[:, 0] == np.inf).any() and (exp[:, 0] == -np.inf).any() and np.isfinite(exp[:, 0]).any()
        assert ((exp[:, 1] != 0) & (np.abs(exp[:, 1]) < tiny)).sum() > 50 and (np.abs(exp[:, 1]) >= tiny).any()
        assert np.isfinite(exp[:, 1:]).all()
        # every column's mean and std matter: with another column's in its place the column changes
        for c in range(14):
            o = (c + 1) % 14
            assert not np.array_equal(exp[:, c], (raw[:, c] - NORM_MEAN[o]) / NORM_STD[c])
            assert not np.array_equal(exp[:, c], (raw[:, c] - NORM_MEAN[c]) / NORM_STD[o])
    mean, std = _dev(NORM_MEAN), _dev(NORM_STD)
    if path == "states":
        f = acx.ops.features(states=_dev(st), mean=mean, std=std).cpu().numpy()
    else:
        f = acx.ops.features(keys=_dev(pack_keys_np(st, L).view(np.int64)), L=L, mean=mean, std=std).cpu().numpy()
    assert np.array_equal(_bits(f), _bits(exp)), _mismatch(f, exp)


@pytest.mark.parametrize("M", [1, 255, 256, 257])
def test_row_counts_around_a_block_keep_to_their_rows(M):
    """M on both sides of the 256-thread block, all four kernels writing out[:M] of a tensor with
    one more row: that row survives.  Tokens at D = 2L + 5, so that M D is no multiple of 256."""
    import acx
    from weak_hash_common import pack_keys_np
    L, D = 19, 2 * 19 + 5
    table = np.load(os.path.join(GOLDEN, "features_edges.npz"))
    rng = np.random.default_rng(M)
    st = np.zeros((M, 2 * L), np.int32)
    for r in st:
        for h in range(2):
            n = int(rng.integers(0, L + 1))
            r[h * L:h * L + n] = rng.choice([1, -1, 2, -2], n)
    wild = table["L19_states"][:M]  # (the states kernels take any letters)
    keys = _dev(pack_keys_np(st, L).view(np.int64))
    fs = np.float32(-12345.5)
    for kw, exp in ((dict(states=_dev(st)), F.compute_features_batch(st, L)),
                    (dict(states=_dev(wild)), table["L19_features"][:M]),
                    (dict(keys=keys, L=L), F.compute_features_batch(st, L))):
        out = torch.full((len(exp) + 1, 14), float(fs), dtype=torch.float32, device=DEV)
        got = acx.ops.features(out=out[:len(exp)], **kw)
        assert got.data_ptr() == out.data_ptr()
        o = out.cpu().numpy()
        assert np.array_equal(_bits(o[:-1]), _bits(exp)) and (o[-1] == fs).all()
    for kw, exp in ((dict(states=_dev(st)), F.token_ids(st, D)), (dict(states=_dev(wild)), F.token_ids(wild, D)),
                    (dict(keys=keys, L=L), F.token_ids(st, D))):
        out = torch.full((len(exp) + 1, D), -77, dtype=torch.int64, device=DEV)
        acx.ops.token_ids(out=out[:len(exp)], max_state_dim=D, **kw)
        o = out.cpu().numpy()
        assert np.array_equal(o[:-1], exp) and (o[-1] == -77).all()
        assert (len(exp) * D) % 256 != 0 or M == 256  # (D is odd: only M = 256 itself ends on a block)


def test_features_api_edges():
    import acx
    s = torch.zeros((0, 8), dtype=torch.int32, device=DEV)
    assert acx.ops.features(states=s).shape == (0, 14)
    with pytest.raises(ValueError):
        acx.ops.features(states=torch.zeros((2, 8), dtype=torch.int32, device=DEV),
                         keys=torch.zeros((2, 1), dtype=torch.int64, device=DEV), L=4)
    with pytest.raises(ValueError):
        acx.ops.token_ids(states=torch.zeros((2, 8), dtype=torch.int32, device=DEV), max_state_dim=7)
