"""The fused value-guided greedy search (acx_vgreedy_run_mlp, csrc/acx_vgreedy.hip: pop, features,
normalisation, the network of csrc/acx_mlp.h and push in one kernel, many pops per launch) through
acx.value_guided_greedy_search_many with an acx.DeviceMLP: against the yardstick
(tests/vgreedy_yardstick.py) scored by mlp.host -- the network's arithmetic is one on both sides, so
results, statuses, nodes, steps and min_length are equal, not close -- against the stepped loop
with the same scorer, across launch boundaries, groups, a solution cache, a NaN, the single-search
wrapper, the C-ABI's refusals and the weak-hash library.  test_mlp_host.py asserts on the CPU that
these searches are not vacuous."""
import numpy as np
import pytest
import torch

import mlp_common as MC
import vgreedy_yardstick as Y
import weak_hash_common as W
from many_common import _norm, _same
from scored_common import AK3, SENTINEL, _pad, _refused
from test_gpu_batch_refusals import _check_search as _refusals_check_search
from test_gpu_batch_refusals import _rows

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
NARROW = (64,)
WIDE = (256, 256, 128)
DEAD = []  # why the weak-hash child died: the tests after it are skipped


@pytest.fixture(autouse=True)
def _one_death_ends_the_module():
    W.skip_after_death(DEAD)


def _many(L, kind, hidden, cyc, **kw):
    import acx
    mlp, mean, std = MC.net(kind, hidden)
    pres, budgets = MC.search_case(L)
    res, st = acx.value_guided_greedy_search_many(pres, mlp, list(budgets), cyclically_reduce_after_moves=cyc,
                                                  feat_mean=mean, feat_std=std, device=DEV, on_error="return",
                                                  return_stats=True, **kw)
    assert len(res) == len(pres) and all(len(v) == len(pres) for v in st.values())
    return [_norm(r) for r in res], st


def _check_yardstick(res, st, ys, tag):
    for i, y in enumerate(ys):
        assert res[i] == (None if y["raises"] else [y["ok"], y["path"]]), (tag, i)
        got = (st["status"][i], st["nodes"][i], st["steps"][i], st["min_length"][i])
        assert got == (y["status"], y["nodes"], y["steps"], y["min_length"]), (tag, i, got)


@pytest.mark.parametrize("L", MC.LS)
def test_fused_search_equals_the_yardstick_and_the_stepped_loop(L):
    """every instantiation of the kernel (1, 2, 3, 4 and 8 words), both flags, both networks; budgets
    per search (budget 1 among them) and a root at which a move raises in the batch"""
    for cyc in (False, True):
        for kind in ("random", "length"):
            fused = _many(L, kind, NARROW, cyc)
            _check_yardstick(*fused, MC.yards(L, kind, NARROW, cyc), (L, cyc, kind))
            assert _same(_many(L, kind, NARROW, cyc, fused=False), fused), (L, cyc, kind)
    assert fused[0][4] is None and fused[1]["status"][4] == Y.MOVE_ERROR and fused[1]["steps"][3] == 1


@pytest.mark.parametrize("kind", ["random", "length"])
def test_the_reference_widths(kind):
    fused = _many(MC.WIDE_L, kind, WIDE, False)
    _check_yardstick(*fused, MC.yards(MC.WIDE_L, kind, WIDE, False), kind)
    assert _same(_many(MC.WIDE_L, kind, WIDE, False, fused=False), fused)


def test_launch_boundaries():
    """a launch of 1 pop, of 7 and of 4,096: the handle's state persists between launches"""
    for L, cyc in ((17, False), (65, True)):
        whole = _many(L, "length", NARROW, cyc)
        assert _same(_many(L, "length", NARROW, cyc, pops_per_launch=1), whole)
        assert _same(_many(L, "length", NARROW, cyc, pops_per_launch=7), whole)
        assert whole[1]["steps"].max() > 50


def test_groups():
    from acx import _lib
    from acx.search import _batch_vgreedy as V
    whole = _many(33, "random", NARROW, False)
    V.release_workspaces()
    per = _lib.load().acx_vgreedy_bytes(33, 600)
    split = _many(33, "random", NARROW, False, workspace_bytes=3 * per - 1)  # groups of 2: 3 full, one of 1
    assert V._HANDLES[(0, 33, False)][1] == 2
    assert _same(split, whole)
    V.release_workspaces()


def test_solution_cache():
    import acx
    L = 17
    mlp, mean, std = MC.net("length", NARROW)
    pres, budgets = MC.search_case(L)
    plain = _many(L, "length", NARROW, False)
    solved = [i for i, r in enumerate(plain[0]) if r is not None and r[0] and len(r[1]) >= 3]
    assert solved
    cache = acx.SolutionCache(L, DEV)
    try:
        cache.backfill_many(pres[solved[:1]], [[tuple(x) for x in plain[0][solved[0]][1]]])
        fused = _many(L, "length", NARROW, False, solution_cache=cache)
        stepped = _many(L, "length", NARROW, False, solution_cache=cache, fused=False)
    finally:
        cache.close()
    assert _same(fused, stepped)
    assert fused[1]["cache_hit"][solved[0]] and (fused[1]["status"] == acx._lib.BFS_CACHED).sum() >= 1
    assert fused[0][solved[0]] == plain[0][solved[0]]  # the root hits: the cached path itself
    assert _same(_many(L, "length", NARROW, False), plain)  # the attachment is gone with the call


def test_a_cache_hit_below_the_root():
    """the cache holds a solved search's path from its second state on: that search's root misses, and
    the child of its first pop that is the path's second state hits, in the cached kernel's own probe"""
    import acx
    import cache_yardstick as CY
    from oracle import oracle as O
    L = 16
    pres, budgets = MC.search_case(L)
    plain = _many(L, "length", NARROW, False)
    i = next(i for i, r in enumerate(plain[0]) if r is not None and r[0] and len(r[1]) >= 3)
    path = [tuple(x) for x in plain[0][i][1]]
    out, _, err = O.move_batch(pres[i][None], np.array([path[0][0]], np.int32), L, False)
    assert err[0] == 0
    second = out[0].astype(np.int32)
    d = {}
    CY.backfill(d, second, path[1:])
    assert CY.check(pres[i], L, d) is None and CY.check(second, L, d) is not None
    cache = acx.SolutionCache(L, DEV)
    try:
        cache.backfill_many(second[None], [path[1:]])
        fused = _many(L, "length", NARROW, False, solution_cache=cache)
        stepped = _many(L, "length", NARROW, False, solution_cache=cache, fused=False)
    finally:
        cache.close()
    assert _same(fused, stepped)
    assert fused[1]["status"][i] == acx._lib.BFS_CACHED and fused[1]["steps"][i] == 1 and fused[1]["cache_hit"][i]
    assert fused[0][i][0] and len(fused[0][i][1]) >= 2


def test_a_nan_weight_raises_as_the_stepped_path_does():
    import acx
    ws, bs = MC.random_layers(NARROW, 0)
    ws[1][0, 5] = np.nan
    mlp = acx.DeviceMLP(ws, bs)
    pres, budgets = MC.search_case(16)
    for fused in (True, False):
        with pytest.raises(ValueError, match=r"the scorer returned NaN in searches \["):
            acx.value_guided_greedy_search_many(pres[:3], mlp, 100, device=DEV, fused=fused)
    assert _same(_many(16, "random", NARROW, False), _many(16, "random", NARROW, False, fused=False))  # the handle is usable


def test_the_single_search_wrapper():
    import acx
    nn = torch.nn
    ws, bs = MC.length_led_layers(NARROW, 0)
    model = nn.Sequential(nn.Linear(14, 64), nn.ReLU(), nn.Dropout(0.1), nn.Linear(64, 1))
    with torch.no_grad():
        for m, w, b in zip([model[0], model[3]], ws, bs):
            m.weight.copy_(torch.from_numpy(w))
            m.bias.copy_(torch.from_numpy(b))
    model = model.to(DEV).eval()
    pres, budgets = MC.search_case(17)
    res, st = _many(17, "length", NARROW, False)
    for i in (0, 1):
        ok, path, stats = acx.value_guided_greedy_search(pres[i], model, "mlp", MC.ZERO, MC.ONE,
                                                         max_nodes_to_explore=budgets[i], device=DEV, fused=True)
        assert [ok, [list(x) for x in path]] == res[i]
        assert stats == {"nodes_explored": st["nodes"][i], "min_length": st["min_length"][i]}
    with pytest.raises(ValueError, match="architecture='mlp'"):
        acx.value_guided_greedy_search(pres[0], model, "cnn", MC.ZERO, MC.ONE, device=DEV, fused=True)


@pytest.mark.parametrize("L", [13, 36])
def test_refused_searches_through_the_c_abi(L):
    """acx_vgreedy_run_mlp next to refused roots: ACX_MBFS_DOMAIN for a row outside the packed domain
    and ACX_MBFS_OVERFLOW for a budget above the handle's leave all-zero outputs and no path, the other
    searches are the yardstick's, and `pair` counts the launch's pops and the live searches"""
    from acx import _lib
    lib = _lib.load()
    mlp, mean, std = MC.net("random", NARROW)
    batch, _ = _rows(L)  # rows 1 .. 4 outside the domain
    batch[[0, 5, 6]] = _pad(AK3, L)  # rows 0, 5, 6: AK(3), which searches on for many pops
    budgets = [40, 40, 40, 40, 40, 65, 30]  # row 5 asks for more than the handle holds
    n = len(batch)
    stream = torch.cuda.current_stream(DEV).cuda_stream
    with torch.cuda.device(DEV):
        h = lib.acx_vgreedy_create(L, n, 64, 0)
        assert h
        try:
            st = torch.from_numpy(np.ascontiguousarray(batch, np.int32)).to(DEV)
            bd = torch.tensor(budgets, dtype=torch.int64, device=DEV)
            pair = torch.full((2,), SENTINEL, dtype=torch.int64, device=DEV)
            params, mean_d, std_d = mlp.params_on(DEV), torch.from_numpy(mean).to(DEV), torch.from_numpy(std).to(DEV)
            assert lib.acx_vgreedy_begin(h, st.data_ptr(), bd.data_ptr(), n, stream) == 0
            run = lambda pops: lib.acx_vgreedy_run_mlp(h, params.data_ptr(), mlp.dims, mlp.n_layers, mean_d.data_ptr(),  # noqa: E731
                                                       std_d.data_ptr(), pops, pair.data_ptr(), stream)
            assert run(0) == _lib.E_ARG and lib.acx_vgreedy_run_mlp(h, params.data_ptr(), mlp.dims, mlp.n_layers,
                                                                    mean_d.data_ptr(), None, 5, pair.data_ptr(),
                                                                    stream) == _lib.E_ARG
            assert run(2) == 0
            ys = [Y.vgreedy(batch[i], mlp.host, budgets[i], mean=mean, std=std, drop_twins=True) for i in (0, 6)]
            assert all(y["steps"] > 2 for y in ys)
            assert pair.tolist() == [4, 2]  # two searches ran two pops each and are live
            total = 4
            for _ in range(64):
                assert run(5) == 0
                pops, live = pair.tolist()
                total += pops
                if live == 0:
                    break
            assert live == 0 and total == sum(y["steps"] for y in ys)
            status, min_len = (torch.full((n,), SENTINEL, dtype=torch.int32, device=DEV) for _ in range(2))
            nodes, steps, plen = (torch.full((n,), SENTINEL, dtype=torch.int64, device=DEV) for _ in range(3))
            assert lib.acx_vgreedy_finish(h, status.data_ptr(), nodes.data_ptr(), steps.data_ptr(), min_len.data_ptr(),
                                          plen.data_ptr(), stream) == 0
            out = {"status": status.cpu().numpy(), "nodes": nodes.cpu().numpy(), "steps": steps.cpu().numpy(),
                   "min_length": min_len.cpu().numpy(), "path_len": plen.cpu().numpy()}
            stride = int(out["path_len"].max()) + 3
            offsets = torch.arange(n, dtype=torch.int64, device=DEV) * stride
            acts, tots = (torch.full((n * stride,), SENTINEL, dtype=torch.int32, device=DEV) for _ in range(2))
            assert lib.acx_vgreedy_paths(h, n, offsets.data_ptr(), acts.data_ptr(), tots.data_ptr(), n * stride, stream) == 0
            out["acts"], out["tots"] = acts.cpu().numpy().reshape(n, stride), tots.cpu().numpy().reshape(n, stride)
        finally:
            lib.acx_vgreedy_destroy(h)
    for i, w in enumerate([0, _lib.MBFS_DOMAIN, _lib.MBFS_DOMAIN, _lib.MBFS_DOMAIN, _lib.MBFS_DOMAIN, _lib.MBFS_OVERFLOW, 0]):
        if w < 0:
            _refused(out, i, w)
        else:
            _refusals_check_search(out, i, ys[i // 6], ("status", "nodes", "steps", "min_length"))


def test_through_the_weak_hash_library(tmp_path):
    """one case of the comparison with the yardstick through libacx_weakhash.so (8 hash classes: every
    insert of the visited set meets other states' entries): a fresh process, as
    tests/weak_hash_child.py runs the other engines"""
    L, kind, cyc = 17, "length", False
    pres, budgets = MC.search_case(L)
    calls = [dict(op="vgreedy_mlp_many", pres=pres.tolist(), budgets=list(budgets), cyc=cyc, kind=kind,
                  hidden=list(NARROW), fused=f) for f in (True, False)]
    try:
        (fused, stepped), _, _ = W.run_child(calls, tmp_path, timeout=120)
    except W.ChildDied as e:
        DEAD.append(f"the weak-hash child died: {e}")
        pytest.fail(DEAD[-1])
    want = _many(L, kind, NARROW, cyc)
    for got in (fused, stepped):
        assert got["res"] == want[0]
        assert all(np.array_equal(got["st"][k], want[1][k]) for k in want[1])
    big = [(n, c) for n, c in zip(fused["nodes"], fused["classes"]) if n >= 512]
    assert big
    for n, c in big:
        W.check_classes(n, c, "vgreedy_mlp_many")
    _check_yardstick([r for r in fused["res"]], {k: np.array(v) for k, v in fused["st"].items()},
                     MC.yards(L, kind, NARROW, cyc), "weak hash")
