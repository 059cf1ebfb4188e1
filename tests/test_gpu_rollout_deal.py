"""GPU: the rollout's XCC deal (acx_rollout_deal, ops.rollout / RolloutPlan deal="xcc": a workgroup
finds its block of 256 envs from the XCC it runs on, and steals from the other XCCs' ranges when its
own is exhausted) gives the bytes of the plain deal (block = workgroup index) and of the oracle env
replay -- at every weight, including 0 %, where the odd XCCs own nothing and every workgroup on
them steals; every block is run exactly once; the heads are re-armed by every launch; plans do not
share heads; and deal=None takes the deal only above one resident round (and only for launches of
more than 32 steps)."""
import functools

import numpy as np
import pytest
import torch

from oracle import oracle as O

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
H = 5           # horizon: resets happen
SENTINEL = -7   # no observation holds it
NAMES = ("state", "step_count", "obs", "reward", "done", "truncated", "err", "err_count")


def _starts(L, B, seed=0):
    import os

    import acx
    ms = np.load(os.path.join(os.path.dirname(acx.__file__), "data", "all_presentations.npy"))
    rng = np.random.default_rng(seed)
    out = np.zeros((B, 2 * L), np.int32)
    for i in range(B):
        p = ms[rng.integers(len(ms))]
        a, b = p[:18][p[:18] != 0], p[18:][p[18:] != 0]
        a, b = a[:L], b[:L]
        out[i, : len(a)] = a
        out[i, L : L + len(b)] = b
    return out


def _chosen_pct():
    from acx import _lib
    return _lib.DEAL_PCT


def _bufs(L, B, T):
    return dict(obs_traj=torch.full((T, B, 2 * L), SENTINEL, dtype=torch.int32, device=DEV),
                reward_traj=torch.zeros((T, B), dtype=torch.int32, device=DEV),
                done_traj=torch.zeros((T, B), dtype=torch.uint8, device=DEV),
                trunc_traj=torch.zeros((T, B), dtype=torch.uint8, device=DEV),
                err=torch.zeros(B, dtype=torch.uint8, device=DEV),
                err_count=torch.zeros(1, dtype=torch.int32, device=DEV))


def _outputs(st, cnt, b):
    return [x.cpu().numpy() for x in (st, cnt, b["obs_traj"], b["reward_traj"], b["done_traj"], b["trunc_traj"],
                                      b["err"], b["err_count"])]


def _roll(starts, acts, L, pack, **deal):
    from acx import ops
    T, B = acts.shape
    st = torch.tensor(starts, device=DEV)  # copies: the cached inputs are read-only
    cnt = torch.zeros(B, dtype=torch.int32, device=DEV)
    b = _bufs(L, B, T)
    ops.rollout(st, torch.tensor(acts, device=DEV), st.clone(), cnt, horizon=H, cyclical=True, pack_actions=pack,
                **b, **deal)
    return _outputs(st, cnt, b)


def _same(got, want):
    for n, x, y in zip(NAMES, got, want):
        assert np.array_equal(x, y), n


# L, B, T, packed ids.  B = 64: one tile, one wave; 2,000: the last block holds 208 envs (a partial
# last wave, 3 of 4 waves live); 256*8*3 + 100: ranges of unequal size and a partial last block;
# L = 128 and 17: the other tile types.  T = 40: the packed path with a partial last id group;
# T = 13: the int32 ids.
SHAPES = [(36, 64, 40, True), (36, 2000, 40, True), (36, 256 * 8 * 3 + 100, 40, True), (36, 2000, 13, False),
          (128, 333, 40, True), (17, 333, 40, True)]


@functools.lru_cache(maxsize=None)
def _case(L, B, T, pack):
    """a shape's inputs, its plain launch and its oracle replay (same-step autoreset), made once"""
    rng = np.random.default_rng(L * 1000 + B + T)
    starts = _starts(L, B, seed=T)
    acts = rng.integers(0, 12, size=(T, B)).astype(np.int32)
    plain = _roll(starts, acts, L, pack, deal="plain")
    st = starts.copy()
    cnt = np.zeros(B, np.int32)
    obs, rew, dn, tr = (np.zeros_like(plain[i]) for i in (2, 3, 4, 5))
    for t in range(T):
        rew[t], dn[t], tr[t], _, _, _ = O.env_step(st, acts[t], L, H, cnt, reset_state=starts, cyclical=True)
        obs[t] = st
    oracle = [st, cnt, obs, rew, dn, tr, np.zeros(B, np.uint8), np.zeros(1, np.int32)]
    for x in (starts, acts, *plain, *oracle):
        x.setflags(write=False)
    return starts, acts, plain, oracle


@pytest.mark.parametrize("pct", [100, "chosen", 0])
@pytest.mark.parametrize("L,B,T,pack", SHAPES)
def test_xcc_deal_equals_plain_and_oracle(L, B, T, pack, pct):
    pct = _chosen_pct() if pct == "chosen" else pct
    starts, acts, plain, oracle = _case(L, B, T, pack)
    _same(plain, oracle)
    assert (plain[4] | plain[5]).any()  # resets happened
    got = _roll(starts, acts, L, pack, deal="xcc", deal_pct=pct)
    assert not (got[2] == SENTINEL).any()
    _same(got, plain)
    _same(got, oracle)


def test_empty_odd_ranges_with_fewer_tiles_than_xccs():
    """5 tiles at 0 %: the odd XCCs' ranges are empty and three XCCs' worth of workgroups find
    their own range gone at once"""
    from acx import ops
    L, B, T = 36, 256 * 5, 40
    info = ops.rollout_deal_info(T, B, L, torch.empty(0, dtype=torch.int32), deal="xcc", deal_pct=0)
    assert info["xcc"] and info["tiles"] == 5 < 8 and sum(info["quotas"]) == 5
    assert all(q == 0 for q in info["quotas"][1::2])
    assert info["grid"] >= info["tiles"] and info["grid"] % 8 == 0
    starts, acts, plain, oracle = _case(L, B, T, True)
    got = _roll(starts, acts, L, True, deal="xcc", deal_pct=0)
    assert not (got[2] == SENTINEL).any()
    _same(got, plain)
    _same(got, oracle)


@pytest.mark.parametrize("pct", [100, "chosen", 0])
def test_every_tile_is_run_exactly_once(pct):
    """2 % of the ids outside [0, 12): err_count is the number of envs hit (a tile run twice would
    count its envs twice and step its states twice), and no sentinel is left (no tile skipped)"""
    pct = _chosen_pct() if pct == "chosen" else pct
    L, B, T = 36, 256 * 8 * 3 + 100, 40
    rng = np.random.default_rng(11)
    starts = _starts(L, B, seed=2)
    acts = rng.integers(0, 12, size=(T, B)).astype(np.int32)
    bad = rng.random((T, B)) < 0.02
    acts[bad] = rng.choice(np.array([12, 15, 16, -1, 1 << 20, -(1 << 31), 255], np.int32), size=int(bad.sum()))
    hit = bad.any(0)
    plain = _roll(starts, acts, L, True, deal="plain")
    got = _roll(starts, acts, L, True, deal="xcc", deal_pct=pct)
    assert not (got[2] == SENTINEL).any()
    assert int(got[7][0]) == int(hit.sum())
    assert (got[6][hit] == 4).all() and (got[6][~hit] == 0).all()
    _same(got, plain)


def _plan_pair(L, B, T, starts, **deal):
    """-> (plan, its state, count and buffers)"""
    from acx import ops
    st, cnt, b = starts.clone(), torch.zeros(B, dtype=torch.int32, device=DEV), _bufs(L, B, T)
    return ops.RolloutPlan(st, starts, cnt, T=T, horizon=H, cyclical=True, **b, **deal), st, cnt, b


def test_heads_are_rearmed_by_every_launch():
    """one RolloutPlan called three times in a row equals three plain calls"""
    from acx import ops
    L, B, T = 36, 2000, 40
    rng = np.random.default_rng(3)
    starts = torch.as_tensor(_starts(L, B, seed=3)).to(DEV)
    acts = torch.as_tensor(rng.integers(0, 12, size=(3 * T, B)).astype(np.int32)).to(DEV)
    plan, st_b, cnt_b, bb = _plan_pair(L, B, T, starts, deal="xcc", deal_pct=0)
    assert plan.deal == "xcc" and plan.deal_info["xcc"]
    st_a, cnt_a, ba = starts.clone(), torch.zeros(B, dtype=torch.int32, device=DEV), _bufs(L, B, T)
    for k in range(3):
        a = acts[k * T:(k + 1) * T]
        ops.rollout(st_a, a, starts, cnt_a, horizon=H, cyclical=True, deal="plain", **ba)
        bb["obs_traj"].fill_(SENTINEL)
        plan(a)
        torch.cuda.synchronize()
        assert not (bb["obs_traj"] == SENTINEL).any(), k
        _same(_outputs(st_b, cnt_b, bb), _outputs(st_a, cnt_a, ba))


def test_two_plans_on_two_streams_do_not_share_heads():
    from acx import ops
    L, B, T = 36, 256 * 8 * 3 + 100, 40
    rng = np.random.default_rng(4)
    starts = torch.as_tensor(_starts(L, B, seed=4)).to(DEV)
    acts = [torch.as_tensor(rng.integers(0, 12, size=(T, B)).astype(np.int32)).to(DEV) for _ in range(2)]
    plans = [_plan_pair(L, B, T, starts, deal="xcc", deal_pct=pct) for pct in (0, _chosen_pct())]
    assert plans[0][0]._deal_ws.data_ptr() != plans[1][0]._deal_ws.data_ptr()
    want = []
    for a in acts:
        st, cnt, b = starts.clone(), torch.zeros(B, dtype=torch.int32, device=DEV), _bufs(L, B, T)
        ops.rollout(st, a, starts, cnt, horizon=H, cyclical=True, deal="plain", **b)
        want.append(_outputs(st, cnt, b))
    torch.cuda.synchronize()
    streams = [torch.cuda.Stream(device=DEV) for _ in range(2)]
    for (plan, *_), a, s in zip(plans, acts, streams):  # back to back, then synchronised
        with torch.cuda.stream(s):
            plan(a)
    torch.cuda.synchronize()
    for (plan, st, cnt, b), w in zip(plans, want):
        assert not (b["obs_traj"] == SENTINEL).any()
        _same(_outputs(st, cnt, b), w)


def test_auto_rule_takes_the_deal_only_above_one_resident_round():
    """deal=None: plain while the batch fits one resident round of the kernel (blocks per CU from
    the occupancy query x CUs), the XCC deal above it for launches of more than 32 steps; asked of
    the plan, not timed.  No trajectory here, so the larger batch stays small in memory."""
    from acx import ops
    L, T = 36, 38

    def plan_for(B, T=T, **deal):
        st = torch.zeros((B, 2 * L), dtype=torch.int32, device=DEV)
        st[:, 0], st[:, L] = 1, 2
        cnt = torch.zeros(B, dtype=torch.int32, device=DEV)
        return ops.RolloutPlan(st, st.clone(), cnt, T=T, horizon=H, cyclical=True, **deal), st, cnt

    small, _, _ = plan_for(2000)
    resident = small.deal_info["resident"]
    assert resident >= 8 and small.deal == "plain" and not small.deal_info["xcc"]
    assert small.deal_info["grid"] == small.deal_info["tiles"] == 8
    assert plan_for(2000, deal="xcc")[0].deal == "xcc"  # forced at any B
    at, _, _ = plan_for(resident * 256)
    assert at.deal == "plain" and at.deal_info["tiles"] == resident
    B = resident * 256 + 1
    above, st_x, cnt_x = plan_for(B)
    info = above.deal_info
    assert above.deal == "xcc" and info["xcc"] and info["tiles"] == resident + 1
    assert sum(info["quotas"]) == info["tiles"] <= info["grid"] and info["grid"] % 8 == 0
    assert plan_for(B, T=32)[0].deal == "plain"  # launches that read int32 ids keep the plain deal
    plain, st_p, cnt_p = plan_for(B, deal="plain")
    assert plain.deal == "plain"
    acts = torch.randint(0, 12, (T, B), dtype=torch.int32, device=DEV, generator=torch.Generator(DEV).manual_seed(0))
    above(acts)
    plain(acts)
    torch.cuda.synchronize()
    assert torch.equal(st_x, st_p) and torch.equal(cnt_x, cnt_p)
    # T is no multiple of the horizon: an env that was stepped shows it in its count
    assert int((cnt_p > 0).sum()) > B // 2
