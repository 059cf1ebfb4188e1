"""GPU: every instantiation of the env-side kernels at the relator lengths where a runtime-L
kernel is most likely to be wrong, bit-exact against the C oracle (oracle/oracle.py, pinned to the
reference's fixtures by tests/test_oracle.py).  Reads no golden file.

acx_launch.h::dispatch picks one of twelve instantiations by L: <3,36,4> at L = 36, <8,128,4> at
L = 128, else a runtime-L GenericTile set <NW,0,VEC> with NW = 1, 2, 3, 4, 8 for L <= 16, 32, 48,
64, else (nw_for) and VEC = 4 for even L, 2 for odd L.  MATRIX_L reaches all ten generic sets:

    L     1      15     16     17     32     33     40     48     49     64     65     126    127
    set <1,0,2><1,0,2><1,0,4><2,0,2><2,0,4><3,0,2><3,0,4><3,0,4><4,0,2><4,0,4><8,0,2><8,0,4><8,0,2>

16, 32, 48 and 64 are full tiles (16 NW letters), 17, 33, 49 and 65 the first L of a class, 127 the
last generic L and 126 the last even one (65 and 127 are both odd: without it no walk would run
<8,0,4>); tests/test_instantiation_matrix.py checks the list against the thresholds in the sources.
36 and 128 have suites of their own.

Shapes: B = 323 envs (two blocks, a partial last wave), horizon 5 with step_count[i] = i mod 5 (a
scattered subset of every wave resets on every step), T = 16 per-call steps, T = 19 rollout steps
(more than two packed action words, not a multiple of 8).  matrix_rows cycles five kinds of starting
row through each wave (both relators full, L - 1 letters, trivial, r1 = r0^-1, random reduced) and
matrix_actions plants move ids 12, -1 and 255.  Every walk is replayed by oracle_walk -- the oracle's
ACMove under acx's error contract (conftest.env_step_contract) -- and assert_not_vacuous holds that
replay, not the kernel's output, to: more resets than envs, a done, 5 % of (row, step) pairs with a
relator of exactly L letters, B moves that leave their row as it is with err 0 (the result would
exceed L), and both err 1 and err 4.  assert_walk_equal is the one comparison of a kernel's walk
with the oracle's (its own test: tests/test_instantiation_matrix.py).
"""
import numpy as np
import pytest
import torch

from conftest import env_step_contract, in_packed_domain, unpack_keys_np

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")

MATRIX_L = [1, 15, 16, 17, 32, 33, 40, 48, 49, 64, 65, 126, 127]
B_MATRIX = 64 * 5 + 3
H_MATRIX = 5
T_STEP = 16
T_ROLLOUT = 19
BAD_IDS = (12, -1, 255)

_TRIVIAL = [(1, 2), (1, -2), (-1, 2), (-1, -2), (2, 1), (2, -1), (-2, 1), (-2, -1)]


# ---------------------------------------------------------------------------------------------
# rows, move ids, the oracle's replay and the comparison (numpy only)
# ---------------------------------------------------------------------------------------------
def _reduced_words(rng, count, n):
    """(count, n) freely reduced random words over x, y (every prefix is freely reduced too)"""
    idx = np.empty((count, n), np.int64)
    idx[:, 0] = rng.integers(4, size=count)
    for k in range(1, n):  # any letter but the inverse ((i + 2) % 4) of the one before
        idx[:, k] = (idx[:, k - 1] + 3 + rng.integers(3, size=count)) % 4
    return np.array([1, 2, -1, -2], np.int32)[idx]


def matrix_rows(L, B, rng):
    """(B, 2L) starting rows, five kinds cycled through every wave (row b is kind b mod 5): both
    relators exactly L letters; L - 1 letters (one at L = 1); a trivial row [x^+-1], [y^+-1] in
    either order; r1 = r0^-1 (a concatenation empties a relator: err 1); freely reduced random
    relators of random lengths.  Every row is a valid presentation inside the packed domain."""
    words = _reduced_words(rng, 2 * B, L).reshape(B, 2, L)
    s = np.zeros((B, 2 * L), np.int32)
    for b in range(B):
        kind = b % 5
        if kind == 2:
            s[b, 0], s[b, L] = _TRIVIAL[(b // 5) % 8]
            continue
        if kind == 0:
            n0 = n1 = L
        elif kind == 1:
            n0 = n1 = max(1, L - 1)
        else:
            n0, n1 = int(rng.integers(1, L + 1)), int(rng.integers(1, L + 1))
        s[b, :n0] = words[b, 0, :n0]
        if kind == 3:
            s[b, L:L + n0] = -words[b, 0, :n0][::-1]
        else:
            s[b, L:L + n1] = words[b, 1, :n1]
    return s


def matrix_actions(T, B, rng):
    """(T, B) int32 move ids in [0,12) with a few outside planted (12, -1, 255: err 4)"""
    a = rng.integers(0, 12, size=(T, B)).astype(np.int32)
    for k, bad in enumerate(BAD_IDS):
        a[1 + k::5, 11 + 18 * k::64] = bad
    return a


def oracle_walk(starts, count0, acts, L, H, cyc, resets=None):
    """T env steps of the oracle's ACMove under acx's error contract with same-step autoreset to
    `resets` (default: the starting rows).  Per step t: state / count (after the step), reward,
    done, trunc, err, err_count (envs with err != 0 in steps 0..t), final_obs (every env's state
    before its reset), lengths (the rows' non-zero counts), unchanged (the move succeeded and left
    the row as it was)."""
    from oracle import oracle as O
    resets = starts if resets is None else resets
    T, B = acts.shape
    st, cnt = starts.copy(), count0.copy()
    keys = ("state", "reward", "done", "trunc", "count", "err", "final_obs", "lengths", "unchanged")
    w = {k: [] for k in keys}
    for t in range(T):
        before = st.copy()
        moved, _, merr = O.move_batch(before, acts[t], L, cyc)
        moves = in_packed_domain(before, L) & (merr == 0)
        fin = before.copy()
        fin[moves] = moved[moves]
        r, d, tr, e = env_step_contract(st, acts[t], cnt, resets, L, H, cyc)
        lens = np.stack([np.count_nonzero(st[:, :L], 1), np.count_nonzero(st[:, L:], 1)], 1).astype(np.int32)
        for k, v in zip(keys, (st.copy(), r, d, tr, cnt.copy(), e, fin, lens, moves & (fin == before).all(1))):
            w[k].append(v)
    w = {k: np.stack(v) for k, v in w.items()}
    w["err_count"] = np.cumsum((w["err"] != 0).sum(1)).astype(np.int32)
    return w


def walk_stats(w, L):
    n = np.stack([np.count_nonzero(w["state"][:, :, :L], 2), np.count_nonzero(w["state"][:, :, L:], 2)], 2)
    return {"resets": int((w["done"] | w["trunc"]).sum()), "dones": int(w["done"].sum()),
            "full": float((n == L).any(2).mean()), "unchanged": int(w["unchanged"].sum()),
            "errs": set(np.unique(w["err"]).tolist())}


def assert_not_vacuous(w, L, errs=(1, 4)):
    """conditions on the oracle's replay alone"""
    B = w["state"].shape[1]
    s = walk_stats(w, L)
    assert s["resets"] > B, s
    assert s["dones"] >= 1, s
    assert s["full"] >= 0.05, s
    assert s["unchanged"] >= B, s
    assert set(errs) <= s["errs"], s
    return s


def _same(name, got, want, where):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, (where, name, got.shape, want.shape)
    if not np.array_equal(got, want):
        at = tuple(int(i[0]) for i in np.nonzero(got != want))
        raise AssertionError(f"{where}: {name} differs first at {at}: got {got[at]}, oracle {want[at]}")


def assert_walk_equal(got, want, L, where=""):
    """A kernel's walk against oracle_walk's, bit for bit: `got` holds (T, ...) arrays under
    oracle_walk's names; whatever it holds is compared.  state, reward, done, trunc, count, err
    and err_count everywhere; final_obs on the rows that reset (the kernels leave the others
    untouched); lengths on the rows inside the packed domain (an out-of-domain row's lengths differ
    by entry point, include/acx.h)."""
    for k in ("state", "reward", "done", "trunc", "count", "err", "err_count"):
        if k in got:
            _same(k, got[k], want[k], where)
    if "final_obs" in got:
        m = (want["done"] | want["trunc"]).astype(bool)
        assert got["final_obs"].shape == want["final_obs"].shape, (where, "final_obs")
        _same("final_obs (rows that reset)", got["final_obs"][m], want["final_obs"][m], where)
    if "lengths" in got:
        m = want["err"] != 3
        assert got["lengths"].shape == want["lengths"].shape, (where, "lengths")
        _same("lengths", got["lengths"][m], want["lengths"][m], where)


def matrix_case(L, cyc, T, seed=0):
    """the starting rows, initial step counts and move ids of one (L, cyclical) case"""
    rng = np.random.default_rng(1000 * L + 10 * cyc + seed)
    starts = matrix_rows(L, B_MATRIX, rng)
    count0 = (np.arange(B_MATRIX) % H_MATRIX).astype(np.int32)
    return starts, count0, matrix_actions(T, B_MATRIX, rng)


# ---------------------------------------------------------------------------------------------
# GPU side
# ---------------------------------------------------------------------------------------------
def _t(x):
    return torch.as_tensor(np.ascontiguousarray(x)).to(DEV)


def _counts(rows, L):
    return np.stack([np.count_nonzero(rows[:, :L], 1), np.count_nonzero(rows[:, L:], 1)], 1).astype(np.int32)


def _step_walk(kind, starts, resets, count0, acts, L, H, cyc, lens0=None):
    """T calls of one per-call step entry on buffers of its own: kind "out" (acx_step into a fresh
    buffer filled with -7), "in" (acx_step in place), "lengths" / "reduced" (acx_step_lengths /
    acx_step_lengths_reduced, the lengths -- and flags -- carried from call to call, starting from
    lens0).  Returns the walk under oracle_walk's names and, for "reduced", each step's flags."""
    from acx import _lib
    lib = _lib.load()
    T, B = acts.shape
    st, rs, cnt = _t(starts), _t(resets), _t(count0)
    rew = torch.zeros(B, dtype=torch.int32, device=DEV)
    dn = torch.zeros(B, dtype=torch.uint8, device=DEV)
    tr = torch.zeros(B, dtype=torch.uint8, device=DEV)
    fo = torch.full((B, 2 * L), -7, dtype=torch.int32, device=DEV)
    err = torch.zeros(B, dtype=torch.uint8, device=DEV)
    ec = torch.zeros(1, dtype=torch.int32, device=DEV)
    lens = torch.zeros((B, 2), dtype=torch.int32, device=DEV) if lens0 is None else _t(lens0)
    red = torch.zeros(B, dtype=torch.uint8, device=DEV)
    stream = torch.cuda.current_stream(DEV).cuda_stream
    P = lambda x: x.data_ptr()  # noqa: E731
    names = ("state", "reward", "done", "trunc", "count", "err", "err_count", "final_obs", "lengths")
    got = {k: [] for k in names}
    flags = []
    for t in range(T):
        at = _t(acts[t])
        if kind in ("out", "in"):
            dst = st if kind == "in" else torch.full_like(st, -7)
            rc = lib.acx_step(P(st), P(dst), P(at), P(rs), P(cnt), P(rew), P(dn), P(tr), P(lens), P(fo), P(err), P(ec),
                              B, L, H, cyc, stream)
            st = dst
        elif kind == "lengths":
            rc = lib.acx_step_lengths(P(st), P(at), P(rs), P(cnt), P(rew), P(dn), P(tr), P(lens), P(fo), P(err), P(ec),
                                      B, L, H, cyc, stream)
        else:
            rc = lib.acx_step_lengths_reduced(P(st), P(at), P(rs), P(cnt), P(rew), P(dn), P(tr), P(lens), P(red), P(fo),
                                              P(err), P(ec), B, L, H, cyc, stream)
            flags.append(red.cpu().numpy().copy())
        assert rc == 0, (kind, t, rc)
        for k, x in zip(names, (st, rew, dn, tr, cnt, err, ec, fo, lens)):
            got[k].append(x.cpu().numpy().copy())
    got = {k: np.stack(v) for k, v in got.items()}
    got["err_count"] = got["err_count"].reshape(T)
    return got, flags


def _check_flags(flags, states, L, where):
    from test_gpu_step_lengths import _check_reduced_flags
    return sum(_check_reduced_flags(torch.as_tensor(f), states[t], L, (where, t)) for t, f in enumerate(flags))


@pytest.mark.parametrize("L", MATRIX_L)
@pytest.mark.parametrize("cyc", [1, 0])
def test_step_three_ways_vs_oracle(L, cyc):
    """acx_step out of place, acx_step in place, and acx_step_lengths / acx_step_lengths_reduced in
    place (lengths carried, every 13th row starting at (L, L): "read the whole row") over one walk:
    state, reward, done, truncated, step count, err, err_count, final_obs on the rows that reset and
    lengths_out / the carried lengths (= the rows' letter counts), every env and step against the
    oracle; the reduced flags claim only what holds (_check_reduced_flags)."""
    starts, count0, acts = matrix_case(L, cyc, T_STEP)
    want = oracle_walk(starts, count0, acts, L, H_MATRIX, cyc)
    assert_not_vacuous(want, L)
    lens0 = _counts(starts, L)
    lens0[::13] = L
    for kind in ("out", "in", "lengths", "reduced"):
        got, flags = _step_walk(kind, starts, starts, count0, acts, L, H_MATRIX, cyc,
                                lens0 if kind in ("lengths", "reduced") else None)
        assert_walk_equal(got, want, L, where=f"L={L} cyc={cyc} {kind}")
        if kind == "reduced":
            assert _check_flags(flags, want["state"], L, f"L={L} cyc={cyc}") > 0


@pytest.mark.parametrize("L", [16, 33, 48, 49, 65, 127])
def test_error_stream_vs_oracle(L):
    """test_gpu_rollout_errors._error_stream -- on top of the matrix's err 1 and err 4: conjugation
    of an emptied relator (err 2), out-of-domain input rows and starting rows (err 3) -- through
    acx_step in place and both lengths-carrying steps (lengths as VecACEnv computes them,
    _row_extent), against the oracle contract; an out-of-domain row's carried lengths are (L, L)."""
    from acx.envs.ac_env import _row_extent
    from test_gpu_rollout_errors import _error_stream
    B, T, H = B_MATRIX, T_STEP, H_MATRIX
    st0, resets, count0, acts, _, bad_in, bad_rs = _error_stream(L, B, T, H, seed=L + 7)
    want = oracle_walk(st0, count0, acts, L, H, 1, resets=resets)
    assert {1, 2, 3, 4} <= set(np.unique(want["err"]).tolist())
    assert (want["err"][:, bad_in] == 3).all() and (want["err"][-1, bad_rs] != 0).all()
    lens0 = _row_extent(_t(st0), L).cpu().numpy()
    for kind in ("in", "lengths", "reduced"):
        got, flags = _step_walk(kind, st0, resets, count0, acts, L, H, 1, None if kind == "in" else lens0)
        assert_walk_equal(got, want, L, where=f"L={L} errors {kind}")
        if kind != "in":
            assert (got["lengths"][want["err"] == 3] == L).all(), kind
        if kind == "reduced":
            _check_flags(flags, want["state"], L, f"L={L} errors")


LEARNER_L = [15, 16, 33, 48, 49, 64, 65, 127]


@pytest.mark.parametrize("L", LEARNER_L)
@pytest.mark.parametrize("cyc", [1, 0])
def test_step_learner_vs_oracle(L, cyc):
    """acx_step_learner (step_kernel<.., LEARN = true>: int64 move ids, float32 observation, reward
    and done) over the matrix walk against the oracle: the float outputs are the oracle's values
    converted, state, flags, step count, err, err_count and final_obs the oracle's."""
    from acx import _lib
    lib = _lib.load()
    starts, count0, acts = matrix_case(L, cyc, T_STEP)
    want = oracle_walk(starts, count0, acts, L, H_MATRIX, cyc)
    assert_not_vacuous(want, L)
    T, B = acts.shape
    st, rs, cnt = _t(starts), _t(starts), _t(count0)
    obs = torch.full((B, 2 * L), -7, dtype=torch.float32, device=DEV)
    rf = torch.zeros(B, dtype=torch.float32, device=DEV)
    df = torch.zeros(B, dtype=torch.float32, device=DEV)
    dn = torch.zeros(B, dtype=torch.uint8, device=DEV)
    tr = torch.zeros(B, dtype=torch.uint8, device=DEV)
    fo = torch.full((B, 2 * L), -7, dtype=torch.int32, device=DEV)
    err = torch.zeros(B, dtype=torch.uint8, device=DEV)
    ec = torch.zeros(1, dtype=torch.int32, device=DEV)
    stream = torch.cuda.current_stream(DEV).cuda_stream
    P = lambda x: x.data_ptr()  # noqa: E731
    names = ("state", "done", "trunc", "count", "err", "err_count", "final_obs", "obs", "rf", "df")
    got = {k: [] for k in names}
    for t in range(T):
        a64 = _t(acts[t].astype(np.int64))
        rc = lib.acx_step_learner(P(st), None, P(a64), P(rs), P(cnt), P(obs), P(rf), P(df), P(dn), P(tr), None, 0, None,
                                  0, None, P(fo), P(err), P(ec), B, L, H_MATRIX, cyc, stream)
        assert rc == 0, (t, rc)
        for k, x in zip(names, (st, dn, tr, cnt, err, ec, fo, obs, rf, df)):
            got[k].append(x.cpu().numpy().copy())
    got = {k: np.stack(v) for k, v in got.items()}
    got["err_count"] = got["err_count"].reshape(T)
    floats = {k: got.pop(k) for k in ("obs", "rf", "df")}
    assert_walk_equal(got, want, L, where=f"L={L} cyc={cyc} learner")
    assert floats["obs"].dtype == np.float32
    _same("obs_f32", floats["obs"], want["state"].astype(np.float32), L)
    _same("reward_f32", floats["rf"], want["reward"].astype(np.float32), L)
    _same("done_f32", floats["df"], want["done"].astype(np.float32), L)


@pytest.mark.parametrize("L", LEARNER_L)
def test_fused_learner_step_equals_two_calls_matrix(L):
    """LearnerEnv.step(fused=True) (acx_learner_step: one launch) against fused=False
    (acx_step_learner + acx_curriculum_assign) over one curriculum round, as
    test_gpu_learner.test_fused_learner_step_equals_two_calls, on the matrix's rows."""
    from acx.agents import LearnerEnv
    B, H = B_MATRIX, 3
    N = 2 * B + 5
    init = matrix_rows(L, N, np.random.default_rng(L))
    init[3] = 0
    init[3, 0], init[3, L], init[3, L + 1] = 1, 2, 1  # solves in one move: done events
    ea = LearnerEnv(init, B, horizon_length=H, device=DEV)
    eb = LearnerEnv(init, B, horizon_length=H, device=DEV)
    T = 3 * H + 2 * (N - B) // max(1, B // H) + 4
    g = torch.Generator(device=DEV)
    g.manual_seed(L + B)
    outs = [[torch.empty((B, 2 * L), dtype=torch.float32, device=DEV), torch.empty(B, dtype=torch.float32, device=DEV),
             torch.empty(B, dtype=torch.float32, device=DEV)] for _ in range(2)]
    hosted = n_done = 0
    for t in range(T):
        a = torch.randint(0, 12, (B,), dtype=torch.int64, device=DEV, generator=g)
        ra = ea.step(a, *outs[0], fused=True)
        rb = eb.step(a, *outs[1], fused=False)
        for x, y in zip(ra, rb):
            assert torch.equal(x, y), t
        for x, y in zip(outs[0], outs[1]):
            assert torch.equal(x, y), t
        assert torch.equal(ea.state, eb.state) and torch.equal(ea.vec.reset_state, eb.vec.reset_state), t
        assert torch.equal(ea.vec.step_count, eb.vec.step_count) and torch.equal(ea.vec.err, eb.vec.err), t
        assert torch.equal(ea.curr_index, eb.curr_index) and torch.equal(ea.next_index, eb.next_index), t
        n_done += int(ra[0].sum())
        nh = ra[3].cpu().numpy().nonzero()[0]
        for i in nh[:20]:
            ea.place(int(i), int(i) % N, obs_out=outs[0][0])
            eb.place(int(i), int(i) % N, obs_out=outs[1][0])
        for i in nh[20:]:
            ea.needs_host[int(i)] = 0
            eb.needs_host[int(i)] = 0
        hosted += len(nh)
    assert int(ea.next_index.item()) == N and hosted > 0 and n_done > 0


def _roll(starts, count0, acts, L, H, cyc, pack, obs_dtype):
    from acx import ops
    T, B = acts.shape
    st, rs, cnt = _t(starts), _t(starts), _t(count0)
    obs = None if obs_dtype is None else torch.full((T, B, 2 * L), -7, dtype=obs_dtype, device=DEV)
    rew = torch.zeros((T, B), dtype=torch.int32, device=DEV)
    dn = torch.zeros((T, B), dtype=torch.uint8, device=DEV)
    tr = torch.zeros((T, B), dtype=torch.uint8, device=DEV)
    err = torch.zeros(B, dtype=torch.uint8, device=DEV)
    ec = torch.zeros(1, dtype=torch.int32, device=DEV)
    ops.rollout(st, _t(acts), rs, cnt, horizon=H, cyclical=bool(cyc), obs_traj=obs, reward_traj=rew, done_traj=dn,
                trunc_traj=tr, err=err, err_count=ec, pack_actions=pack)
    r = {"state": st, "count": cnt, "reward": rew, "done": dn, "trunc": tr, "err": err, "err_count": ec}
    if obs is not None:
        r["obs"] = obs
    return {k: v.cpu().numpy() for k, v in r.items()}


@pytest.mark.parametrize("L", MATRIX_L)
@pytest.mark.parametrize("cyc", [1, 0])
def test_rollout_vs_oracle(L, cyc):
    """ops.rollout with no observation trajectory, an int32 one and an int8 one (rollout_kernel's
    OBS = 0, 1, 2), each with the int32 move ids and the packed ones (acx_rollout /
    acx_rollout_obs8 / acx_rollout_packed), T = 19: every step's observation, reward, done and
    truncated, the final state and step count, err (each env's first error) and err_count against the
    oracle's replay -- env_step_contract, as the planted err 1 / err 4 moves keep the step count,
    which O.env_step's loop (test_desynchronised_resets_equal_oracle) does not model; the int8
    trajectory is the int32 one cast, the packed path equals the unpacked one."""
    starts, count0, acts = matrix_case(L, cyc, T_ROLLOUT, seed=1)
    want = oracle_walk(starts, count0, acts, L, H_MATRIX, cyc)
    assert_not_vacuous(want, L)
    first_err = np.zeros(B_MATRIX, np.uint8)
    for e in want["err"]:
        first_err = np.where(first_err == 0, e, first_err)
    runs = {}
    for obs_dtype in (None, torch.int32, torch.int8):
        for pack in (False, True):
            g = runs[obs_dtype, pack] = _roll(starts, count0, acts, L, H_MATRIX, cyc, pack, obs_dtype)
            where = f"L={L} cyc={cyc} obs={obs_dtype} pack={pack}"
            traj = {k: g[k] for k in ("reward", "done", "trunc")}
            if obs_dtype == torch.int32:
                traj["state"] = g["obs"]
            assert_walk_equal(traj, want, L, where=where)
            _same("final state", g["state"], want["state"][-1], where)
            _same("final count", g["count"], want["count"][-1], where)
            _same("err", g["err"], first_err, where)
            assert int(g["err_count"][0]) == int((first_err != 0).sum()), where
    for pack in (False, True):
        _same("int8 obs", runs[torch.int8, pack]["obs"], runs[torch.int32, pack]["obs"].astype(np.int8), pack)
    for obs_dtype in (None, torch.int32, torch.int8):
        a, b = runs[obs_dtype, False], runs[obs_dtype, True]
        for k in a:
            _same(f"packed vs unpacked {k}", b[k], a[k], obs_dtype)


# ---------------------------------------------------------------------------------------------
# the search family: expand12 (four kernels), unpack_keys, canonicalize
# ---------------------------------------------------------------------------------------------
SEARCH_L = MATRIX_L + [76, 77, 100, 101]


def _search_parents(L, cyc):
    """N = 133 parents (two tiles and a partial one): random letters, unreduced; every 7th row both
    relators exactly L letters, reduced; and the six planted x y x y .. rows of
    test_gpu_parity.test_expand12_keys_only_equals_keys_of_children (r1 = r0^-1: two of their
    children empty a relator, err 1)"""
    rng = np.random.default_rng(2000 + 10 * L + cyc)
    N = 133
    s = np.zeros((N, 2 * L), np.int32)
    for b in range(N):
        for h in range(2):
            n = int(rng.integers(1, L + 1))
            s[b, h * L:h * L + n] = rng.choice([1, -1, 2, -2], size=n)
    full = _reduced_words(rng, 2 * N, L).reshape(N, 2 * L)
    for w in full.reshape(2 * N, L):  # cyclically reduced as well: ACMove leaves such a relator as it is
        if L > 1 and w[-1] == -w[0]:
            w[-1] = next(x for x in (1, 2, -1, -2) if x != -w[0] and x != -w[-2])
    s[::7] = full[::7]  # 19 parents with both relators exactly L letters
    xy = np.tile(np.array([1, 2], np.int32), L)[:L]
    for row, n in zip((3, 63, 64, 100, 127, 132), (1, 2, L // 2, L - 1, L, 3)):
        n = min(max(n, 1), L)
        s[row] = 0
        s[row, :n] = xy[:n]
        s[row, L:L + n] = -xy[:n][::-1]
    return s


@pytest.mark.parametrize("L", SEARCH_L)
@pytest.mark.parametrize("cyc", [0, 1])
def test_search_family_vs_oracle(L, cyc):
    """expand12 with children and keys, keys only and children only against O.expand12; the 0xFFFF
    length bytes of an errored child's key; unpack_keys(lengths=True) of the good keys = the
    children and their lengths = conftest.unpack_keys_np; canonicalize in place and out of place
    against O.simplify_presentation, rows with an empty relator (err 1) and rows outside the domain
    (err 3, kept exactly) included.  Every call returns ACX_OK (ops raises otherwise).

    Which expand12 kernel a call launches (launch_expand in acx_launch.h; the rows kernel needs a
    compile-time L, so no L here takes it).  With WAVE = 64 and WPB = 4, GenericTile<NW,0,VEC> has
    row_bytes(L) = (((L + 16 NW + 3) >> 2) | 1) * 4 and wave_bytes(L) = 64 row_bytes(L) + 64.
      with children: expand12_children_kernel while ExpandChildrenSmem::bytes = 4 * align16(
        wave_bytes) + 64*12*2*4 + 64*12 = 4 * align16(wave_bytes) + 6912 <= 65536, i.e. wave_bytes
        <= 14656, row_bytes <= 228.  At NW = 8: (L + 131) >> 2 is 56 or 57 for L = 93..100, both
        | 1 = 57, row_bytes 228, and the launch asks for exactly 65,536 bytes of dynamic LDS (it
        succeeds on an MI355X: the L = 100 cases here make it); at
        L = 101 it is 58 | 1 = 59, row_bytes 236, 67,584 bytes: expand12_kernel.  NW <= 4 (L <= 64)
        never comes near (at most 4 * 8,512 + 6,912 = 40,960 at L = 64).  So children at L <= 100, expand12_kernel at 101,
        126 and 127.
      keys only: expand12_keys_kernel while ExpandKeysSmem::bytes = max(wave_bytes, 64*12*8*kw)
        + 64 * (2 NW + 2) * 4 <= 40960, kw = ceil((4L + 16) / 64).  At NW = 8 the second term is
        4,608 and 6,144 kw <= 36,352 means kw <= 5, i.e. 4L + 16 <= 320, L <= 76 (35,328 bytes);
        L = 77 has kw = 6 (41,472 bytes): expand12_kernel and its staged key groups.  NW <= 4 has
        kw <= 5.  So keys kernel at L <= 76, expand12_kernel at 77, 100, 101, 126 and 127.
    """
    import acx
    from oracle import oracle as O
    s = _search_parents(L, cyc)
    N = s.shape[0]
    ch, lens, err = O.expand12(s, L, cyc)
    bad = err != 0
    ok = ~bad
    assert bad.sum() >= 12 and ok.mean() > 0.5  # errored children, and mostly good ones
    # children with r0 exactly L letters: 18 full reduced parents x the 6 moves that leave r0 alone
    assert (np.count_nonzero(ch[ok][:, :L], 1) == L).sum() >= 100
    par = _t(s)
    both = acx.ops.expand12(par, cyclical=bool(cyc), children=True, keys=True)
    konly = acx.ops.expand12(par, cyclical=bool(cyc), children=False, keys=True, lengths=True, err=True)
    conly = acx.ops.expand12(par, cyclical=bool(cyc), children=True, keys=False)
    assert "children" not in konly and "keys" not in conly
    where = f"L={L} cyc={cyc}"
    for name, res in (("children+keys", both), ("keys only", konly), ("children only", conly)):
        _same(f"{name}: err", res["err"].cpu().numpy(), err, where)
        _same(f"{name}: lengths", res["lengths"].cpu().numpy()[ok], lens[ok], where)
        if "children" in res:
            _same(f"{name}: children", res["children"].cpu().numpy(), ch, where)
    k_both = both["keys"].cpu().numpy().view(np.uint64)
    k_only = konly["keys"].cpu().numpy().view(np.uint64)
    _same("keys of the good children", k_only[ok], k_both[ok], where)
    from test_gpu_parity import _key_length_bytes
    assert (_key_length_bytes(k_both, L)[bad] == 0xFFFF).all(), where
    assert (_key_length_bytes(k_only, L)[bad] == 0xFFFF).all(), where
    okt = _t(ok)
    for keys in (both["keys"], konly["keys"]):
        back, blen = acx.ops.unpack_keys(keys[okt], L, lengths=True)
        _same("unpack_keys", back.cpu().numpy(), ch[ok], where)
        _same("unpack_keys lengths", blen.cpu().numpy(), lens[ok], where)
    _same("unpack_keys_np", unpack_keys_np(k_only[ok], L).astype(np.int32), ch[ok], where)

    # canonicalize: the parents plus rows with an empty relator and rows outside the domain
    c = s.copy()
    empty = np.arange(5, N, 23)
    c[empty[::2], :L] = 0
    c[empty[1::2], L:] = 0
    ood = np.arange(9, N, 29)
    c[ood[::2], 0] = 3
    if L > 2:
        c[ood[1::2], L:L + 3] = (1, 0, 2)  # a zero inside r1
    else:
        c[ood[1::2], L] = -7
    exp = [O.simplify_presentation(c[b], L, cyc) for b in range(N)]
    e_want = np.array([e for _, _, e in exp], np.uint8)
    dom = in_packed_domain(c, L)
    e_want[~dom] = 3
    assert (e_want[empty] == 1).all() and (e_want[ood] == 3).all() and (e_want == 0).sum() > N // 2
    good = e_want == 0
    s_want = np.stack([x for x, _, _ in exp])
    l_want = np.array([x for _, x, _ in exp], np.int32)
    src = _t(c)
    out, ln, er = acx.ops.canonicalize(src, cyclical=bool(cyc))
    assert torch.equal(src, _t(c))  # the out-of-place call leaves its input alone
    inp = _t(c)
    out2, ln2, er2 = acx.ops.canonicalize(inp, cyclical=bool(cyc), out=inp)
    assert out2.data_ptr() == inp.data_ptr()
    for name, (o, l_, e) in (("out of place", (out, ln, er)), ("in place", (out2, ln2, er2))):
        o, l_, e = o.cpu().numpy(), l_.cpu().numpy(), e.cpu().numpy()
        _same(f"canonicalize {name}: err", e, e_want, where)
        _same(f"canonicalize {name}: rows", o[good], s_want[good], where)
        _same(f"canonicalize {name}: lengths", l_[good], l_want[good], where)
        _same(f"canonicalize {name}: failed rows kept", o[~good], c[~good], where)  # include/acx.h


@pytest.mark.parametrize("L", [15, 31, 47, 49, 63, 64])
@pytest.mark.parametrize("cyc", [0, 1])
def test_features_and_token_ids_of_expand12_keys(L, cyc):
    """ops.features(keys=) / ops.token_ids(keys=) on expand12's packed keys against the oracle's
    compute_features_batch / token_ids of the oracle's children, bit for bit (as
    test_gpu_features.test_features_of_expand12_keys_equal_features_of_children).  49, 63 and 64 are
    features_keys_kernel<4>; at 15, 31, 47 and 63 the key's two length bytes (bits 4L .. 4L + 15)
    lie across a 64-bit word boundary."""
    import acx
    from oracle import features as F
    from oracle import oracle as O
    assert (4 * L) // 64 != (4 * L + 15) // 64 or L in (49, 64)
    P = matrix_rows(L, B_MATRIX, np.random.default_rng(3000 + L))
    res = acx.ops.expand12(_t(P), cyclical=bool(cyc), children=False, keys=True)
    ch, _, err = O.expand12(P, L, cyc)
    ok = err.reshape(-1) == 0
    kids = ch.reshape(-1, 2 * L)[ok]
    assert (~ok).sum() > 0 and (np.count_nonzero(kids[:, :L], 1) == L).sum() > 0
    _same("expand12 err", res["err"].cpu().numpy(), err, L)
    f = acx.ops.features(keys=res["keys"], L=L).cpu().numpy()[ok]
    exp = F.compute_features_batch(kids, L)
    _same("features", np.asarray(f, np.float32).view(np.uint32), np.asarray(exp, np.float32).view(np.uint32), L)
    for D in (2 * L, 2 * L + 5):
        t = acx.ops.token_ids(keys=res["keys"], L=L, max_state_dim=D).cpu().numpy()[ok]
        _same(f"token_ids D={D}", t, F.token_ids(kids, D), L)
