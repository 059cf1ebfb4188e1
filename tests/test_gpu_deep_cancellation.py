"""GPU: every kernel's word algebra on rows with a cancellation of a chosen depth planted in them
(tests/planted_rows.py, checked on the CPU by tests/test_planted_rows.py), bit-exact against the C
oracle.  Reads no golden file.

Every kernel finds a concatenation's junction cancellation count, and the cyclic peel after it, as
the first set bit of a mismatch mask spread over several machine words -- 32-bit words of 16 letters
(acx_moves.h wfirst / wshr / wshl / wrev: expand12, the search engines, canonicalize, the key
readers), 64-bit plane words of 64 letters (acx_planes.h bfirst / noncancel / prev: step,
step-lengths, rollout, learner, the two-lane pair kernel), int32 letters (acx_words.hip) -- and then
splices with multi-word shifts.  Random rows reach a depth d with probability 3^-d; the planted
rows have junction depth k and peel depth m in {0, 1, 16j - 1, 16j, 16j + 1, L - 2}, the length
gate's edges (product of exactly L, L + 1, L + 2 letters; fits only after the cancellation; fits
only after the peel -- a no-op, the gate comes first), unclean twins (one more cancelling pair:
the general ac_move and not ac_move_clean) and nested unreduced relators.

PLANTED_L: 17, 33, 49 and 65 are the first L of a packed-word class, 32, 48 and 64 full tiles, 36
and 128 the compile-time tiles, 65 / 100 / 127 / 128 two plane words; 100, 127 and 128 take
expand12_kernel, 65 the children and keys kernels (test_gpu_instantiations).
"""
import collections
import functools
import heapq

import numpy as np
import pytest
import torch

import planted_rows as P
import test_gpu_instantiations as M
from conftest import unpack_keys_np

# the shared planted sets are read-only arrays; copying them to the device writes nothing to them
pytestmark = [pytest.mark.gpu, pytest.mark.filterwarnings("ignore:The given NumPy array is not writable")]

DEV = M.DEV
H = 5
UNDO = np.array([2, 3, 0, 1], np.int32)  # the concatenation that appends the inverse of what id a appended


@functools.lru_cache(maxsize=None)
def planted(L):
    """base: the junction and gate rows with their move ids; twins: their unclean twins; nested"""
    base = P.concat_sets([P.junction_rows(L)] + list(P.gate_rows(L).values()))
    sets = {"base": base, "twins": P.unclean_twin(base, L), "nested": P.nested_rows(L)}
    for s in sets.values():
        for v in s.values():
            v.setflags(write=False)
    return sets


def _own(L):
    """the planted rows and twins, each with its own move id"""
    s = planted(L)
    return np.concatenate([s["base"]["rows"], s["twins"]["rows"]]), np.concatenate([s["base"]["ids"], s["twins"]["ids"]])


def _partial_wave(n):
    """rows to repeat so that the last wave of 64 is partial"""
    return n + (37 - n) % 64


@functools.lru_cache(maxsize=None)
def step_case(L, cyc):
    """(starts, count0, acts (2, B), oracle walk).  Rows: the planted rows and twins with their own
    id, then every one of them under each of the 12 ids; B padded to a partial last wave.  Step 1:
    for the first block the undo of step 0 (the product loses what it gained: a second deep
    junction, on the kernels' clean / known-reduced path), seeded random ids for the rest."""
    rows, ids = _own(L)
    n = len(rows)
    starts = np.concatenate([rows, np.repeat(rows, 12, 0)])
    a0 = np.concatenate([ids, np.tile(np.arange(12, dtype=np.int32), n)])
    a1 = np.random.default_rng(L).integers(0, 12, size=len(a0)).astype(np.int32)
    a1[:n] = UNDO[ids]
    B = _partial_wave(len(starts))
    pick = np.arange(B) % len(starts)
    starts, acts = starts[pick], np.stack([a0[pick], a1[pick]])
    count0 = (np.arange(B) % H).astype(np.int32)
    want = M.oracle_walk(starts, count0, acts, L, H, cyc)
    assert (want["err"][0, :n] == 0).all()
    # the planted moves are applied (or gated) as constructed: conditions on the oracle alone
    ap = planted(L)["base"]["applies"]
    changed = (want["final_obs"][0, :len(ap)] != starts[:len(ap)]).any(1)
    assert np.array_equal(changed, ap)
    for v in (starts, count0, acts, *want.values()):
        v.setflags(write=False)
    return starts, count0, acts, want


def _learner_walk(starts, count0, acts, L, cyc):
    """acx_step_learner over the walk, as test_gpu_instantiations.test_step_learner_vs_oracle"""
    from acx import _lib
    lib = _lib.load()
    T, B = acts.shape
    st, rs, cnt = M._t(starts), M._t(starts), M._t(count0)
    obs = torch.full((B, 2 * L), -7, dtype=torch.float32, device=DEV)
    rf, df = (torch.zeros(B, dtype=torch.float32, device=DEV) for _ in range(2))
    dn, tr, err = (torch.zeros(B, dtype=torch.uint8, device=DEV) for _ in range(3))
    fo = torch.full((B, 2 * L), -7, dtype=torch.int32, device=DEV)
    ec = torch.zeros(1, dtype=torch.int32, device=DEV)
    stream = torch.cuda.current_stream(DEV).cuda_stream
    P_ = lambda x: x.data_ptr()  # noqa: E731
    names = ("state", "done", "trunc", "count", "err", "err_count", "final_obs", "obs", "rf", "df")
    got = {k: [] for k in names}
    for t in range(T):
        a64 = M._t(acts[t].astype(np.int64))
        rc = lib.acx_step_learner(P_(st), None, P_(a64), P_(rs), P_(cnt), P_(obs), P_(rf), P_(df), P_(dn), P_(tr), None, 0,
                                  None, 0, None, P_(fo), P_(err), P_(ec), B, L, H, cyc, stream)
        assert rc == 0, (t, rc)
        for k, x in zip(names, (st, dn, tr, cnt, err, ec, fo, obs, rf, df)):
            got[k].append(x.cpu().numpy().copy())
    got = {k: np.stack(v) for k, v in got.items()}
    got["err_count"] = got["err_count"].reshape(T)
    return got


@pytest.mark.parametrize("L", P.PLANTED_L)
@pytest.mark.parametrize("cyc", [1, 0])
def test_planted_step_vs_oracle(L, cyc):
    """acx_step out of place and in place, acx_step_lengths and acx_step_lengths_reduced (lengths
    carried, every 13th row starting at (L, L)) and acx_step_learner over step_case's two steps:
    everything assert_walk_equal compares, the reduced flags, the learner's float outputs."""
    starts, count0, acts, want = step_case(L, cyc)
    lens0 = M._counts(starts, L)
    lens0[::13] = L
    for kind in ("out", "in", "lengths", "reduced"):
        got, flags = M._step_walk(kind, starts, starts, count0, acts, L, H, cyc,
                                  lens0 if kind in ("lengths", "reduced") else None)
        M.assert_walk_equal(got, want, L, where=f"L={L} cyc={cyc} {kind}")
        if kind == "reduced":
            assert M._check_flags(flags, want["state"], L, f"L={L} cyc={cyc}") > 0
    got = _learner_walk(starts, count0, acts, L, cyc)
    floats = {k: got.pop(k) for k in ("obs", "rf", "df")}
    M.assert_walk_equal(got, want, L, where=f"L={L} cyc={cyc} learner")
    M._same("obs_f32", floats["obs"], want["state"].astype(np.float32), L)
    M._same("reward_f32", floats["rf"], want["reward"].astype(np.float32), L)
    M._same("done_f32", floats["df"], want["done"].astype(np.float32), L)


@pytest.mark.parametrize("cyc", [1, 0])
def test_planted_step_large_batch_L36(cyc):
    """At L = 36 acx_step runs step_pair_kernel up to SMALL_STEP_MAX_B envs (step_case's batch) and
    step_kernel<3,36,4> above: the planted rows and twins with their own ids, tiled past it.  The
    oracle's walk is computed once on the untiled rows and tiled (a row's step depends on nothing
    but the row)."""
    from acx import ops
    L = 36
    rows, ids = _own(L)
    n = len(rows)
    B = ops.SMALL_STEP_MAX_B + 64 * 3 + 5
    assert ops.step_kernel_name(B, L) != ops.step_kernel_name(n, L)
    count_n = (np.arange(n) % H).astype(np.int32)
    base = M.oracle_walk(rows, count_n, ids[None], L, H, cyc)
    pick = np.arange(B) % n
    want = {k: v[:, pick] for k, v in base.items() if k != "err_count"}
    want["err_count"] = np.cumsum((want["err"] != 0).sum(1)).astype(np.int32)
    for kind in ("out", "in"):
        got, _ = M._step_walk(kind, rows[pick], rows[pick], count_n[pick], ids[None][:, pick], L, H, cyc)
        M.assert_walk_equal(got, want, L, where=f"L=36 B={B} cyc={cyc} {kind}")


@pytest.mark.parametrize("L", P.PLANTED_L)
@pytest.mark.parametrize("cyc", [1, 0])
def test_planted_rollout_vs_oracle(L, cyc):
    """ops.rollout, T = 3: step 0 the planted id, step 1 its undo, step 2 seeded random; horizon 5
    with scattered step counts; no observation trajectory, int32 and int8, packed ids and not."""
    rows, ids = _own(L)
    B = _partial_wave(len(rows))
    pick = np.arange(B) % len(rows)
    starts = rows[pick]
    rng = np.random.default_rng(7 * L + cyc)
    acts = np.stack([ids[pick], UNDO[ids[pick]], rng.integers(0, 12, size=B).astype(np.int32)])
    acts[1, 1::3] = rng.integers(0, 12, size=len(acts[1, 1::3]))
    count0 = (np.arange(B) % H).astype(np.int32)
    want = M.oracle_walk(starts, count0, acts, L, H, cyc)
    first_err = np.zeros(B, np.uint8)
    for e in want["err"]:
        first_err = np.where(first_err == 0, e, first_err)
    runs = {}
    for obs_dtype in (None, torch.int32, torch.int8):
        for pack in (False, True):
            g = runs[obs_dtype, pack] = M._roll(starts, count0, acts, L, H, cyc, pack, obs_dtype)
            where = f"L={L} cyc={cyc} obs={obs_dtype} pack={pack}"
            traj = {k: g[k] for k in ("reward", "done", "trunc")}
            if obs_dtype == torch.int32:
                traj["state"] = g["obs"]
            M.assert_walk_equal(traj, want, L, where=where)
            M._same("final state", g["state"], want["state"][-1], where)
            M._same("final count", g["count"], want["count"][-1], where)
            M._same("err", g["err"], first_err, where)
            assert int(g["err_count"][0]) == int((first_err != 0).sum()), where
    for pack in (False, True):
        M._same("int8 obs", runs[torch.int8, pack]["obs"], want["state"].astype(np.int8), pack)


# ---------------------------------------------------------------------------------------------
# the search family
# ---------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def search_parents(L):
    s = planted(L)
    rows = np.concatenate([s["base"]["rows"], s["twins"]["rows"], s["nested"]["rows"]])
    rows.setflags(write=False)
    return rows


@pytest.mark.parametrize("L", P.PLANTED_L)
@pytest.mark.parametrize("cyc", [0, 1])
def test_planted_expand12_vs_oracle(L, cyc):
    """expand12 with children and keys, keys only and children only on the planted rows, their
    twins and the nested rows against O.expand12: children, lengths, err, keys (the two calls'
    agree; unpack_keys and conftest.unpack_keys_np give the children and lengths back)."""
    import acx
    from oracle import oracle as O
    s = search_parents(L)
    ch, lens, err = O.expand12(s, L, cyc)
    ok = err == 0
    b = planted(L)["base"]
    own = ch[np.arange(len(b["ids"])), b["ids"]]  # the planted id's child: the constructed result
    assert np.array_equal(own, b["want_cyc"] if cyc else b["want_flat"]) and ok.mean() > 0.9
    par = M._t(s)
    both = acx.ops.expand12(par, cyclical=bool(cyc), children=True, keys=True)
    konly = acx.ops.expand12(par, cyclical=bool(cyc), children=False, keys=True, lengths=True, err=True)
    conly = acx.ops.expand12(par, cyclical=bool(cyc), children=True, keys=False)
    where = f"L={L} cyc={cyc}"
    for name, res in (("children+keys", both), ("keys only", konly), ("children only", conly)):
        M._same(f"{name}: err", res["err"].cpu().numpy(), err, where)
        M._same(f"{name}: lengths", res["lengths"].cpu().numpy()[ok], lens[ok], where)
        if "children" in res:
            M._same(f"{name}: children", res["children"].cpu().numpy(), ch, where)
    k_both = both["keys"].cpu().numpy().view(np.uint64)
    k_only = konly["keys"].cpu().numpy().view(np.uint64)
    M._same("keys of the good children", k_only[ok], k_both[ok], where)
    M._same("unpack_keys_np", unpack_keys_np(k_only[ok], L).astype(np.int32), ch[ok], where)
    okt = M._t(ok)
    for keys in (both["keys"], konly["keys"]):
        back, blen = acx.ops.unpack_keys(keys[okt], L, lengths=True)
        M._same("unpack_keys", back.cpu().numpy(), ch[ok], where)
        M._same("unpack_keys lengths", blen.cpu().numpy(), lens[ok], where)


@pytest.mark.parametrize("L", P.PLANTED_L)
@pytest.mark.parametrize("cyc", [0, 1])
def test_planted_canonicalize_vs_oracle(L, cyc):
    """canonicalize in place and out of place against O.simplify_presentation on the nested rows
    (they reduce to their outer words, as constructed), the unclean twins, and the applied planted
    products p A B p^-1 -- freely reduced, so only the cyclic flag changes them: a peel of depth m"""
    import acx
    from oracle import oracle as O
    s = planted(L)
    b = s["base"]
    c = np.concatenate([s["nested"]["rows"], s["twins"]["rows"], b["want_flat"][b["applies"]]])
    exp = [O.simplify_presentation(r, L, cyc) for r in c]
    assert all(e == 0 for _, _, e in exp)
    s_want = np.stack([x for x, _, _ in exp])
    l_want = np.array([x for _, x, _ in exp], np.int32)
    n_unreduced = len(s["nested"]["rows"]) + len(s["twins"]["rows"])
    assert np.array_equal(s_want[:len(s["nested"]["rows"])], s["nested"]["want"])
    assert (s_want != c).any(1)[:n_unreduced].all()
    assert np.array_equal(s_want[n_unreduced:], (b["want_cyc"] if cyc else b["want_flat"])[b["applies"]])
    src = M._t(c)
    out, ln, er = acx.ops.canonicalize(src, cyclical=bool(cyc))
    assert torch.equal(src, M._t(c))
    inp = M._t(c)
    out2, ln2, er2 = acx.ops.canonicalize(inp, cyclical=bool(cyc), out=inp)
    assert out2.data_ptr() == inp.data_ptr()
    for name, (o, l_, e) in (("out of place", (out, ln, er)), ("in place", (out2, ln2, er2))):
        where = f"L={L} cyc={cyc} canonicalize {name}"
        M._same("err", e.cpu().numpy(), np.zeros(len(c), np.uint8), where)
        M._same("rows", o.cpu().numpy(), s_want, where)
        M._same("lengths", l_.cpu().numpy(), l_want, where)


@pytest.mark.parametrize("L", P.PLANTED_L)
@pytest.mark.parametrize("cyc", [0, 1])
def test_planted_features_and_token_ids_of_keys(L, cyc):
    """ops.features(keys=) / ops.token_ids(keys=) on expand12's keys of the planted rows' children
    against the oracle's features and token ids of the oracle's children, bit for bit"""
    import acx
    from oracle import features as F
    from oracle import oracle as O
    rows = planted(L)["base"]["rows"]
    res = acx.ops.expand12(M._t(rows), cyclical=bool(cyc), children=False, keys=True)
    ch, _, err = O.expand12(rows, L, cyc)
    ok = err.reshape(-1) == 0
    kids = ch.reshape(-1, 2 * L)[ok]
    M._same("expand12 err", res["err"].cpu().numpy(), err, L)
    f = acx.ops.features(keys=res["keys"], L=L).cpu().numpy()[ok]
    exp = F.compute_features_batch(kids, L)
    M._same("features", np.asarray(f, np.float32).view(np.uint32), np.asarray(exp, np.float32).view(np.uint32), L)
    for D in (2 * L, 2 * L + 5):
        t = acx.ops.token_ids(keys=res["keys"], L=L, max_state_dim=D).cpu().numpy()[ok]
        M._same(f"token_ids D={D}", t, F.token_ids(kids, D), L)


# ---------------------------------------------------------------------------------------------
# the int32-letter word kernels (acx_words.hip)
# ---------------------------------------------------------------------------------------------
def _generic(x):
    """letters +-1 -> +-3, +-2 -> +-5: the same structure outside the packed domain"""
    return (np.sign(x) * np.array([0, 3, 5])[np.abs(x)]).astype(np.int32)


@pytest.mark.parametrize("L", P.PLANTED_L)
@pytest.mark.parametrize("letters", ["packed", "generic"])
def test_planted_word_kernels_vs_oracle(L, letters):
    """ops.word_move (both flags), ops.concatenate (the four concatenations) and
    ops.word_simplify_relator (the raw products r_i r_j^sign, 2L letters with the planted junction
    and peel nested inside, and the nested relators; both flags, padded and not) on the planted
    rows, with letters +-1/+-2 and mapped to +-3/+-5"""
    from acx import ops
    from oracle import oracle as O
    rows, ids = _own(L)
    conv = _generic if letters == "generic" else (lambda x: x)
    rows = conv(rows)
    st = M._t(rows)
    where = f"L={L} {letters}"
    for cyc in (1, 0):
        out, lens, done, err = (x.cpu().numpy() for x in ops.word_move(st, M._t(ids), cyclical=bool(cyc)))
        o_want, l_want, e_want = O.move_batch(rows, ids, L, cyc)
        M._same(f"word_move cyc={cyc}: err", err, e_want, where)
        M._same(f"word_move cyc={cyc}: rows", out, o_want, where)
        M._same(f"word_move cyc={cyc}: lengths", lens, l_want, where)
        triv = np.array([l_want[b].sum() == 2 and O.is_trivial(o_want[b]) for b in range(len(rows))])
        M._same(f"word_move cyc={cyc}: done", done.astype(bool), triv & (e_want == 0), where)
    products = []
    for a, (i, sign) in P.CONCAT.items():
        out, _ = ops.concatenate(st, i, 1 - i, sign)
        out = out.cpu().numpy()
        sel = np.nonzero(ids == a)[0]
        want = np.stack([O.concatenate(rows[b], L, i, 1 - i, sign) for b in sel])
        M._same(f"concatenate id {a}", out[sel], want, where)
        for b in sel[::4]:  # the raw product, junction uncancelled
            r = P.relators(rows[b], L)
            w = r[1 - i] if sign == 1 else P.inv(r[1 - i])
            products.append(r[i] + w)
    nest = planted(L)["nested"]
    products += [P.relators(conv(r), L)[h] for r, h in zip(nest["rows"], nest["half"])]
    m = 2 * L
    rel = np.zeros((len(products), m), np.int32)
    for b, w in enumerate(products):
        rel[b, :len(w)] = w
    for cyc in (True, False):
        for padded in (True, False):
            out, ol, n, err = (x.cpu().numpy() for x in ops.word_simplify_relator(M._t(rel), m, cyclical=cyc, padded=padded))
            for b in range(len(rel)):
                o, nn, e = O.simplify_relator(rel[b], m, cyc, padded)
                assert err[b] == e == 0, (where, b)
                assert out[b, :ol[b]].tolist() == o.tolist() and n[b] == nn, (where, cyc, padded, b)


# ---------------------------------------------------------------------------------------------
# the search engines
# ---------------------------------------------------------------------------------------------
BUDGET = 200


def _oracle_search(start, L, cyc, budget, greedy):
    """breadth_first.py:15-97 / greedy.py:17-121 over O.expand12: (stored states in discovery order,
    popped indices, errs, found).  A child equal to a stored state -- a move that leaves its row as
    it is -- is a duplicate."""
    from oracle import oracle as O
    order = [start.astype(np.int8)]
    index = {order[0].tobytes(): 0}
    fifo = collections.deque([0])
    heap = [(int(np.count_nonzero(start)), 0, tuple(order[0].tolist()), 0)]
    popped, errs, found = [], 0, False
    while (heap if greedy else fifo) and not found:
        if greedy:
            _, depth, _, at = heapq.heappop(heap)
        else:
            at, depth = fifo.popleft(), 0
        popped.append(at)
        ch, lens, err = O.expand12(order[at].astype(np.int32)[None], L, cyc)
        for a in range(12):
            errs += int(err[0, a] != 0)
            found |= int(lens[0, a].sum()) == 2
            c = ch[0, a].astype(np.int8)
            if err[0, a] == 0 and c.tobytes() not in index:
                index[c.tobytes()] = len(order)
                order.append(c)
                fifo.append(len(order) - 1)
                heapq.heappush(heap, (int(lens[0, a].sum()), depth + 1, tuple(c.tolist()), len(order) - 1))
        if len(order) >= budget:
            break
    return np.stack(order), popped, errs, found


@functools.lru_cache(maxsize=None)
def search_starts(L, cyc):
    """three applied junction rows with k >= 16 whose searches (BFS and greedy, on the oracle alone)
    meet no err and no trivial state within the budget, with the oracle's BFS of each"""
    b = planted(L)["base"]
    cand = np.nonzero(b["applies"] & (b["k"] >= 16))[0]
    picked = []
    for n in cand[:: max(1, len(cand) // 12)]:
        start = b["rows"][n]
        runs = [_oracle_search(start, L, cyc, BUDGET, g) for g in (False, True)]
        if all(errs == 0 and not found for _, _, errs, found in runs):
            picked.append((start, runs[0][0]))
        if len(picked) == 3:
            break
    assert len(picked) == 3
    return picked


@pytest.mark.parametrize("L", [36, 65, 128])
@pytest.mark.parametrize("cyc", [False, True])
def test_planted_bfs_engines_store_the_oracle_bfs(L, cyc, capsys):
    """The device BFS at chunk 0 and 3, the sharded BFS at one rank and the host engine from planted
    starts, budget 200 (the root, its 12 children, theirs): the same node keys in the same order as
    a plain FIFO + dedup BFS over O.expand12."""
    from acx.search import _device_bfs as D
    from acx.search import _engine as E
    from acx.search import _sharded_bfs as S
    for start, order in search_starts(L, cyc):
        n = len(order)
        assert n >= BUDGET

        def check(name, nodes, keys):
            assert nodes == n, (name, nodes, n)
            M._same(f"L={L} cyc={cyc} {name}: nodes", unpack_keys_np(keys[:n], L), order, name)

        for chunk in (0, 3):
            assert D.device_bfs(start, BUDGET, cyclically_reduce_after_moves=cyc, device=DEV, chunk=chunk,
                                keep_node_keys=True) == (False, None)
            check(f"device bfs chunk {chunk}", D.LAST_STATS["nodes"], D.LAST_STATS["node_keys"])
        assert S.sharded_bfs(start, BUDGET, cyclically_reduce_after_moves=cyc, device=DEV, chunk=3,
                             keep_node_keys=True) == (False, None)
        assert np.array_equal(S.LAST_STATS["node_ids"][:n], np.arange(n))
        check("sharded bfs", S.LAST_STATS["nodes"], S.LAST_STATS["node_keys"])
        ok, _ = E.run_search(E.BFS, start, BUDGET, False, cyc, device=DEV, keep_node_keys=True)
        assert not ok
        check("host engine", E.LAST_STATS["nodes"], E.LAST_STATS["node_keys"])
    capsys.readouterr()


@pytest.mark.parametrize("L", [36, 65, 128])
@pytest.mark.parametrize("cyc", [False, True])
@pytest.mark.parametrize("engine", ["host", "device"])
def test_planted_greedy_engines_are_closed_under_the_oracle(L, cyc, engine, capsys):
    """Both greedy engines from the planted starts, budget 200: every popped node but the last has
    all its err-0 oracle children among the stored keys, and every stored key but the root is an
    oracle child of a stored node."""
    from acx.search import _engine as E
    from oracle import oracle as O
    for start, _ in search_starts(L, cyc):
        E.run_search(E.GREEDY, start, BUDGET, False, cyc, device=DEV, keep_node_keys=True, engine=engine)
        st = dict(E.LAST_STATS)
        nodes = unpack_keys_np(st["node_keys"], L)
        assert len(nodes) >= BUDGET and np.array_equal(nodes[0], start.astype(np.int8))
        stored = {r.tobytes() for r in nodes}
        assert len(stored) == len(nodes)
        ch, _, err = O.expand12(nodes.astype(np.int32), L, cyc)
        ch = ch.astype(np.int8)
        popped = [int(i) for i in st["popped"]]
        assert len(popped) >= 2
        for i in popped[:-1]:
            for a in range(12):
                assert err[i, a] != 0 or ch[i, a].tobytes() in stored, (L, cyc, engine, i, a)
        children = {ch[i, a].tobytes() for i in range(len(nodes)) for a in range(12) if err[i, a] == 0}
        assert all(r.tobytes() in children for r in nodes[1:]), (L, cyc, engine)
    capsys.readouterr()
