"""CPU: what makes tests/test_gpu_search_edge.py say something, checked on the sources and on the
two yardsticks alone (tests/search_edge_common.py describes the lengths and the starts).

EDGE_L must still hold every length at which the search engines' dispatch (bfs::nw_for, by_nw) or
the key's word count (key_words) changes: someone who adds a class or moves a threshold gets a
failing test, not a silent hole.  And per (L, cyclical) the starts must do what the GPU tests rely
on: the twins are stored, their packed keys differ in one 2-bit field at the top of the long
relator's tile, greedy's second pop on the power starts is decided at that letter, a move is
refused at the length limit, and a stored relator fills its tile.  The host engine
(csrc/acx_search.cpp) needs no GPU when the oracle expands for it: it runs here too, at every length."""
import ctypes
import re

import numpy as np
import pytest

import search_edge_common as SE
from bfs_yardstick import BUDGET
from conftest import PKG_ROOT, REPO, unpack_keys_np
from oracle import oracle as O
from test_instantiation_matrix import _nw_classes, _read
from weak_hash_common import pack_keys_np


def _key_words():
    m = re.search(r"constexpr int key_words\(int L\)\s*\{\s*return\s+([^;]+);", _read(PKG_ROOT, "csrc", "acx_expand_kernels.h"))
    assert m and re.fullmatch(r"[0-9L+*/() ]+", m.group(1)), "key_words not found"
    expr = m.group(1).replace("/", "//")
    assert re.search(r"int32_t acx_key_words\(int32_t L\)\s*\{\s*return key_words\(L\);", _read(PKG_ROOT, "csrc", "acx_kernels.hip"))
    return lambda L: int(eval(expr, {"L": L}))  # noqa: S307 -- digits, L and arithmetic only (checked above)


def test_edge_lengths_cover_every_class_edge_and_key_word_step():
    common = _read(PKG_ROOT, "csrc", "acx_bfs_common.h")
    steps, nw_rest = _nw_classes(common)
    # by_nw's switch handles every NW that nw_for returns, the last one as its default
    assert [int(x) for x in re.findall(r"case (\d+): f\(std::integral_constant<int, \1>\{\}\); break;", common)] == \
        [nw for _, nw in steps]
    assert re.search(rf"default: f\(std::integral_constant<int, {nw_rest}>\{{\}}\); break;", common)
    max_l = int(re.search(r"#define\s+ACX_MAX_L\s+(\d+)", _read(REPO, "include", "acx.h")).group(1))
    kw = _key_words()
    assert SE.TILE_L == [15, 16, 17, 31, 32, 33, 47, 48, 49, 63, 64, 65, 76, 77, 127, 128]
    assert SE.EDGE_L == sorted(set(SE.EDGE_L)) and set(SE.TILE_L) <= set(SE.EDGE_L) and max(SE.EDGE_L) == max_l
    bounds = [t for t, _ in steps]
    assert bounds == sorted(bounds) and bounds[-1] < max_l
    lo = 1  # (the starts need a relator of 11 letters or more: of the first class only its last lengths are held)
    for hi, nw in steps + [(max_l, nw_rest)]:
        in_class = [x for x in SE.EDGE_L if lo <= x <= hi]
        if (hi, nw) in steps:
            assert hi == 16 * nw, (hi, nw)  # a class ends on a full tile of 16 NW letters
            assert kw(hi) == nw + 1  # where the two length bytes open a key word of their own
            assert hi + 1 in SE.EDGE_L, f"first L of the class after NW={nw} ({hi + 1}) not in EDGE_L"
        assert hi in SE.EDGE_L, f"full tile L={hi} of class NW={nw} not in EDGE_L"
        assert any((4 * x) % 64 > 48 for x in in_class), f"no L of class NW={nw} whose length bytes straddle a word"
        assert len({kw(x) for x in in_class}) >= 2, f"one key-word count only in class NW={nw}"
        lo = hi + 1
    for L in range(1, max_l):  # both sides of every change of the key-word count
        if kw(L) != kw(L + 1):
            assert L in SE.EDGE_L and L + 1 in SE.EDGE_L, f"key words step at {L} | {L + 1}, not both in EDGE_L"
    assert max_l - 1 in SE.EDGE_L and kw(max_l) == max(kw(x) for x in SE.EDGE_L)
    # the near-full word is what the module says it is
    for L in SE.EDGE_L:
        v = SE.near_full_word(L)
        assert len(v) == L - 1 and v[0] == v[-1] == SE.Y and all(a != -b for a, b in zip(v, v[1:]))
        assert len(set(v)) >= 3


@pytest.mark.parametrize("L,cyc", SE.CASES)
def test_edge_starts_turn_on_the_top_key_word(L, cyc):
    for name, case in SE.cases(L, cyc).items():
        where = (L, cyc, name)
        s = case["start"]
        if name == "T1":  # its first child is a new node whose key differs from the root's in the last word only
            assert L % 16 == 13 and not any(y["raises"] for e in ("bfs", "greedy") for _, y in case[e]), where
            child = O.expand12(s[None], L, cyc)[0][0, 0].astype(np.int32)
            diff = np.bitwise_xor.reduce(pack_keys_np(np.stack([s, child]), L))
            assert np.nonzero(diff)[0].tolist() == [len(diff) - 1] and int(diff[-1]) < 16, where
            assert np.array_equal(SE.mid_run(case, "bfs")["states"][1], child), where
            assert tuple(int(v) for v in child) in SE.mid_run(case, "greedy")["stored"], where
            continue
        half, (a_x, a_inv) = SE.TWINS[name]
        at = half * L + L - 1  # the long relator's last letter
        ch, lens, err = (v[0] for v in O.expand12(s[None], L, cyc))
        twins = ch[[a_x, a_inv]].astype(np.int32)
        assert not err[[a_x, a_inv]].any() and (lens[[a_x, a_inv], half] == L).all(), where
        assert np.nonzero(twins[0] != twins[1])[0].tolist() == [at] and twins[:, at].tolist() == [SE.X, -SE.X], where
        # their keys: one word differs, in one 2-bit field, the top one of the relator's tile
        keys = pack_keys_np(twins, L)
        assert np.array_equal(unpack_keys_np(keys, L), twins)
        diff = keys[0] ^ keys[1]
        bit = SE.twin_bit(name, L)
        assert bit == 2 * at and np.nonzero(diff)[0].tolist() == [bit // 64], where
        assert int(diff[bit // 64]) >> (bit % 64) in (1, 2, 3) and int(diff[bit // 64]) & ((1 << (bit % 64)) - 1) == 0, where
        assert bit // 64 == (2 * (half + 1) * L - 1) // 64, where  # no later word holds a letter of that relator
        # no run raises; the BFS runs and the power starts' greedy runs end on the budget
        for engine in ("bfs", "greedy"):
            assert not any(y["raises"] for _, y in case[engine]), where
            assert [b for b, _ in case[engine]][1:] == [case["mid"], 1], where
        b, g = SE.mid_run(case, "bfs"), SE.mid_run(case, "greedy")
        assert b["status"] == BUDGET and b["nodes"] >= case["mid"], where
        # both twins are stored, as nodes of their own
        rows = {r.tobytes(): i for i, r in enumerate(b["states"])}
        assert len(rows) == len(b["states"]) == b["nodes"], where
        ids = [rows.get(t.tobytes()) for t in twins]
        assert None not in ids and ids[0] != ids[1] and all(b["node_parent"][i] == 0 for i in ids), where
        assert len(set(g["stored"])) == len(g["stored"]) == g["nodes"], where
        assert all(tuple(int(v) for v in t) in g["stored"] for t in twins), where
        # a refused move (the child is its own parent), and a stored relator of exactly L letters
        assert any(p == j for p, j in b["dups"]), where
        assert ((b["states"].reshape(-1, 2, L) != 0).sum(2) == L).any(), where
        if name[0] != "P":
            continue
        # greedy's second pop takes one twin, the other is the runner-up: equal in total and depth,
        # first different at the last position a comparison of the two tuples can reach
        assert g["status"] == BUDGET, where
        popped, (total, depth, runner) = g["pops"][1], g["runner_up"][1]
        assert {popped, runner} == {tuple(int(v) for v in t) for t in twins}, where
        assert total == L + 1 == int(np.count_nonzero(popped)) and depth == 1, where
        assert next(i for i in range(2 * L) if popped[i] != runner[i]) == at, where
        assert at == (2 * L - 1 if half else L - 1) and popped[at] == -SE.X, where
        # ended right after that pop, the search returns a path that begins with the popped twin's id
        b1, y1 = case["greedy"][0]
        assert b1 == g["nodes_after"][1] and (y1["status"], y1["parents"]) == (BUDGET, 2), where
        assert y1["path"][1][0] == a_inv, where


@pytest.mark.parametrize("cyc", [False, True])
def test_a_compare_short_of_the_last_key_word_merges_stored_nodes(cyc):
    """At every L but 13 (where the last key word is always zero) some start's stored nodes, under
    BFS and under greedy, hold two whose keys agree in all words but the last: an engine whose key
    compare, hash, copy or priority compare stopped at kw - 1 words would take them for one node
    or leave their order open, and its node counts and stored states would differ from the
    yardstick's."""
    for L in SE.EDGE_L:
        merged = {"bfs": [], "greedy": []}
        for name, case in SE.cases(L, cyc).items():
            for engine, rows in (("bfs", SE.mid_run(case, "bfs")["states"]),
                                 ("greedy", np.array(SE.mid_run(case, "greedy")["stored"], np.int32))):
                keys = pack_keys_np(rows, L)
                assert len(np.unique(keys, axis=0)) == len(keys)
                if len(np.unique(keys[:, :-1], axis=0)) < len(keys):
                    merged[engine].append(name)
        if L == 13:
            assert all(int(pack_keys_np(SE.mid_run(c, "bfs")["states"], L)[:, -1].max()) == 0
                       for c in SE.cases(L, cyc).values())
            continue
        assert merged["bfs"] and merged["greedy"], (L, cyc, merged)
        if L % 16 == 13:
            assert merged == {"bfs": ["T1"], "greedy": ["T1"]}, (L, cyc, merged)


def _drive(mode, start, budget, cyc, batch=256):
    """The host engine with the GPU expansion replaced by the oracle's: what _engine.run_search
    reads of it (status, min_length, nodes, node keys, popped ids, path)"""
    from acx import _lib
    from acx.search import _engine as E
    L = len(start) // 2
    lib, kw = _lib.load(), _lib.key_words(L)
    h = lib.acx_search_create(mode, L, E._pack_key(start.astype(np.int64), L).ctypes.data, budget)
    try:
        buf, status = np.zeros((batch, kw), np.uint64), 0
        while status == 0:
            n = lib.acx_search_next_batch(h, buf.ctypes.data, batch)
            if n == 0:
                break
            ch, _, err = O.expand12(unpack_keys_np(buf[:n], L).astype(np.int32), L, cyc)
            assert not err.any()
            keys = np.ascontiguousarray(pack_keys_np(ch.reshape(-1, 2 * L), L).reshape(n, 12, kw))
            status = lib.acx_search_feed(h, keys.ctypes.data, n)
        nodes, min_len = ctypes.c_int64(0), ctypes.c_int32(0)
        status = lib.acx_search_status(h, None, ctypes.byref(min_len), ctypes.byref(nodes))
        npop = lib.acx_search_popped(h, None, 0)
        pops = np.zeros(max(npop, 1), np.int64)
        lib.acx_search_popped(h, pops.ctypes.data, npop)
        nk = np.zeros((nodes.value, kw), np.uint64)
        lib.acx_search_node_keys(h, nk.ctypes.data, nodes.value)
        acts, tots = np.zeros(4096, np.int32), np.zeros(4096, np.int32)
        m = lib.acx_search_path(h, acts.ctypes.data, tots.ctypes.data, 4096)
        return dict(status=status, min_length=min_len.value, nodes=nodes.value, popped=pops[:npop],
                    states=unpack_keys_np(nk, L).astype(np.int32), path=[(int(acts[i]), int(tots[i])) for i in range(m)])
    finally:
        lib.acx_search_destroy(h)


@pytest.mark.parametrize("L,cyc", SE.CASES)
def test_host_engine_on_oracle_expansions(L, cyc):
    """BFS stores the yardstick's states in order; greedy stores the yardstick's set of states,
    pops the yardstick's pops in order and returns its path"""
    from acx.search import _engine as E
    for name, case in SE.cases(L, cyc).items():
        for mode, engine in ((E.BFS, "bfs"), (E.GREEDY, "greedy")):
            for budget, y in case[engine]:
                where = (L, cyc, name, engine, budget)
                r = _drive(mode, case["start"], budget, cyc)
                assert (r["status"] == 1, r["min_length"]) == (y["ok"], y["min_length"]), where
                if y["status"] == BUDGET:
                    assert r["nodes"] == y["nodes"], where
                if engine == "bfs":
                    assert np.array_equal(r["states"][:y["nodes"]], y["states"]), where
                    assert (r["path"] if y["ok"] else None) == SE.want_result(y)[1], where
                else:
                    assert {tuple(x) for x in r["states"].tolist()} == set(y["stored"]), where
                    assert np.array_equal(r["states"][r["popped"]], np.array(y["pops"], np.int32).reshape(-1, 2 * L)), where
                    assert r["path"] == SE.want_result(y)[1], where
