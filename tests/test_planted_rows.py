"""CPU: the planted rows of tests/planted_rows.py are what they claim to be -- conditions on the
constructors and the oracle alone, no kernel.  The junction and peel depth measured on every row
equal its (k, m); the oracle's ACMove gives the constructed result; every word-boundary depth
occurs for every concatenation id; the gate classes are non-empty and behave as described; nested
rows reduce to their outer words; the unclean twins keep their junction depth."""
import numpy as np
import pytest

import planted_rows as P
from oracle import oracle as O


def _all_gate(L):
    return P.concat_sets(list(P.gate_rows(L).values()))


def _measure(row, a, L):
    """(junction depth, peel depth of the freely reduced product) of move id a on row"""
    i, sign = P.CONCAT[a]
    rel = P.relators(row, L)
    assert P.is_cyc_reduced(rel[0]) and P.is_cyc_reduced(rel[1])
    w = rel[1 - i] if sign == 1 else P.inv(rel[1 - i])
    k = P.junction_depth(rel[i], w)
    prod = rel[i][:len(rel[i]) - k] + w[k:]
    assert P.is_reduced(prod) and len(prod) > 0
    return k, P.peel_depth(prod), len(prod)


@pytest.mark.parametrize("L", P.PLANTED_L)
def test_measured_depths_equal_the_planted_ones(L):
    for s in (P.junction_rows(L), _all_gate(L)):
        for n, row in enumerate(s["rows"]):
            k, m, size = _measure(row, int(s["ids"][n]), L)
            assert (k, m) == (int(s["k"][n]), int(s["m"][n])), (L, n)
            assert size == 2 * m + int(s["ta"][n]) + int(s["tb"][n])
            assert bool(s["applies"][n]) == (size <= L)


@pytest.mark.parametrize("L", P.PLANTED_L)
def test_oracle_move_gives_the_constructed_result(L):
    for s in (P.junction_rows(L), _all_gate(L)):
        core = s["ta"] + s["tb"]
        for cyc, want in ((1, s["want_cyc"]), (0, s["want_flat"])):
            out, lens, err = O.move_batch(s["rows"], s["ids"], L, cyc)
            assert (err == 0).all()
            assert np.array_equal(out, want)
            ap = s["applies"]
            assert (want[ap] != s["rows"][ap]).any(1).all() and np.array_equal(want[~ap], s["rows"][~ap])
            tgt = np.array([P.CONCAT[int(a)][0] for a in s["ids"]])
            n_t = lens[np.arange(len(tgt)), tgt]
            assert np.array_equal(n_t[ap], (core + (0 if cyc else 2 * s["m"]))[ap])


@pytest.mark.parametrize("L", P.PLANTED_L)
def test_every_boundary_depth_occurs_for_every_id(L):
    """every d in DEPTHS(L) for which an applied combination exists at all (arithmetic on L alone)
    has an applied row with k = d for each move id 0..3; every d <= L/2 - 1 has an applied row with
    m = d"""
    s = P.junction_rows(L)
    D = P.depths(L)
    assert {0, 1, L - 2} <= set(D) and all(d in D for d in (15, 16) if d < L)
    have_k = {(int(a), int(k)) for a, k, ap in zip(s["ids"], s["k"], s["applies"]) if ap}
    have_m = {int(m) for m, ap in zip(s["m"], s["applies"]) if ap}
    n_k = 0
    for d in D:
        possible = any(max(d, m) >= 15 and P.fits(L, d, m, t) and P.applies(L, m, t) for m in D for t in P.TAILS)
        if possible:
            n_k += 1
            assert all((a, d) in have_k for a in range(4)), (L, d)
        if d <= L / 2 - 1:
            assert d in have_m, (L, d)
    assert n_k >= len([d for d in D if 15 <= d <= L - 1])  # every deep k that a relator can hold
    assert all(v.shape[0] == s["rows"].shape[0] for v in s.values())
    assert len(s["rows"]) <= 1300


@pytest.mark.parametrize("L", P.PLANTED_L)
def test_gate_classes(L):
    g = P.gate_rows(L)
    for name, s in g.items():
        assert len(s["rows"]) > 0, (L, name)
        size = 2 * s["m"] + s["ta"] + s["tb"]
        n_i = s["k"] + s["m"] + s["ta"]
        n_j = s["k"] + s["m"] + s["tb"]
        if name in ("len_L", "len_L1", "len_L2"):
            assert (size == L + ("len_L", "len_L1", "len_L2").index(name)).all()
            assert (s["applies"] == (name == "len_L")).all()
            assert s["k"].max() == L - s["m"][s["k"].argmax()] - max(s["ta"][s["k"].argmax()], s["tb"][s["k"].argmax()])
        elif name == "cancel_to_fit":
            assert (n_i + n_j > L).all() and s["applies"].all()
        else:
            assert (size > L).all() and (s["ta"] + s["tb"] <= L).all() and (s["k"] <= 2).all() and not s["applies"].any()
        for cyc in (0, 1):
            out, _, err = O.move_batch(s["rows"], s["ids"], L, cyc)
            assert (err == 0).all()
            same = (out == s["rows"]).all(1)
            assert np.array_equal(same, ~s["applies"]), (L, name, cyc)


@pytest.mark.parametrize("L", P.PLANTED_L)
def test_nested_rows_reduce_to_their_outer_words(L):
    s = P.nested_rows(L)
    assert set(s["half"].tolist()) == {0, 1}
    assert {d for d in P.depths(L) if 1 <= d <= (L - 2) // 2} <= set(s["depth"].tolist())
    for h in (0, 1):  # a cascade, and a plain nest, in either half
        assert set(s["cascade"][s["half"] == h].tolist()) == {False, True}
    for cyc in (0, 1):
        for row, want in zip(s["rows"], s["want"]):
            out, _, e = O.simplify_presentation(row, L, cyc)
            assert e == 0 and np.array_equal(out, want)
    for row, h, d in zip(s["rows"], s["half"], s["depth"]):
        w = P.relators(row, L)[h]
        mid = next(i for i in range(len(w) - 1) if w[i] == -w[i + 1])
        assert P.junction_depth(w[:mid + 1], w[mid + 1:]) == d  # one nest, exactly that deep


@pytest.mark.parametrize("L", P.PLANTED_L)
def test_unclean_twins_keep_the_junction(L):
    s = P.concat_sets([P.junction_rows(L), _all_gate(L)])
    t = P.unclean_twin(s, L)
    assert len(t["rows"]) >= len(s["rows"]) // 3  # the others have no room for two more letters
    deep = 0
    for row, a, k in zip(t["rows"], t["ids"], t["k"]):
        i, sign = P.CONCAT[int(a)]
        rel = P.relators(row, L)
        assert sum(not P.is_reduced(r) for r in rel) == 1
        w = rel[1 - i] if sign == 1 else P.inv(rel[1 - i])
        assert P.junction_depth(rel[i], w) == k
        deep += k >= 15
    assert deep > 0 or L < 15 + 1 + 2  # k = 15, a one-letter tail and the pair need 18 letters
    for cyc in (0, 1):
        assert (O.move_batch(t["rows"], t["ids"], L, cyc)[2] == 0).all()
