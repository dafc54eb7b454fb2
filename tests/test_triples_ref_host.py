"""The NumPy reference of the triples correction (tests/_triples_ref.py) against itself, on the CPU: the closed-shell
working form against the determinant definition, the restricted sum against the full one, the elements that must
vanish, and the rounding bound of the kernel's sum -- that the fp64 evaluation lies inside it and a wrong one far
outside."""

import numpy as np
import pytest

import _rccd_ref as rc
import _triples_ref as tr

CASES = [(5, 2), (6, 3)]


def amplitudes(ls, ns, seed, complex_):
    return rc.closed_shell_amplitudes(np.random.default_rng(seed), ls - ns, ns, complex_=complex_)


@pytest.mark.parametrize("complex_", [False, True], ids=["real", "complex"])
@pytest.mark.parametrize("ls, ns", CASES)
def test_working_form_is_the_determinant_sum(ls, ns, complex_):
    h, u, eps = tr.canonical_problem(ls, ns, 7 + ls, complex_=complex_)
    f, _ = rc.orbital_tensors(h, u, np.eye(ls), ns)
    assert np.abs(f - np.diag(eps)).max() <= 1e-13                  # canonical: f = diag(eps)
    t = amplitudes(ls, ns, 3, complex_)
    want = tr.definition(h, u, eps, ns, t)
    _, got = tr.working(u, eps, ns, t)
    print(f"l = {ls}, o = {ns}: definition {want:.15e}, working form {got:.15e}, relative {abs(got - want) / abs(want):.1e}")
    assert want < 0.0
    assert abs(got - want) <= 1e-12 * abs(want)


@pytest.mark.parametrize("complex_", [False, True], ids=["real", "complex"])
def test_restricted_sum_is_the_full_sum(complex_):
    ls, ns = 7, 3
    _, u, eps = tr.canonical_problem(ls, ns, 21, complex_=complex_)
    e, total = tr.working(u, eps, ns, amplitudes(ls, ns, 5, complex_))
    full = e.sum()
    print(f"restricted {total:.15e}, full {full:.15e}")
    assert abs(total - full) <= 1e-13 * abs(full)
    for i, j, k in tr.triples(ns):                                  # e is symmetric in (i, j, k)
        assert abs(e[i, j, k] - e[k, i, j]) <= 1e-13 * abs(full) and abs(e[i, j, k] - e[j, i, k]) <= 1e-13 * abs(full)


@pytest.mark.parametrize("complex_", [False, True], ids=["real", "complex"])
def test_like_spins_in_one_orbital_vanish(complex_):
    """``e_iii`` and every a = b = c element are zero to the kernel's bound."""
    ls, ns = 6, 2
    nv = ls - ns
    _, u, eps = tr.canonical_problem(ls, ns, 33, complex_=complex_)
    X = tr.packed_blocks(tr.blocks(u, ns, amplitudes(ls, ns, 8, complex_)))
    ev = eps[ns:]
    for i in range(ns):
        row, eo3 = tr.slot_row(ns, i, i, i), 3 * eps[i]
        e = tr.kernel_ref(X, [row], [eo3], ev)[0]
        bound = tr.kernel_bound(X, [row], [eo3], ev)[0]
        scale = np.abs(tr.kernel_terms(X, row, eo3, ev)).sum()
        print(f"e_{i}{i}{i} = {e:.3e}, bound {bound:.3e}, sum of |terms| {scale:.3e}")
        assert abs(e) <= bound
    row, eo3 = tr.slot_row(ns, 0, 1, 1), eps[0] + 2 * eps[1]
    terms = tr.kernel_terms(X, row, eo3, ev)
    bounds = tr.kernel_bound_terms(X, row, eo3, ev, 1)
    d = np.arange(nv)
    assert np.abs(terms).max() > 1e3 * bounds.max()                 # the triple itself is far from zero
    assert (np.abs(terms[d, d, d]) <= bounds[d, d, d]).all()


@pytest.mark.parametrize("share", ["none", "pair", "all"])
@pytest.mark.parametrize("complex_", [False, True], ids=["real", "complex"])
def test_bound_holds_the_fp64_sum_and_sees_a_wrong_one(complex_, share):
    X, slots, eo3, ev = tr.kernel_problem(9, 4, 8, 17, complex_=complex_, share=share)
    wide = tr.kernel_ref(X, slots, eo3, ev, extended=True)
    bound = tr.kernel_bound(X, slots, eo3, ev)
    own = np.abs(tr.kernel_ref(X, slots, eo3, ev) - wide).astype(np.float64)
    print(f"fp64 against extended: worst ratio to the bound {(own / bound).max():.3e}")
    assert (own <= bound).all()
    for drop in range(6):
        wrong = np.abs(tr.kernel_ref(X, slots, eo3, ev, drop=drop) - wide).astype(np.float64)
        assert (wrong > 1e3 * bound).all(), drop


# -- the helpers of tests/test_gpu_triples_scale.py


@pytest.mark.parametrize("v, T", [(5, 8), (8, 8), (10, 8), (13, 6), (19, 6), (20, 3)])
def test_tile_set_sums_add_up_to_the_reference(v, T):
    X, slots, eo3, ev = tr.kernel_problem(v, 1, 6, 100 + v, complex_=T == 6)
    terms = tr.kernel_terms(X, slots[0], eo3[0], ev, extended=True)
    sums = tr.tile_set_sums(terms, T)
    nt = -(-v // T)
    assert sums.shape == (nt * (nt + 1) * (nt + 2) // 6,) and sums.dtype == np.longdouble
    wide = tr.kernel_ref(X, slots, eo3, ev, extended=True)[0]
    assert abs(sums.sum() - wide) <= 1e-16 * np.abs(terms).sum()
    # the kernel's order: tc slowest, then tb, then ta; an element goes to the set of its sorted tile indices
    sets = [(ta, tb, tc) for tc in range(nt) for tb in range(tc + 1) for ta in range(tb + 1)]
    assert len(sets) == len(sums)
    tile = np.arange(v) // T
    for x, (ta, tb, tc) in enumerate(sets):
        mask = np.zeros((v, v, v), dtype=bool)
        for p, q, r in {(ta, tb, tc), (ta, tc, tb), (tb, ta, tc), (tb, tc, ta), (tc, ta, tb), (tc, tb, ta)}:
            mask |= (tile[:, None, None] == p) & (tile[None, :, None] == q) & (tile[None, None, :] == r)
        assert abs(sums[x] - terms[mask].sum()) <= 1e-16 * np.abs(terms[mask]).sum(), (ta, tb, tc)


def test_sensitivity_leaves_out_what_vanishes_by_identity_only():
    T = 8
    for v, share in ((2 * T + 1, "none"), (T + 2, "none"), (T + 2, "pair")):
        X, slots, eo3, ev = tr.kernel_problem(v, 1, 6, 100 + v, share=share)
        terms = tr.kernel_terms(X, slots[0], eo3[0], ev, extended=True)
        sums = np.abs(tr.tile_set_sums(terms, T)).astype(np.float64)
        bound = tr.kernel_bound(X, slots, eo3, ev)[0]
        ratio = tr.tile_set_sensitivity(X, slots, eo3, ev, T)
        print(f"v = {v}, {share}: set contributions / bound {sums / bound}, sensitivity {ratio:.3e}")
        if v % T == 1:                                              # the one-element ragged tile: its diagonal set is ~0
            assert sums[-1] <= bound and ratio == sums[:-1].min() / bound
        else:
            assert ratio == sums.min() / bound
        assert ratio >= 100
    X, slots, eo3, ev = tr.kernel_problem(T + 2, 1, 6, 3, share="all")      # one block six times: e = 0, nothing to see
    assert abs(tr.kernel_ref(X, slots, eo3, ev, extended=True)[0]) <= tr.kernel_bound(X, slots, eo3, ev)[0]
    assert tr.tile_set_sensitivity(X, slots, eo3, ev, T) == np.inf
    # even orders one block, odd orders another: W is cyclic, and totally symmetric where two indices are equal -- all
    # that the diagonal set of a ragged tile of two holds; one element more in that tile and the set counts again
    for v, blind in ((T + 2, True), (T + 3, False)):
        X, _, eo3, ev = tr.kernel_problem(v, 2, 6, 100 + v)
        slots = np.array([[2, 5, 5, 2, 2, 5], [2, 5, 5, 2, 5, 2]], dtype=np.int32)
        bound = tr.kernel_bound(X, slots, eo3, ev)
        last = [abs(tr.tile_set_sums(tr.kernel_terms(X, row, eo3[x], ev, extended=True), T)[-1]) for x, row in enumerate(slots)]
        assert (last[0] <= bound[0]) == blind and last[1] > 100 * bound[1]
        assert tr.tile_set_sensitivity(X, slots, eo3, ev, T) >= 100


@pytest.mark.parametrize("v, T, complex_", [(10, 8, False), (8, 6, True)])
def test_sensitivity_of_every_slot_pattern(v, T, complex_):
    """At a ragged tile of two, what is left out is below the bound (0 by identity), everything else 100 bounds at least."""
    X, _, eo3, ev = tr.kernel_problem(v, 203, 12, 300 + v, complex_=complex_)
    slots = tr.slot_partitions(12, seed=v)
    bound = tr.kernel_bound(X, slots, eo3, ev)
    left_out = 0
    for x, row in enumerate(slots):
        sums = np.abs(tr.tile_set_sums(tr.kernel_terms(X, row, eo3[x], ev, extended=True), T)).astype(np.float64)
        small = sums < 100 * bound[x]
        assert (sums[small] <= bound[x]).all(), (tr.coincidence(row), sums / bound[x])
        if small.any():
            left_out += 1
            assert tr.coincidence(row) in ((0,) * 6, (0, 1, 1, 0, 0, 1)), (tr.coincidence(row), sums / bound[x])
            assert small.all() or (small == [False, False, False, True]).all()
    assert left_out == 2 and tr.tile_set_sensitivity(X, slots, eo3, ev, T) >= 100


def test_slot_partitions_are_the_203_coincidences():
    rows = tr.slot_partitions(12, seed=4)
    assert rows.shape == (203, 6) and rows.dtype == np.int32
    assert rows.min() >= 0 and rows.max() < 12 and len(set(rows.ravel().tolist())) == 12
    patterns = {tr.coincidence(row) for row in rows}
    assert len(patterns) == 203                                     # the Bell number of six
    assert all(len(set(row.tolist())) == max(tr.coincidence(row)) + 1 for row in rows)     # classes on distinct blocks
    assert tr.coincidence(tr.slot_row(3, 0, 0, 1)) == (0, 1, 0, 1, 2, 2) in patterns       # i = j < k
    assert tr.coincidence(tr.slot_row(3, 0, 1, 1)) == (0, 0, 1, 2, 1, 2) in patterns       # i < j = k
    assert tr.coincidence(tr.slot_row(3, 0, 1, 2)) == (0, 1, 2, 3, 4, 5) in patterns       # all different
    assert (0,) * 6 in patterns
    # the seed moves the blocks and their order of appearance, not the patterns; the first class is not always the lowest
    other = tr.slot_partitions(12, seed=5)
    assert [tr.coincidence(r) for r in other] == [tr.coincidence(r) for r in rows] and (other != rows).any()
    assert any(row[0] != row.min() for row in rows) and any(row[0] == row.min() for row in rows)
    assert np.array_equal(rows, tr.slot_partitions(12, seed=4))
