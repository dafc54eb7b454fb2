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
