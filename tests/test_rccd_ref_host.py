"""CPU-only checks of the closed-shell coupled-cluster-doubles reference of tests/_rccd_ref.py itself, before anything
on the device is compared with it: its residual is the alpha-beta-alpha-beta block of the spin-orbital residual of
tests/_ccd_ref.py on the spin-doubled, anti-symmetrised problem with the embedded amplitudes (and that residual is itself
the embedding of the closed-shell one), the two iterations converge to the same energy, the start is the closed-shell
MP2 energy, and the packed-triangle form of the pair contraction is the full ``einsum`` on a tensor with particle-exchange
symmetry and ANY amplitudes."""

import numpy as np
import pytest

import _ccd_ref as cc
import _rccd_ref as rc

SHAPES = [(3, 1), (4, 2), (5, 2), (6, 3)]


@pytest.mark.parametrize("complex_", [False, True], ids=["real", "complex"])
@pytest.mark.parametrize("ls,ns", SHAPES)
def test_residual_is_the_block_of_the_spin_orbital_one(ls, ns, complex_):
    h, u, C = rc.closed_shell_problem(ls, seed=10 * ls + ns, complex_=complex_)
    assert np.abs(u - u.transpose(1, 0, 3, 2)).max() == 0 and np.abs(u - u.transpose(0, 1, 3, 2)).max() > 1e-3
    f, ut = rc.orbital_tensors(h, u, C, ns)
    assert np.abs(f - np.diag(np.diagonal(f))).max() > 1e-2                       # non-canonical orbitals
    t = rc.closed_shell_amplitudes(np.random.default_rng(ls), ls - ns, ns, complex_)
    R = rc.residual(f, ut, t, ns)

    hs, us, Cs = rc.spin_double(h, u, C)
    fs, uts = cc.orbital_tensors(hs, us, Cs, 2 * ns)
    np.testing.assert_allclose(fs, np.kron(f, np.eye(2)), atol=1e-13)           # the closed-shell Fock matrix, doubled
    Rs = cc.residual(fs, uts, rc.embed(t), 2 * ns)
    size = np.abs(Rs).max()
    dev = np.abs(rc.block(Rs) - R).max()
    print(f"({ls}, {ns}) {'complex' if complex_ else 'real'}: residual size {size:.2f}, deviation {dev:.2e}")
    assert dev <= 1e-13
    assert np.abs(rc.embed(R) - Rs).max() <= 1e-13
    np.testing.assert_allclose(R, R.transpose(1, 0, 3, 2), atol=1e-14)           # R^{ab}_{ij} = R^{ba}_{ji}
    np.testing.assert_array_equal(rc.block(rc.embed(t)), t)
    # the two energies and the two sets of denominators
    assert abs(rc.energy(ut, t, ns) - cc.energy(uts, rc.embed(t), 2 * ns)) <= 1e-13
    np.testing.assert_allclose(rc.block(cc.denominators(fs, 2 * ns)), rc.denominators(f, ns), atol=1e-13)
    wide = rc.residual(*(x.astype(np.clongdouble if complex_ else np.longdouble) for x in (f, ut, t)), ns)
    assert wide.dtype in (np.longdouble, np.clongdouble) and np.abs(wide - R).max() < 1e-13


@pytest.mark.parametrize("complex_", [False, True], ids=["real", "complex"])
@pytest.mark.parametrize("ls,ns", SHAPES)
def test_solve_agrees_with_the_spin_doubled_reference(ls, ns, complex_):
    h, u, C = rc.closed_shell_problem(ls, seed=10 * ls + ns, complex_=complex_)
    e, t, its = rc.solve(h, u, C, ns, tol=1e-12)
    es, ts, its_s = cc.solve(*rc.spin_double(h, u, C), 2 * ns, tol=1e-12)
    print(f"({ls}, {ns}): RCCD {e:.12f} in {its} iterations, spin-doubled CCD {es:.12f} in {its_s}")
    assert abs(e - es) <= 1e-12
    assert np.abs(rc.block(ts) - t).max() <= 1e-11
    np.testing.assert_allclose(t, t.transpose(1, 0, 3, 2), atol=1e-14)


def test_zero_iterations_is_closed_shell_mp2():
    ls, ns = 6, 3
    h, u, C = rc.closed_shell_problem(ls, seed=3, complex_=True)
    f, ut = rc.orbital_tensors(h, u, C, ns)
    t = rc.first_order(f, ut, ns)
    want = rc.mp2(f, ut, ns)
    assert abs(rc.energy(ut, t, ns) - want) <= 1e-13 * abs(want)
    fs, uts = cc.orbital_tensors(*rc.spin_double(h, u, C), 2 * ns)
    assert abs(want - cc.mp2(fs, uts, 2 * ns)) <= 1e-13 * abs(want)


@pytest.mark.parametrize("complex_", [False, True], ids=["real", "complex"])
@pytest.mark.parametrize("l", [1, 2, 3, 5, 8])
def test_packed_triangle_is_the_full_sum(l, complex_):
    rng = np.random.default_rng(l)
    _, u, _ = rc.closed_shell_problem(l, seed=l, complex_=complex_, scale=1.0)
    T = rng.standard_normal((3, l, l)) + (1j * rng.standard_normal((3, l, l)) if complex_ else 0)     # generic
    got = rc.pair_contract_exchange(u, T)
    want = np.einsum("pqrs,krs->kpq", u.astype(np.clongdouble if complex_ else np.longdouble), T)
    bound = rc.pair_bound(u, T)
    assert (np.abs(got - want) <= bound).all()
    r, s = rc.triangle(l)
    assert len(r) == l * (l + 1) // 2 and (r <= s).all()
    assert rc.pair_contract_exchange(u, T, extended=True).dtype in (np.longdouble, np.clongdouble)
    assert (np.abs(got - rc.pair_contract_exchange(u, T, extended=True)) <= bound).all()
    # only r <= s of U is used
    lower = np.tril(np.ones((l, l), dtype=bool), -1)
    np.testing.assert_array_equal(rc.pair_contract_exchange(np.where(lower[None, None], np.nan, u), T), got)
