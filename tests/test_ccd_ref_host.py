"""CPU-only checks of the coupled-cluster-doubles reference of tests/_ccd_ref.py itself, before anything on the device
is compared with it: for two particles CCD is CID (``exp(T2)|0> = (1 + T2)|0>``), so the converged energy must be an
eigenvalue of the Hamiltonian on {reference} + {doubles}, built independently by tests/_det_ci_ref.py; the start of the
iteration is the MP2 energy; and the packed-triangle form of the pair contraction is the full ``einsum`` on an
anti-symmetrised tensor."""

import numpy as np
import pytest

import _ccd_ref as cc
import _det_ci_ref as dref


def cid_levels(ht, ut, n):
    """Eigenvalues of H on the reference determinant (the n lowest orbitals) and its double excitations, ascending,
    minus the reference's own energy: the lowest is the CID correlation energy."""
    m = ht.shape[0]
    H = dref.dense_hamiltonian(ht, ut, n)
    sec = dref.sector(m, n)
    ref = (1 << n) - 1
    keep = [i for i, x in enumerate(sec) if x == ref or dref.popcount(int(x) ^ ref) == 4]
    i0 = keep.index(int(np.nonzero(sec == ref)[0][0]))
    sub = H[np.ix_(keep, keep)]
    return np.linalg.eigvalsh(sub) - float(np.real(sub[i0, i0]))


@pytest.mark.parametrize("complex_", [False, True], ids=["real", "complex"])
def test_two_particles_ccd_is_cid(complex_):
    l, n = 6, 2
    h, u, C = cc.antisymmetric_problem(l, seed=17, complex_=complex_)
    assert np.abs(C.conj().T @ C - np.eye(l)).max() < 1e-13
    f, ut = cc.orbital_tensors(h, u, C, n)
    assert np.abs(f - np.diag(np.diagonal(f))).max() > 1e-2                       # non-canonical orbitals
    ht = np.einsum("pa,pq,qb->ab", C.conj(), h, C)
    e, t, its = cc.solve(h, u, C, n, tol=1e-12)
    want = cid_levels(ht, ut, n)[0]
    print(f"CCD {e:.12f}, CID {want:.12f}, {its} iterations")
    assert abs(e - want) <= 1e-10
    np.testing.assert_allclose(t, -t.transpose(1, 0, 2, 3), atol=1e-12)
    np.testing.assert_allclose(t, -t.transpose(0, 1, 3, 2), atol=1e-12)


def test_zero_iterations_is_mp2():
    l, n = 6, 3
    h, u, C = cc.antisymmetric_problem(l, seed=3, complex_=True)
    f, ut = cc.orbital_tensors(h, u, C, n)
    t = cc.first_order(f, ut, n)
    assert abs(cc.energy(ut, t, n) - cc.mp2(f, ut, n)) <= 1e-14 * abs(cc.mp2(f, ut, n)) * 10


def test_residual_vanishes_at_the_fixed_point_and_keeps_the_symmetry():
    l, n = 7, 3
    h, u, C = cc.antisymmetric_problem(l, seed=5, complex_=False)
    f, ut = cc.orbital_tensors(h, u, C, n)
    e, t, _ = cc.solve(h, u, C, n, tol=1e-12)
    R = cc.residual(f, ut, t, n)
    assert np.linalg.norm(R.ravel()) < 1e-12
    t0 = cc.antisymmetric_amplitudes(np.random.default_rng(1), l - n, n)
    R0 = cc.residual(f, ut, t0, n)
    np.testing.assert_allclose(R0, -R0.transpose(1, 0, 2, 3), atol=1e-13)
    np.testing.assert_allclose(R0, -R0.transpose(0, 1, 3, 2), atol=1e-13)
    wide = cc.residual(f.astype(np.longdouble), ut.astype(np.longdouble), t0.astype(np.longdouble), n)
    assert wide.dtype == np.longdouble and np.abs(wide - R0).max() < 1e-13


@pytest.mark.parametrize("complex_", [False, True], ids=["real", "complex"])
@pytest.mark.parametrize("l", [2, 3, 5, 8])
def test_packed_triangle_is_the_full_sum(l, complex_):
    rng = np.random.default_rng(l)
    _, u, _ = cc.antisymmetric_problem(l, seed=l, complex_=complex_)
    T = rng.standard_normal((3, l, l)) + (1j * rng.standard_normal((3, l, l)) if complex_ else 0)
    T = T - T.transpose(0, 2, 1)
    got = cc.pair_contract_antisym(u, T)
    want = np.einsum("pqrs,krs->kpq", u, T)
    np.testing.assert_allclose(got, want, atol=1e-12 * max(1.0, np.abs(want).max()))
    r, s = cc.triangle(l)
    assert len(r) == l * (l - 1) // 2 and (r < s).all()
    assert (got[:, np.arange(l), np.arange(l)] == 0).all()
    assert cc.pair_contract_antisym(u, T, extended=True).dtype in (np.longdouble, np.clongdouble)
    assert (np.abs(got - cc.pair_contract_antisym(u, T, extended=True)) <= cc.pair_bound(u, T) + 0).all()
