"""Pins the NumPy oracle of tests/_two_particle_ref.py on the CPU: without interaction the levels are sums of orbital
energies, and the spin-orbital spectrum is the singlets once and the triplets three times."""

import numpy as np
import pytest

import _mean_field_ref as mf
import _two_particle_ref as tp


def test_pair_contract_restatement_and_bound():
    rng = np.random.default_rng(1)
    u = rng.standard_normal((3, 4, 5, 6)) + 1j * rng.standard_normal((3, 4, 5, 6))
    T = rng.standard_normal((2, 5, 6)) + 1j * rng.standard_normal((2, 5, 6))
    S = tp.pair_contract(u, T)
    want = (u.reshape(12, 30) @ T.reshape(2, 30).T).T.reshape(2, 3, 4)
    np.testing.assert_allclose(S, want, rtol=1e-13, atol=1e-13)
    np.testing.assert_array_equal(tp.pair_contract(u, T[1]), S[1])
    exact = tp.pair_contract(u, T, extended=True)
    assert exact.dtype == np.clongdouble
    assert (np.abs(S - exact) <= tp.error_bound(u, T)).all()
    assert tp.pair_contract(u.real, T.real, extended=True).dtype == np.longdouble
    assert (tp.error_bound(u, T) == 2 * np.sqrt(2) * tp.error_bound(np.abs(u), np.abs(T))).all()


def test_pair_basis_is_orthonormal_and_has_the_symmetry():
    for m in (2, 3, 5):
        for sign in (1, -1):
            B = tp.pair_basis(m, sign)
            assert B.shape[0] == (m * (m + 1) // 2 if sign > 0 else m * (m - 1) // 2)
            np.testing.assert_array_equal(B, sign * B.transpose(0, 2, 1))
            G = B.reshape(len(B), -1) @ B.reshape(len(B), -1).T
            np.testing.assert_allclose(G, np.eye(len(B)), atol=1e-15)


@pytest.mark.parametrize("complex_", [False, True])
def test_without_interaction_the_levels_are_sums_of_orbital_energies(complex_):
    l = 5
    h, u, s = mf.hermitian_problem(l, seed=3, complex_=complex_)
    X = tp.loewdin(s)
    eps = np.linalg.eigvalsh(X.conj().T @ h @ X)
    singlets = sorted(eps[i] + eps[j] for i in range(l) for j in range(i, l))
    triplets = sorted(eps[i] + eps[j] for i in range(l) for j in range(i + 1, l))
    np.testing.assert_allclose(tp.spectrum(h, 0 * u, X, +1), singlets, atol=1e-12)
    np.testing.assert_allclose(tp.spectrum(h, 0 * u, X, -1), triplets, atol=1e-12)


@pytest.mark.parametrize("l", [4, 5])
@pytest.mark.parametrize("complex_", [False, True])
def test_spin_orbital_spectrum_is_singlets_once_and_triplets_three_times(l, complex_):
    h, u, s = mf.hermitian_problem(l, seed=40 + l, scale=0.2, complex_=complex_)
    X = tp.loewdin(s)
    es, et = tp.spectrum(h, u, X, +1), tp.spectrum(h, u, X, -1)
    assert np.abs(es[:, None] - et[None, :]).min() > 1e-6           # the interaction tells the two sectors apart
    want = np.sort(np.concatenate([es, et, et, et]))
    for anti in (False, True):
        h2, u2, C2, f = tp.spin_double(h, u, X, anti)
        got = tp.spectrum(h2, u2, C2, -1, f)
        assert got.shape == want.shape
        np.testing.assert_allclose(got, want, atol=1e-12)
