"""The host oracle of tests/_string_ci_density_ref.py against independent statements of the same quantities (no GPU):
the spin sum of ``_det_ci_density_ref``'s spin-orbital two-body density, the spectrum of S^2, and <c|H|c> of the
Jordan-Wigner Hamiltonian of ``_string_ci_ref``."""

import numpy as np
import pytest

import _det_ci_density_ref as ddref
import _string_ci_density_ref as sref
import _string_ci_ref as ref


def vectors(m, Na, Nb, cplx, seed):
    na, nb = len(ref.strings(m, Na)), len(ref.strings(m, Nb))
    rng = np.random.default_rng(seed)
    c = rng.standard_normal((2, na, nb))
    if cplx:
        c = c + 1j * rng.standard_normal((2, na, nb))
    return c[0] / np.linalg.norm(c[0]), c[1] / np.linalg.norm(c[1])


@pytest.mark.parametrize("cplx", [False, True])
@pytest.mark.parametrize("m,Na,Nb", ref.SHAPES)
def test_gamma_is_the_spin_sum_of_the_spin_orbital_density(m, Na, Nb, cplx):
    E = ref.dense_E(m, Na, Nb)
    bra, ket = vectors(m, Na, Nb, cplx, 31 * m + Na)
    pos, phase = ref.sector_map(m, Na, Nb)
    for b, k in ((bra, bra), (bra, ket)):
        G, rho = sref.dense_gamma(E, b, k)
        rho_so, G_so = ddref.jw_densities(phase * b.reshape(-1), phase * k.reshape(-1), 2 * m, Na + Nb, keep=pos)
        assert np.abs(G - sref.spin_sum(G_so)).max() <= 1e-15
        assert np.abs(rho - (rho_so[0::2, 0::2] + rho_so[1::2, 1::2])).max() <= 1e-15
        # the truncated-list form on complete lists is the same operator
        pair = (ref.list_E(ref.strings(m, Na), m), ref.list_E(ref.strings(m, Nb), m))
        G2, rho2 = sref.dense_gamma(pair, b, k)
        assert np.abs(G - G2).max() <= 1e-15 and np.abs(rho - rho2).max() <= 1e-15
        N = Na + Nb
        assert np.abs(np.einsum("pqrq->pr", G) - (N - 1) * rho.T).max() <= 1e-14
        assert np.abs(G - G.transpose(1, 0, 3, 2)).max() <= 1e-15
    G, _ = sref.dense_gamma(E, bra, bra)
    assert np.abs(G - G.transpose(2, 3, 0, 1).conj()).max() <= 1e-15
    assert abs(np.einsum("pqpq->", G) - (Na + Nb) * (Na + Nb - 1)) <= 1e-14


@pytest.mark.parametrize("m,Na,Nb", ref.SHAPES)
def test_spin_squared_has_eigenvalues_s_s_plus_1_only(m, Na, Nb):
    S2 = sref.dense_spin_squared(m, Na, Nb)
    assert np.array_equal(S2, S2.T)
    lam = np.linalg.eigvalsh(S2)
    smin = abs(Na - Nb) / 2.0
    allowed = np.array([(smin + j) * (smin + j + 1) for j in range(min(Na, Nb, m - Na, m - Nb) + 1)])
    assert np.abs(lam[:, None] - allowed[None, :]).min(axis=1).max() <= 1e-12
    assert np.abs(lam - smin * (smin + 1)).min() <= 1e-12                     # the lowest multiplet is there
    # the table form: s0 c - sum_pq E^alpha_qp E^beta_pq c
    Ea, Eb = ref.list_E(ref.strings(m, Na), m), ref.list_E(ref.strings(m, Nb), m)
    c = np.eye(S2.shape[0]).reshape(S2.shape[0], Ea.shape[2], Eb.shape[2])
    got = sref.list_spin_squared(Ea, Eb, Na, Nb, c).reshape(S2.shape[0], -1)
    assert np.abs(got.T - S2).max() == 0


@pytest.mark.parametrize("cplx", [False, True])
@pytest.mark.parametrize("m,Na,Nb", ref.SHAPES)
def test_energy_functional_is_the_rayleigh_quotient(m, Na, Nb, cplx):
    ht, ut = ref.random_hamiltonian(m, 7 + m + Na, cplx)
    Hx = ref.dense_hamiltonian(ht, ut, Na, Nb, extended=True)
    bra, ket = vectors(m, Na, Nb, cplx, 5)
    E = ref.dense_E(m, Na, Nb)
    for b, k in ((bra, bra), (bra, ket)):
        G, rho = sref.dense_gamma(E, b, k)
        e = np.sum(ref._wide(ht) * rho.T) + np.longdouble(0.5) * np.sum(ref._wide(ut) * G)
        want = ref._wide(b).reshape(-1).conj() @ (Hx @ ref._wide(k).reshape(-1))
        assert abs(e - want) <= 1e-13 * max(1.0, float(np.abs(Hx).max()))
