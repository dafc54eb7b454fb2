"""CPU checks of the TESTS' dense CIS (tests/_cis_ref.py), before the GPU tests lean on it: A is Hermitian, the one-by-
one case equals its closed forms, the orbitals agree with ``ref.plain_scf``, and the spin-orbital spectrum of a spin-
doubled closed shell is its singlet spectrum united with three copies of its triplet spectrum."""

import numpy as np

import _cis_ref as cis
import _mean_field_ref as ref


def test_cis_matrix_is_hermitian_and_scf_agrees_with_plain_scf():
    l, n = 6, 2
    h, u, s = ref.hermitian_problem(l, seed=11)
    e, eps, C = cis.scf_orbitals(h, u, s, n, 2.0, 1.0, -0.5)
    e_ref, _, _ = ref.plain_scf(h, u, s, n, 2.0, 1.0, -0.5)
    assert abs(e - e_ref) <= 1e-12
    np.testing.assert_allclose(C.conj().T @ s @ C, np.eye(l), atol=1e-12)
    u_mo = cis.to_canonical(u, C)
    for flavour, (cj, ck) in cis.FLAVOURS.items():
        A = cis.cis_matrix(eps, u_mo, n, cj, ck)
        assert A.shape == (n * (l - n),) * 2
        np.testing.assert_allclose(A, A.conj().T, atol=1e-13, err_msg=flavour)


def test_one_by_one_closed_forms():
    h, u, s = ref.hermitian_problem(2, seed=3)
    eps = np.array([-0.7, 0.4])
    J, K = u[1, 0, 0, 1], u[1, 0, 1, 0]                     # <10|01> (direct), <10|10> (exchange)
    closed = {"gos": 1.1 + J, "gos_plain": 1.1 + J - K, "singlet": 1.1 + 2 * J - K, "triplet": 1.1 - K}
    for flavour, want in closed.items():
        A = cis.cis_matrix(eps, u, 1, *cis.FLAVOURS[flavour])
        assert A.shape == (1, 1) and abs(A[0, 0] - want) <= 1e-15, flavour


def test_spin_doubled_spectrum_is_singlets_and_three_times_triplets():
    from oracle import qs_oracle as orc

    l, n = 6, 2
    h, u, s = ref.hermitian_problem(l, seed=21)
    _, eps, C = cis.scf_orbitals(h, u, s, n, 2.0, 1.0, -0.5)
    u_mo = cis.to_canonical(u, C)
    singlet, triplet = cis.spectrum(eps, u_mo, n, "singlet"), cis.spectrum(eps, u_mo, n, "triplet")
    want = np.sort(np.concatenate([singlet, triplet, triplet, triplet]))
    plain = orc.add_spin_two_body(u_mo)                       # spin orbital 2 p + sigma
    eps2 = np.repeat(eps, 2)
    np.testing.assert_allclose(cis.spectrum(eps2, plain, 2 * n, "gos_plain"), want, rtol=0, atol=1e-12)
    np.testing.assert_allclose(cis.spectrum(eps2, orc.anti_symmetrize_u(plain), 2 * n, "gos"), want, rtol=0, atol=1e-12)
