"""CPU-only checks of the mean-field entry (``qs_mean_field`` / ``qs_mean_field_workspace``): the workspace formula
the header documents, every refused argument (no GPU is touched: the checks run before any HIP call), and the pin of
the TESTS' oracle (tests/_mean_field_ref.py) to reference-generated numbers
(tests/golden/fock_energy_random_basis.npz)."""

import numpy as np
import pytest

import _mean_field_ref as ref

F64, C128 = 0, 1


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as entry

    entry.build()
    from quantum_systems_amd import _lib

    return _lib.load()


def documented_chunks(L, R, d_dtype):
    """include/qs_amd.h: Rc = min(ceil(R / min(ceil(4096 / L), R)), max(1, floor(2048 / (Le * dw))))."""
    cdiv = lambda a, b: -(-a // b)  # noqa: E731
    Le, dw = (L + 1) // 2 * 2, (2 if d_dtype == C128 else 1)
    Rc = min(cdiv(R, min(cdiv(4096, L), R)), max(1, 2048 // (Le * dw)))
    return cdiv(R, Rc)


@pytest.mark.parametrize("u_dtype,d_dtype", [(F64, F64), (C128, C128), (F64, C128)])
def test_workspace_is_rows_times_chunks(lib, u_dtype, d_dtype):
    es = 16 if d_dtype == C128 else 8
    for L, P, R in [(1, 1, 1), (5, 5, 5), (5, 2, 5), (31, 31, 7), (64, 64, 64), (96, 17, 96), (256, 256, 256),
                    (256, 32, 256), (256, 256, 32), (1024, 3, 1024)]:
        got = lib.qs_mean_field_workspace(u_dtype, d_dtype, L, P, R)
        assert got == P * L * documented_chunks(L, R, d_dtype) * es, (L, P, R)
        assert got == P * lib.qs_mean_field_workspace(u_dtype, d_dtype, L, 1, R)        # linear in P
    assert lib.qs_mean_field_workspace(C128, F64, 8, 8, 8) == -6
    assert lib.qs_mean_field_workspace(7, F64, 8, 8, 8) == -6
    assert lib.qs_mean_field_workspace(u_dtype, d_dtype, 0, 1, 1) == -1
    assert lib.qs_mean_field_workspace(u_dtype, d_dtype, 8, 9, 8) == -1
    assert lib.qs_mean_field_workspace(u_dtype, d_dtype, 8, 8, 9) == -1
    assert lib.qs_mean_field_workspace(u_dtype, d_dtype, 8, 8, 0) == -1


def test_refused_arguments_without_gpu(lib):
    # fake, well-separated device addresses: every call below returns before any HIP call is made
    u, D, W, work = 1 << 40, 2 << 40, 3 << 40, 4 << 40
    L, P, R = 8, 8, 8
    need = lib.qs_mean_field_workspace(F64, F64, L, P, R)

    def call(u_dtype=F64, d_dtype=F64, u=u, D=D, W=W, L=L, P=P, R=R, r_lo=0, work=work, nbytes=need):
        return lib.qs_mean_field(u_dtype, d_dtype, u, D, W, L, P, R, r_lo, 1.0, -0.5, work, nbytes, None)

    assert call(u=None) == -2 and call(D=None) == -2 and call(W=None) == -2 and call(work=None) == -2
    assert call(L=0) == -1 and call(L=-3) == -1
    assert call(P=0) == -1 and call(P=9) == -1 and call(R=0) == -1
    assert call(R=4, r_lo=5) == -1                       # r_lo + R > L
    assert call(R=4, r_lo=-1) == -1
    assert call(u_dtype=C128, d_dtype=F64) == -6         # complex u with a real D
    assert call(u_dtype=3) == -6 and call(d_dtype=-1) == -6
    assert call(nbytes=need - 1) == -4
    assert call(u=u + 4) == -3 and call(D=D + 4) == -3 and call(W=W + 4) == -3 and call(work=work + 8) == -3
    assert call(u_dtype=C128, d_dtype=C128, u=u + 8, nbytes=2 * need) == -3     # complex operands: 16 bytes
    assert call(W=u) == -7 and call(W=D) == -7 and call(W=work) == -7
    assert call(W=u + 8 * (P * R * L * L - 1)) == -7     # W starts inside u
    assert call(W=D - 8) == -7                           # W reaches into D


def test_error_strings_and_binding(lib):
    from quantum_systems_amd import _lib, kernels

    assert "qs_mean_field" in _lib.SIGNATURES and "qs_mean_field_workspace" in _lib.SIGNATURES
    assert lib.qs_abi_version() == 4
    import torch

    with pytest.raises(RuntimeError, match="GPU only"):
        kernels.mean_field(torch.zeros(3, 3, 3, 3, dtype=torch.float64), torch.zeros(3, 3, dtype=torch.float64))


def test_restatement_reproduces_reference_values(golden):
    # the numbers of the reference's own system classes, from formula (1) with the reference-determinant density
    from oracle import qs_oracle as orc

    g = golden("fock_energy_random_basis")
    l, n, e_nuc = int(g["l"]), int(g["n"]) // 2, float(g["e_nuc"])
    h, u = g["h"], g["u"]
    rho = ref.reference_density(l, n, 2.0)
    tol = dict(rtol=1e-11, atol=1e-11)               # the tolerance of tests/test_gpu_fock_energy.py
    np.testing.assert_allclose(ref.fock_from_density(h, u, rho, 1.0, -0.5), g["spas_fock"], **tol)
    np.testing.assert_allclose(ref.energy_from_density(h, u, rho, 1.0, -0.5, e_nuc), g["spas_energy"], **tol)

    C = g["C"]
    h_cb, u_cb = orc.transform_one_body(h, C), orc.transform_two_body(u, C)
    np.testing.assert_allclose(ref.fock_from_density(h_cb, u_cb, rho, 1.0, -0.5), g["spas_cb_fock"], **tol)
    np.testing.assert_allclose(ref.energy_from_density(h_cb, u_cb, rho, 1.0, -0.5, e_nuc), g["spas_cb_energy"], **tol)

    # spin orbitals: anti-symmetrised u carries the exchange (cj = 1, ck = 0); a plain u needs ck = -1
    h_gos = orc.add_spin_one_body(h).astype(np.complex128)
    u_plain = orc.add_spin_two_body(u)
    u_gos = orc.anti_symmetrize_u(u_plain)
    rho_gos = ref.reference_density(2 * l, 2 * n, 1.0)
    np.testing.assert_allclose(h_gos, g["gos_h"], **tol)
    np.testing.assert_allclose(ref.fock_from_density(h_gos, u_gos, rho_gos, 1.0, 0.0), g["gos_fock"], **tol)
    np.testing.assert_allclose(ref.fock_from_density(h_gos, u_plain, rho_gos, 1.0, -1.0), g["gos_fock"], **tol)
    np.testing.assert_allclose(ref.energy_from_density(h_gos, u_gos, rho_gos, 1.0, 0.0, e_nuc), g["gos_energy"], **tol)
    C2 = g["C_gos"]
    h2, u2 = orc.transform_one_body(h_gos, C2), orc.transform_two_body(u_gos, C2)
    np.testing.assert_allclose(ref.fock_from_density(h2, u2, rho_gos, 1.0, 0.0), g["gos_cb_fock"], **tol)
    np.testing.assert_allclose(ref.energy_from_density(h2, u2, rho_gos, 1.0, 0.0, e_nuc), g["gos_cb_energy"], **tol)

    # the second closed-shell case, rectangular change of basis 10 -> 8
    bl, bn = int(g["b_l"]), int(g["b_n"]) // 2
    Cb = g["b_C"]
    hb, ub = orc.transform_one_body(g["b_h"], Cb), orc.transform_two_body(g["b_u"], Cb)
    rho_b = ref.reference_density(Cb.shape[1], bn, 2.0)
    np.testing.assert_allclose(ref.fock_from_density(hb, ub, rho_b, 1.0, -0.5), g["b_cb_fock"], **tol)
    np.testing.assert_allclose(ref.energy_from_density(hb, ub, rho_b, 1.0, -0.5, float(g["b_e_nuc"])),
                               g["b_cb_energy"], **tol)
    assert bl == 10


def test_plain_scf_helper_lowers_the_core_guess_energy():
    h, u, s = ref.hermitian_problem(6, seed=5)
    e, e0, its = ref.plain_scf(h, u, s, 2, 2.0, 1.0, -0.5)
    assert e <= e0 + 1e-12 and its > 1
