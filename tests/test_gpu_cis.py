"""``configuration_interaction.CIS`` on the GPU against the dense NumPy CIS of tests/_cis_ref.py.

Tolerance of the excitation energies (derived, not tuned): a Ritz value of a Hermitian matrix whose residual 2-norm is
<= tol lies within tol of an eigenvalue.  The package's SCF and the reference's plain SCF both stop at a commutator of
tol_scf = 1e-10, so their orbitals agree to tol_scf / gap and the two CIS matrices to that times |u| l -- the slack
reasoning of ``_check_scf`` in tests/test_gpu_mean_field.py (a factor 100 covers gap >= 0.1 and |u| l <= 10: 1e-8).
With the Davidson tol = 1e-8 the sum stays below 1e-7 = 10 tol, which is what is asserted.  The residual ||A X - w X||
is taken with the dense A built on the PACKAGE's own orbitals (eigenvectors carry the orbitals' phases) and must be
<= 10 tol by the same reasoning."""

import ctypes

import numpy as np
import pytest
import torch

import _cis_ref as cis
import _mean_field_ref as ref

pytestmark = pytest.mark.gpu
TOL = 1e-8


def H(x):
    return torch.as_tensor(x).cpu().numpy() if not isinstance(x, (complex, float, np.ndarray, np.generic)) else x


def streaming_launches(entry):
    """Launches of the streaming kernel in one ``last_dispatch`` entry (repeats of a name are logged as ``name xN``)."""
    import re

    total = 0
    for part in entry.split(";"):
        if "qs::mean_field_batch_kernel<" in part:
            m = re.search(r" x(\d+)$", part.strip())
            total += int(m.group(1)) if m else 1
    return total


def group_size(system):
    from quantum_systems_amd import _lib

    u, h = torch.as_tensor(system.u), torch.as_tensor(system.h)
    cplx_u = u.is_complex()
    u_dtype, d_dtype = (1, 1) if cplx_u else (0, 1 if h.is_complex() else 0)
    out = (ctypes.c_int64 * 9)()
    assert _lib.load().qs_mean_field_batch_plan(u_dtype, d_dtype, system.l, system.l, system.l, 1,
                                                ctypes.cast(out, ctypes.c_void_p), 9) == 0
    return out[0]


def dense(system, C, eps, flavour):
    from quantum_systems_amd.array_module import to_host

    u_mo = cis.to_canonical(to_host(system.u), H(C))
    return cis.cis_matrix(np.asarray(H(eps)).real, u_mo, system.n, *cis.FLAVOURS[flavour])


def reference_spectrum(system, occupation, flavour):
    """The dense spectrum on the reference's OWN plain-SCF orbitals."""
    from quantum_systems_amd.array_module import to_host

    h, u, s = to_host(system.h), to_host(system.u), to_host(system.s)
    cj, ck = system._mean_field_weights()
    _, eps, C = cis.scf_orbitals(h, u, s, system.n, occupation, cj, ck, tol=1e-10)
    return cis.spectrum(eps, cis.to_canonical(u, C), system.n, flavour)


def solve_and_check(system, occupation, flavour, n_roots=5, spin="singlet"):
    from quantum_systems_amd import HartreeFock

    hf = HartreeFock(system)
    C, eps, _ = hf.scf(tol=1e-10, max_iter=200)
    assert hf.converged
    solver = hf.cis()
    omega, X = solver.solve(n_roots, tol=TOL, spin=spin)
    omega, X = H(omega), H(X)
    assert solver.converged and max(solver.residuals) < TOL and len(solver.residuals) == n_roots
    assert X.shape == (n_roots, system.n, system.l - system.n) and (np.diff(omega) >= 0).all()
    want = reference_spectrum(system, occupation, flavour)
    print(f"{flavour} l={system.l} n={system.n}: max |domega| = {np.abs(omega - want[:n_roots]).max():.2e}, "
          f"{solver.iterations} iterations, vectors per step {solver.sigma_history}")
    assert np.abs(omega - want[:n_roots]).max() <= 1e-7                 # the LOWEST n_roots, multiplicities included
    A = dense(system, C, eps, flavour)
    Xf = X.reshape(n_roots, -1)
    for k in range(n_roots):
        assert np.linalg.norm(A @ Xf[k] - omega[k] * Xf[k]) <= 10 * TOL, k
    np.testing.assert_allclose(Xf.conj() @ Xf.T, np.eye(n_roots), atol=1e-9)
    return omega, solver, hf


def spatial_problem(l, n, seed):
    """``n`` doubly occupied of ``l`` spatial orbitals (the system classes count particles: 2 n)."""
    import quantum_systems_amd as qsa
    from quantum_systems_amd import hip

    h, u, s = ref.hermitian_problem(l, seed=seed)
    return qsa.construct_custom_system(2 * n, l, hip.asarray(s), hip.asarray(h), hip.asarray(u), dim=2, np=hip,
                                       system_type="spatial", nuclear_repulsion_energy=0.25)


@pytest.mark.parametrize("l,n", [(8, 2), (12, 3)])
def test_cis_on_a_seeded_hermitian_problem(l, n):
    solve_and_check(spatial_problem(l, n, 200 + l), 2.0, "singlet")
    solve_and_check(spatial_problem(l, n, 200 + l), 2.0, "triplet", spin="triplet")
    solve_and_check(spatial_problem(l, n, 200 + l).construct_general_orbital_system(), 1.0, "gos")
    solve_and_check(spatial_problem(l, n, 200 + l).construct_general_orbital_system(anti_symmetrize=False), 1.0,
                    "gos_plain")


def test_one_pass_per_davidson_step():
    from quantum_systems_amd import HartreeFock, kernels

    system = spatial_problem(12, 3, 77)
    hf = HartreeFock(system)
    hf.scf(tol=1e-10)
    solver = hf.cis()
    G = group_size(system)
    kernels.dispatch_log = []
    try:
        solver.solve(5, tol=TOL)
        log = list(kernels.dispatch_log)
    finally:
        kernels.dispatch_log = None
    assert solver.converged and len(log) == solver.iterations == len(solver.sigma_history)
    for entry, new in zip(log, solver.sigma_history):
        assert streaming_launches(entry) == -(-new // G), (entry, new, G)
        assert "gemm" not in entry and "qs::mean_field_kernel" not in entry, entry
    assert solver.sigma_history[0] == 10 and max(solver.sigma_history[1:], default=0) <= 5


def test_one_dimensional_dot_energies_and_transition_moments():
    import quantum_systems_amd as qsa
    from quantum_systems_amd import HartreeFock, hip
    from quantum_systems_amd.array_module import to_host

    l, n, n_roots = 10, 1, 4
    system = qsa.SpatialOrbitalSystem(2 * n, qsa.ODQD(l, 10.0, 401, potential=qsa.ODQD.HOPotential(omega=0.5), np=hip))
    hf = HartreeFock(system)
    C, eps, _ = hf.scf(tol=1e-10, max_iter=200)
    solver = hf.cis()
    omega, X = solver.solve(n_roots, tol=TOL)
    mu = H(solver.transition_dipole_moments())
    assert mu.shape == (n_roots, 1)
    A = dense(system, C, eps, "singlet")
    w, Y = np.linalg.eigh(A)
    assert np.diff(w[:n_roots + 1]).min() > 1e-6                       # non-degenerate: eigenvectors defined up to a phase
    np.testing.assert_allclose(H(omega), w[:n_roots], rtol=0, atol=1e-7)
    Ch = H(C)
    x_mo = np.einsum("pa,dpq,qb->dab", Ch.conj(), to_host(system.position), Ch)
    want = cis.transition_moments(Y[:, :n_roots].T.reshape(n_roots, n, l - n), x_mo, n, np.sqrt(2.0))
    print("1-D dot: omega", H(omega), "|mu|", np.abs(mu[:, 0]))
    # |mu| moves by at most |x| * the eigenvector error, <= tol / (gap to the next root)
    np.testing.assert_allclose(np.abs(mu), np.abs(want), rtol=0, atol=1e-6)
    assert np.abs(mu).max() > 1e-3
    solver.solve(2, tol=TOL, spin="triplet")
    assert np.abs(H(solver.transition_dipole_moments())).max() == 0.0


def test_two_dimensional_dot_with_degenerate_shells():
    import quantum_systems_amd as qsa
    from quantum_systems_amd import HartreeFock, hip

    l, n = 15, 1
    system = qsa.SpatialOrbitalSystem(2 * n, qsa.TwoDimensionalHarmonicOscillator(l, 6.0, 41, omega=1.0, np=hip))
    hf = HartreeFock(system)
    C, eps, _ = hf.scf(tol=1e-10, max_iter=200)
    w = np.linalg.eigvalsh(dense(system, C, eps, "singlet"))
    cuts = [k for k in range(1, 9) if w[k] - w[k - 1] > 1e-4]          # n_roots = k cuts between w[k-1] and w[k]
    print("2-D dot: dense singlet spectrum", w[:10], "cuts", cuts)
    assert cuts, "no gap > 1e-4 among the nine lowest singlets"
    n_roots = max(cuts)
    omega, _ = hf.cis().solve(n_roots, tol=TOL)
    np.testing.assert_allclose(H(omega), w[:n_roots], rtol=0, atol=1e-7)


def test_consistency_between_the_system_kinds_and_bases():
    from quantum_systems_amd import CIS, HartreeFock, hip

    l, n = 8, 2
    system = spatial_problem(l, n, 321)
    hf = HartreeFock(system)
    C, eps, _ = hf.scf(tol=1e-10)
    no = n * (l - n)
    singlets, _ = hf.cis().solve(no, tol=TOL)
    triplets, _ = hf.cis().solve(no, tol=TOL, spin="triplet")
    want = np.sort(np.concatenate([H(singlets)] + [H(triplets)] * 3))
    gos = system.construct_general_orbital_system()
    C2 = torch.kron(torch.as_tensor(C), torch.eye(2, dtype=torch.complex128, device="cuda"))
    eps2 = torch.as_tensor(eps).repeat_interleave(2)
    both, _ = CIS(gos, hip.asarray(C2), hip.asarray(eps2)).solve(4 * no, tol=TOL)
    np.testing.assert_allclose(H(both), want, rtol=0, atol=1e-7)
    # C = None: the system in its own Hartree-Fock basis
    given, _ = hf.cis().solve(4, tol=TOL)
    hf.change_system_basis()
    own, _ = CIS(system).solve(4, tol=TOL)
    np.testing.assert_allclose(H(own), H(given), rtol=0, atol=1e-8)
    with pytest.raises(RuntimeError):
        hf.cis()


def test_guards():
    from quantum_systems_amd import CIS, HartreeFock, hip
    from quantum_systems_amd.sharded_module import ShardedTensor4

    system = spatial_problem(6, 2, 9)
    hf = HartreeFock(system)
    with pytest.raises(RuntimeError):
        hf.cis()
    C, eps, _ = hf.scf(tol=1e-10)
    with pytest.raises(ValueError):
        hf.cis().solve(2 * 4 + 1)
    with pytest.raises(ValueError):
        hf.cis().solve(0)
    with pytest.raises(ValueError):
        hf.cis().solve(2, spin="quintet")
    with pytest.raises(ValueError):
        CIS(system, C)
    gos = system.construct_general_orbital_system()
    ghf = HartreeFock(gos)
    ghf.scf(tol=1e-10)
    with pytest.raises(ValueError):
        ghf.cis().solve(2, spin="triplet")
    with pytest.raises(RuntimeError):
        hf.cis().transition_dipole_moments()
    # the stack form of the mean field on the system classes, and the sharded refusals
    rhos = hip.asarray(np.stack([ref.reference_density(6, 2, 2.0), np.eye(6)]))
    W = H(system.construct_mean_fields_from_densities(rhos))
    for k in range(2):
        np.testing.assert_allclose(W[k], H(system.construct_mean_field_from_density(rhos[k])), rtol=1e-12, atol=1e-12)
    u = torch.as_tensor(system.u).as_subclass(torch.Tensor)
    sharded_u = ShardedTensor4(u.contiguous(), 6, 0, 0, 1)
    with pytest.raises(NotImplementedError, match="sharded"):
        system.construct_mean_fields_from_densities(rhos, u=sharded_u)
    system._basis_set.u = sharded_u
    assert system.u is sharded_u
    with pytest.raises(NotImplementedError, match="sharded"):
        CIS(system, C, eps)
