"""``two_particle.TwoParticleCI`` on the GPU against the dense two-particle Hamiltonian of tests/_two_particle_ref.py
(built from an explicitly transformed ``u``), and the 2-D quantum dot between its two analytic limits.

Tolerance (derived, not tuned): for a Hermitian matrix an eigenvalue lies within ||r|| of each Ritz value, so with the
Davidson ``tol = 1e-9`` the energies are asserted to ``1e-8 * max(1, max |lambda|)``; the factor 10 covers the rounding
of the sigma products.  Eigenvectors are checked through ``||H_dense c - E c||`` with the same bound."""

import re

import numpy as np
import pytest
import torch

import _mean_field_ref as mf
import _two_particle_ref as tp

pytestmark = pytest.mark.gpu
TOL = 1e-9
E_NUC = 0.25


def H(x):
    return torch.as_tensor(x).cpu().numpy() if not isinstance(x, (complex, float, np.ndarray, np.generic)) else x


def streaming_launches(entry):
    total = 0
    for part in entry.split(";"):
        if "qs::pair_contract_kernel<" in part:
            m = re.search(r" x(\d+)$", part.strip())
            total += int(m.group(1)) if m else 1
    return total


def group_of(entry):
    return int(re.search(r"qs::pair_contract_kernel<\d+, (\d+)>", entry).group(1))


def spatial_system(h, u, s):
    import quantum_systems_amd as qsa
    from quantum_systems_amd import hip

    return qsa.construct_custom_system(2, h.shape[0], hip.asarray(s), hip.asarray(h), hip.asarray(u), dim=2, np=hip,
                                       system_type="spatial", nuclear_repulsion_energy=E_NUC)


def check(solver, dense, n_roots, spin="singlet"):
    from quantum_systems_amd import kernels

    lam = np.linalg.eigvalsh(dense)
    kernels.dispatch_log = log = []
    try:
        E, c = solver.solve(n_roots, tol=TOL, spin=spin)
    finally:
        kernels.dispatch_log = None
    E, c = H(E), H(c)
    m = solver.m
    bound = 1e-8 * max(1.0, np.abs(lam).max())
    print(f"{type(solver.system).__name__} {spin} m={m}: max |dE| = {np.abs(E - E_NUC - lam[:n_roots]).max():.2e} (bound {bound:.1e}), "
          f"{solver.iterations} iterations, vectors per step {solver.sigma_history}, residuals {max(solver.residuals):.1e}")
    assert solver.converged and len(solver.residuals) == n_roots and max(solver.residuals) < TOL
    assert E.shape == (n_roots,) and c.shape == (n_roots, m, m) and (np.diff(E) >= 0).all()
    assert np.abs(E - E_NUC - lam[:n_roots]).max() <= bound
    sign = 1 if (spin == "singlet" and not solver._general) else -1
    np.testing.assert_allclose(c, sign * c.transpose(0, 2, 1), atol=1e-12)
    B = tp.pair_basis(m, sign).reshape(-1, m * m)
    for k in range(n_roots):
        x = B @ c[k].reshape(-1)
        assert abs(np.linalg.norm(x) - 1.0) <= 1e-12                              # unit norm, all of it inside the sector
        assert np.linalg.norm(dense @ x - (E[k] - E_NUC) * x) <= bound, k
    # each Davidson step is one pair_contract call of ceil(vectors / G) launches and nothing else
    mine = [e for e in log if "pair_contract" in e]
    assert len(mine) == len(log) == solver.iterations == len(solver.sigma_history)
    G = group_of(mine[0]) if solver.sigma_history[0] >= 4 else None
    for entry, nvec in zip(mine, solver.sigma_history):
        assert all("pair_contract_kernel" in part for part in entry.split(";") if part.strip()), entry
        if G:
            assert streaming_launches(entry) == -(-nvec // G), (entry, nvec)
    return E


CASES = {"real_l6": (6, False, False), "complex_l7": (7, True, True), "mixed_l6": (6, False, True)}


@pytest.mark.parametrize("case", list(CASES))
def test_against_the_dense_hamiltonian(case):
    from quantum_systems_amd import TwoParticleCI, hip

    l, cplx, cplx_C = CASES[case]
    h, u, s = mf.hermitian_problem(l, seed=300 + l, scale=0.2, complex_=cplx)
    if cplx_C and not cplx:                        # real u (and h), complex orbitals: the mixed form of the kernel
        b = np.random.default_rng(l).standard_normal((l, l))
        s = s + 0.05j * (b - b.T)
    X = tp.loewdin(s)
    assert np.abs(s - np.eye(l)).max() > 1e-2 and np.iscomplexobj(X) == cplx_C
    system = spatial_system(h, u, s)
    solver = TwoParticleCI(system, hip.asarray(X))
    es = check(solver, tp.dense_hamiltonian(h, u, X, +1), 3, "singlet")
    et = check(solver, tp.dense_hamiltonian(h, u, X, -1), 3, "triplet")
    assert solver._u.dtype == (torch.complex128 if cplx else torch.float64)        # a real u stays real
    assert es[0] != et[0]
    for anti in (True, False):
        gos = spatial_system(h, u, s).construct_general_orbital_system(anti_symmetrize=anti)
        h2, u2, C2, f = tp.spin_double(h, u, X, anti)
        np.testing.assert_allclose(H(gos.u), u2, atol=1e-14)                        # the oracle's spin order is the package's
        check(TwoParticleCI(gos, hip.asarray(C2)), tp.dense_hamiltonian(h2, u2, C2, -1, f), 3)


def test_full_space_and_identity_basis():
    from quantum_systems_amd import TwoParticleCI

    l = 3
    h, u, s = mf.hermitian_problem(l, seed=31, scale=0.2, complex_=True)
    system = spatial_system(h, u, np.eye(l))
    solver = TwoParticleCI(system)                                                  # s = 1: C = 1
    check(solver, tp.dense_hamiltonian(h, u, np.eye(l), +1), 6, "singlet")
    assert solver.iterations == 1 and solver.sigma_history == [6]
    check(solver, tp.dense_hamiltonian(h, u, np.eye(l), -1), 3, "triplet")
    # sigma is public: H c for any amplitude, the nuclear repulsion left out
    c = np.random.default_rng(0).standard_normal((2, l, l))
    got = H(solver.sigma(torch.from_numpy(c).cuda()))
    want = np.einsum("ac,kcb->kab", h, c) + np.einsum("kad,bd->kab", c, h) + np.einsum("abcd,kcd->kab", u, c)
    np.testing.assert_allclose(got, want, rtol=1e-12, atol=1e-12)
    np.testing.assert_allclose(H(solver.sigma(torch.from_numpy(c[1]).cuda())), want[1], rtol=1e-12, atol=1e-12)


def test_refusals():
    import quantum_systems_amd as qsa
    from quantum_systems_amd import TwoParticleCI, hip
    from quantum_systems_amd.sharded_module import ShardedTensor4

    h, u, s = mf.hermitian_problem(4, seed=5)
    with pytest.raises(ValueError, match="n = 2"):
        TwoParticleCI(qsa.construct_custom_system(4, 4, hip.asarray(s), hip.asarray(h), hip.asarray(u), dim=2, np=hip,
                                                  system_type="spatial"))
    system = spatial_system(h, u, s)
    with pytest.raises(ValueError, match="orthonormal"):
        TwoParticleCI(system)
    X = hip.asarray(tp.loewdin(s))
    with pytest.raises(ValueError):
        TwoParticleCI(system, hip.asarray(np.eye(5)))
    solver = TwoParticleCI(system, X)
    with pytest.raises(ValueError):
        solver.solve(2, spin="quintet")
    with pytest.raises(ValueError):
        solver.solve(11, spin="singlet")                                            # the singlet sector has 10 states
    with pytest.raises(ValueError):
        solver.solve(7, spin="triplet")
    gos = spatial_system(h, u, s).construct_general_orbital_system()
    with pytest.raises(ValueError, match="spin"):
        TwoParticleCI(gos, hip.asarray(np.kron(tp.loewdin(s), np.eye(2)))).solve(2, spin="triplet")
    with pytest.raises(TypeError):
        TwoParticleCI(object())
    plain = torch.as_tensor(system.u).as_subclass(torch.Tensor)
    system._basis_set.u = ShardedTensor4(plain.contiguous(), 4, 0, 0, 1)
    with pytest.raises(NotImplementedError, match="sharded"):
        TwoParticleCI(system, X)


def test_two_electrons_in_a_dot_lie_between_the_analytic_limits():
    """2-D harmonic dot, omega = 1, n = 2, l = 21 (six shells): the exact singlet ground state of the full problem is
    E = 3 (closed form) and the basis spans a subspace, so 3 < E; the RHF determinant lies in the singlet space, so
    E < E_RHF; the lowest triplet lies above the singlet ground state.  No fitted number."""
    import quantum_systems_amd as qsa
    from quantum_systems_amd import HartreeFock, TwoParticleCI, hip

    system = qsa.SpatialOrbitalSystem(2, qsa.TwoDimensionalHarmonicOscillator(21, 6.0, 41, omega=1.0, np=hip))
    hf = HartreeFock(system)
    C, eps, energies = hf.scf(tol=1e-10, max_iter=200)
    assert hf.converged
    e_rhf = float(np.real(H(energies[-1])))
    solver = TwoParticleCI(system, C)
    e_s = float(H(solver.solve(1, tol=TOL)[0])[0])
    assert solver.converged
    e_t = float(H(solver.solve(1, tol=TOL, spin="triplet")[0])[0])
    assert solver.converged
    print(f"E_RHF = {e_rhf:.8f}, exact singlet = {e_s:.8f}, exact triplet = {e_t:.8f}")
    assert 3.0 < e_s < e_rhf
    assert e_t > e_s
    own = float(H(TwoParticleCI(system).solve(1, tol=TOL)[0])[0])                   # the same state in the basis itself
    assert abs(own - e_s) <= 1e-8 * max(1.0, abs(e_s))
