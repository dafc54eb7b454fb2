"""``coupled_cluster.CCD`` on the GPU against the NumPy reference of tests/_ccd_ref.py (a full ``einsum`` transform and
the literal residual; tests/test_ccd_ref_host.py pins that reference to the CID eigenvalue), and against
``DeterminantCI`` on {reference} + {doubles} for two particles.

Tolerances (derived, not tuned):
  * one residual: the fp64 ``einsum`` reference deviates from its own ``numpy.longdouble`` evaluation by ``d`` on this
    input (measured in the test, before the device is looked at); the device, which does two more small transforms per
    term than the reference (it works on the untransformed tensor), may deviate by 4 d;
  * energies: every run stops at a residual below ``tol``, and an amplitude error of that order moves the energy by
    the same order at most: all energies, the reference's included, within 10 tol of one another."""

import numpy as np
import pytest
import torch

import _ccd_ref as cc

pytestmark = pytest.mark.gpu
TOL = 1e-9
E_NUC = 0.25


def H(x):
    return torch.as_tensor(x).cpu().numpy()


def general_system(n, h, u, anti_symmetrized_u=True):
    """n particles on orthonormal spin orbitals given as they are (no spin doubling)."""
    import quantum_systems_amd as qsa
    from quantum_systems_amd import hip

    l = h.shape[0]
    bs = qsa.setup_basis_set(n, l, hip.asarray(np.eye(l)), hip.asarray(h), hip.asarray(u), 2, -1, hip, True,
                             anti_symmetrized_u, nuclear_repulsion_energy=E_NUC)
    return qsa.GeneralOrbitalSystem(n, bs, anti_symmetrize=False)


def problem(l, seed, complex_u, complex_C=True):
    h, u, _ = cc.antisymmetric_problem(l, seed, complex_=complex_u)
    _, _, C = cc.antisymmetric_problem(l, seed + 1, complex_=complex_C)
    return h, u, C


@pytest.fixture(scope="module")
def residual_case():
    """N = 4, l = 10, complex u and C, a seeded anti-symmetric t: the long-double residual, and the fp64 reference's own
    deviation from it."""
    l, n = 10, 4
    h, u, C = problem(l, 41, True)
    t = cc.antisymmetric_amplitudes(np.random.default_rng(9), l - n, n, complex_=True)
    fw, utw = cc.orbital_tensors(h, u, C, n, extended=True)
    wide = cc.residual(fw, utw, t.astype(np.clongdouble), n)
    f, ut = cc.orbital_tensors(h, u, C, n)
    own = float(np.abs(cc.residual(f, ut, t, n) - wide).max())
    return h, u, C, n, t, f, wide, own


@pytest.mark.parametrize("ladder", ["antisym", "full"])
def test_one_residual_evaluation(residual_case, ladder):
    from quantum_systems_amd import CCD, hip, kernels

    h, u, C, n, t, f, wide, own = residual_case
    assert np.abs(f - np.diag(np.diagonal(f))).max() > 1e-2                       # non-canonical orbitals
    ccd = CCD(general_system(n, h, u), hip.asarray(C), hip.asarray(np.real(np.diagonal(f)).copy()), ladder=ladder)
    kernels.dispatch_log = log = []
    try:
        R = H(ccd.residual(hip.asarray(t)))
    finally:
        kernels.dispatch_log = None
    got = float(np.abs(R - wide).max())
    print(f"ladder={ladder}: device deviation {got:.3e}, fp64 einsum reference {own:.3e}, ratio {got / own:.2f}")
    assert got <= 4 * own
    name = "pair_contract_antisym_kernel" if ladder == "antisym" else "pair_contract_kernel"
    passes = [e for e in log if "pair_contract" in e]
    assert len(passes) == 1 and name in passes[0]                                 # ONE pass over u


@pytest.mark.parametrize("complex_u", [True, False], ids=["complex_u", "real_u_complex_C"])
def test_equal_energies_through_different_paths(complex_u):
    from quantum_systems_amd import CCD, hip

    l, n = 10, 4
    h, u, C = problem(l, 23, complex_u)
    want, t_ref, its = cc.solve(h, u, C, n, tol=1e-11)
    f, _ = cc.orbital_tensors(h, u, C, n)
    eps = hip.asarray(np.real(np.diagonal(f)).copy())
    energies = {}
    for ladder in ("antisym", "full"):
        ccd = CCD(general_system(n, h, u), hip.asarray(C), eps, ladder=ladder)
        energies["C, " + ladder] = ccd.solve(tol=TOL)
        assert ccd.converged and ccd.residuals[-1] < TOL and len(ccd.residuals) == ccd.iterations + 1
        np.testing.assert_allclose(H(ccd.t), t_ref, atol=1e-7)
        if not complex_u:
            assert ccd._u.dtype == torch.float64                                  # a real u stays real
    moved = general_system(n, h, u)
    moved.change_basis(hip.asarray(C))
    ccd = CCD(moved)
    energies["change_basis"] = ccd.solve(tol=TOL)
    assert ccd.converged
    print(f"reference {want:.12f} ({its} iterations): " + ", ".join(f"{k} {v:.12f}" for k, v in energies.items()))
    values = list(energies.values()) + [want]
    assert max(values) - min(values) <= 10 * TOL


def test_two_particles_ccd_is_cid_on_the_device():
    from quantum_systems_amd import CCD, DeterminantCI, hip, truncated_space

    l, n = 8, 2
    h, u, C = problem(l, 77, True)
    system = general_system(n, h, u)
    f, ut = cc.orbital_tensors(h, u, C, n)
    ccd = CCD(system, hip.asarray(C), hip.asarray(np.real(np.diagonal(f)).copy()))
    e_ccd = ccd.solve(tol=TOL)
    assert ccd.converged
    ref = (1 << n) - 1
    dets = truncated_space(l, ref, 2)
    moved = np.array([bin(int(d) & ~ref).count("1") for d in dets])
    dets = dets[moved != 1]                                                         # the singles dropped: CID
    assert len(dets) == 1 + (l - n) * (l - n - 1) // 2
    ci = DeterminantCI(system, hip.asarray(C), dets=dets)
    E, _ = ci.solve(1, tol=TOL)
    e_ref = float(np.real(np.trace(f[:n, :n]) - 0.5 * np.einsum("ijij->", ut[:n, :n, :n, :n]))) + E_NUC
    e_cid = float(H(E)[0]) - e_ref
    print(f"CCD {e_ccd:.12f}, CID {e_cid:.12f}")
    assert abs(e_ccd - e_cid) <= 10 * TOL


def test_zero_iterations_is_mp2():
    from quantum_systems_amd import CCD, hip, mp2_energy

    l, n = 10, 4
    h, u, C = problem(l, 5, True)
    f, _ = cc.orbital_tensors(h, u, C, n)
    eps = hip.asarray(np.real(np.diagonal(f)).copy())
    system = general_system(n, h, u)
    ccd = CCD(system, hip.asarray(C), eps)
    e0 = ccd.solve(max_iter=0)
    want = mp2_energy(system, hip.asarray(C), eps)
    print(f"CCD at zero iterations {e0:.15f}, mp2_energy {want:.15f}")
    assert not ccd.converged and ccd.iterations == 0
    assert abs(e0 - want) <= 1e-13 * abs(want)


def test_refusals():
    import quantum_systems_amd as qsa
    from quantum_systems_amd import CCD, hip
    from quantum_systems_amd.sharded_module import ShardedTensor4

    h, u, C = problem(6, 3, False, complex_C=False)
    np.random.seed(2)
    spatial = qsa.SpatialOrbitalSystem(2, qsa.RandomBasisSet(4, 2))
    with pytest.raises(TypeError, match="construct_general_orbital_system"):
        CCD(spatial)
    with pytest.raises(ValueError, match="anti_symmetrize=True"):
        CCD(general_system(2, h, u, anti_symmetrized_u=False))
    for n in (0, 6):
        with pytest.raises(ValueError, match="occupied"):
            CCD(general_system(n, h, u))
    system = general_system(2, h, u)
    with pytest.raises(ValueError, match="both C and epsilon"):
        CCD(system, hip.asarray(C))
    with pytest.raises(ValueError, match="ladder"):
        CCD(system, ladder="half")
    with pytest.raises(ValueError):
        CCD(system, hip.asarray(C[:, :4]), hip.asarray(np.zeros(4)))
    system._basis_set.u = ShardedTensor4(torch.as_tensor(system.u).as_subclass(torch.Tensor).contiguous(), 6, 0, 0, 1)
    with pytest.raises(NotImplementedError, match="one device"):
        CCD(system)


def test_hartree_fock_entry_point_and_dispatch():
    import quantum_systems_amd as qsa
    from quantum_systems_amd import CCD, HartreeFock, hip, kernels

    spatial = qsa.SpatialOrbitalSystem(2, qsa.ODQD(6, 8.0, 201, potential=qsa.ODQD.HOPotential(omega=1.0), np=hip))
    system = spatial.construct_general_orbital_system(anti_symmetrize=True)
    hf = HartreeFock(system)
    C, eps, _ = hf.scf(tol=1e-10)
    assert hf.converged
    ccd = hf.ccd()
    e = ccd.solve(tol=TOL)
    kernels.dispatch_log = log = []
    try:
        ccd.residual()
    finally:
        kernels.dispatch_log = None
    assert sum("qs::pair_contract_antisym_kernel<" in entry for entry in log) == 1  # the pass is the new kernel's
    other = CCD(system, C, eps)
    assert ccd.converged and abs(other.solve(tol=TOL) - e) <= 1e-12 and e < 0.0
    print(f"ODQD l = {system.l}, n = {system.n}: MP2 {hf.mp2():.10f}, CCD {e:.10f} in {ccd.iterations} iterations")
    damped = ccd.solve(tol=TOL, mixing=0.5, max_iter=300)                          # the same fixed point, more slowly
    assert ccd.converged and abs(damped - e) <= 10 * TOL
    hf.change_system_basis()
    with pytest.raises(RuntimeError, match="coupled_cluster.CCD"):
        hf.ccd()
    assert abs(CCD(system).solve(tol=TOL) - e) <= 10 * TOL
