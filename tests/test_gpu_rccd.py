"""``coupled_cluster.RCCD`` on the GPU against the NumPy reference of tests/_rccd_ref.py (a full ``einsum`` transform and
the literal spin-summed residual; tests/test_rccd_ref_host.py pins that reference to the spin-orbital one of
tests/_ccd_ref.py), and against ``coupled_cluster.CCD`` on the spin-doubled, anti-symmetrised system.

Tolerances (derived, not tuned; those of tests/test_gpu_ccd.py):
  * one residual: the fp64 ``einsum`` reference deviates from its own ``numpy.longdouble`` evaluation by ``d`` on this
    input (measured in the test, before the device is looked at); the device, which does two more small transforms per
    term than the reference (it works on the untransformed tensor), may deviate by 4 d;
  * energies: every run stops at a residual below ``tol``, and an amplitude error of that order moves the energy by
    the same order at most: all energies, the reference's included, within 10 tol of one another."""

import numpy as np
import pytest
import torch

import _rccd_ref as rc

pytestmark = pytest.mark.gpu
TOL = 1e-9
E_NUC = 0.25
LS, NS = 5, 2


def H(x):
    return torch.as_tensor(x).cpu().numpy()


def spatial_system(ns, h, u):
    """2 ns particles in ns doubly occupied of the orthonormal spatial orbitals given as they are."""
    import quantum_systems_amd as qsa
    from quantum_systems_amd import hip

    l = h.shape[0]
    bs = qsa.setup_basis_set(2 * ns, l, hip.asarray(np.eye(l)), hip.asarray(h), hip.asarray(u), 2, -1, hip, False,
                             False, nuclear_repulsion_energy=E_NUC)
    return qsa.SpatialOrbitalSystem(2 * ns, bs)


def problem(l, seed, complex_u, complex_C=True):
    h, u, _ = rc.closed_shell_problem(l, seed, complex_=complex_u)
    _, _, C = rc.closed_shell_problem(l, seed + 1, complex_=complex_C)
    return h, u, C


@pytest.fixture(scope="module")
def residual_case():
    """(l_s, n_s) = (5, 2), complex u and C, seeded amplitudes with t[a,b,i,j] = t[b,a,j,i]: the long-double residual,
    and the fp64 reference's own deviation from it."""
    h, u, C = problem(LS, 41, True)
    t = rc.closed_shell_amplitudes(np.random.default_rng(9), LS - NS, NS, complex_=True)
    fw, utw = rc.orbital_tensors(h, u, C, NS, extended=True)
    wide = rc.residual(fw, utw, t.astype(np.clongdouble), NS)
    f, ut = rc.orbital_tensors(h, u, C, NS)
    own = float(np.abs(rc.residual(f, ut, t, NS) - wide).max())
    return h, u, C, t, f, wide, own


@pytest.mark.parametrize("ladder", ["exchange", "full"])
def test_one_residual_evaluation(residual_case, ladder):
    from quantum_systems_amd import RCCD, hip, kernels

    h, u, C, t, f, wide, own = residual_case
    assert np.abs(f - np.diag(np.diagonal(f))).max() > 1e-2                       # non-canonical orbitals
    ccd = RCCD(spatial_system(NS, h, u), hip.asarray(C), hip.asarray(np.real(np.diagonal(f)).copy()), ladder=ladder)
    kernels.dispatch_log = log = []
    try:
        R = H(ccd.residual(hip.asarray(t)))
    finally:
        kernels.dispatch_log = None
    got = float(np.abs(R - wide).max())
    print(f"ladder={ladder}: device deviation {got:.3e}, fp64 einsum reference {own:.3e}, ratio {got / own:.2f}")
    assert got <= 4 * own
    name = "pair_contract_exchange_kernel" if ladder == "exchange" else "pair_contract_kernel"
    passes = [e for e in log if "pair_contract" in e]
    assert len(passes) == 1 and name in passes[0]                                 # ONE pass over u


@pytest.mark.parametrize("complex_u", [True, False], ids=["complex", "real"])
def test_equal_energies_through_different_paths(complex_u):
    """RCCD with (C, eps) on both ladders, RCCD after change_basis, CCD on the spin-doubled anti-symmetrised system with
    kron(C, 1_2), and the reference; the alpha-beta-alpha-beta block of the converged spin-orbital amplitudes solves
    the closed-shell equations."""
    from quantum_systems_amd import CCD, RCCD, hip

    h, u, C = problem(LS, 23, complex_u, complex_C=complex_u)
    want, t_ref, its = rc.solve(h, u, C, NS, tol=1e-11)
    f, _ = rc.orbital_tensors(h, u, C, NS)
    e = np.real(np.diagonal(f)).copy()
    eps = hip.asarray(e)
    energies = {}
    for ladder in ("exchange", "full"):
        ccd = RCCD(spatial_system(NS, h, u), hip.asarray(C), eps, ladder=ladder)
        energies["C, " + ladder] = ccd.solve(tol=TOL)
        assert ccd.converged and ccd.residuals[-1] < TOL and len(ccd.residuals) == ccd.iterations + 1
        np.testing.assert_allclose(H(ccd.t), t_ref, atol=1e-7)
        if not complex_u:
            assert ccd._u.dtype == torch.float64 and ccd._t.dtype == torch.float64
    rccd = ccd
    moved = spatial_system(NS, h, u)
    moved.change_basis(hip.asarray(C))
    ccd = RCCD(moved)
    energies["change_basis"] = ccd.solve(tol=TOL)
    assert ccd.converged
    general = spatial_system(NS, h, u).construct_general_orbital_system(anti_symmetrize=True)
    so = CCD(general, hip.asarray(np.kron(C, np.eye(2))), hip.asarray(np.repeat(e, 2)))
    energies["spin-doubled CCD"] = so.solve(tol=TOL)
    assert so.converged
    print(f"reference {want:.12f} ({its} iterations): " + ", ".join(f"{k} {v:.12f}" for k, v in energies.items()))
    values = list(energies.values()) + [want]
    assert max(values) - min(values) <= 10 * TOL
    block = rc.block(H(so.t))
    if not complex_u and np.iscomplexobj(block):          # the spin-doubled system is complex, its amplitudes here are not
        assert np.abs(block.imag).max() <= TOL
        block = block.real
    norm = float(torch.linalg.vector_norm(rccd.residual(hip.asarray(np.ascontiguousarray(block)))).item())
    print(f"closed-shell residual of the spin-orbital block: {norm:.3e}")
    assert norm <= 2 * TOL


def test_zero_iterations_is_mp2():
    from quantum_systems_amd import RCCD, hip, mp2_energy

    h, u, C = problem(LS, 5, True)
    f, _ = rc.orbital_tensors(h, u, C, NS)
    eps = hip.asarray(np.real(np.diagonal(f)).copy())
    system = spatial_system(NS, h, u)
    ccd = RCCD(system, hip.asarray(C), eps)
    e0 = ccd.solve(max_iter=0)
    want = mp2_energy(system, hip.asarray(C), eps)
    print(f"RCCD at zero iterations {e0:.15f}, mp2_energy {want:.15f}")
    assert not ccd.converged and ccd.iterations == 0
    assert abs(e0 - want) <= 1e-13 * abs(want)


def test_refusals():
    import quantum_systems_amd as qsa
    from quantum_systems_amd import CCD, RCCD, hip
    from quantum_systems_amd.sharded_module import ShardedTensor4

    h, u, C = problem(6, 3, False, complex_C=False)
    system = spatial_system(2, h, u)
    with pytest.raises(TypeError, match="coupled_cluster.CCD"):
        RCCD(system.construct_general_orbital_system(anti_symmetrize=True))
    with pytest.raises(TypeError, match="construct_general_orbital_system"):
        CCD(system)                                                                 # as before
    for ns in (0, 6):
        with pytest.raises(ValueError, match="occupied"):
            RCCD(spatial_system(ns, h, u))
    with pytest.raises(AssertionError):
        qsa.SpatialOrbitalSystem(3, system._basis_set)                             # an odd particle number: no closed shell
    with pytest.raises(ValueError, match="both C and epsilon"):
        RCCD(system, hip.asarray(C))
    with pytest.raises(ValueError, match="ladder"):
        RCCD(system, ladder="antisym")
    with pytest.raises(ValueError):
        RCCD(system, hip.asarray(C[:, :4]), hip.asarray(np.zeros(4)))
    with pytest.raises(ValueError, match="mixing"):
        RCCD(system).solve(mixing=1.0)
    broken = u.copy()
    broken[0, 1, 2, 3] += 1e-9                                                      # u[0,1,2,3] != u[1,0,3,2]
    for ladder in ("exchange", "full"):
        with pytest.raises(ValueError, match="particle-exchange symmetry"):
            RCCD(spatial_system(2, h, broken), ladder=ladder)
    system._basis_set.u = ShardedTensor4(torch.as_tensor(system.u).as_subclass(torch.Tensor).contiguous(), 6, 0, 0, 1)
    with pytest.raises(NotImplementedError, match="one device"):
        RCCD(system)


def test_hartree_fock_entry_point_and_dispatch():
    import quantum_systems_amd as qsa
    from quantum_systems_amd import CCD, RCCD, HartreeFock, hip, kernels

    spatial = qsa.SpatialOrbitalSystem(2, qsa.ODQD(6, 8.0, 201, potential=qsa.ODQD.HOPotential(omega=1.0), np=hip))
    hf = HartreeFock(spatial)
    C, eps, _ = hf.scf(tol=1e-10)
    assert hf.converged
    ccd = hf.ccd()
    assert isinstance(ccd, RCCD) and ccd.ladder == "exchange"
    e = ccd.solve(tol=TOL)
    assert ccd.converged and e < 0.0
    kernels.dispatch_log = log = []
    try:
        ccd.residual()
    finally:
        kernels.dispatch_log = None
    passes = [entry for entry in log if "pair_contract" in entry]
    assert len(passes) == 1 and "qs::pair_contract_exchange_kernel<" in passes[0]  # one pass, the new kernel's
    assert abs(hf.ccd(ladder="full").solve(tol=TOL) - e) <= 10 * TOL

    general = spatial.construct_general_orbital_system(anti_symmetrize=True)
    ghf = HartreeFock(general)
    ghf.scf(tol=1e-10)
    so = ghf.ccd()
    assert isinstance(so, CCD)
    e_so = so.solve(tol=TOL)
    print(f"ODQD l = {spatial.l}, 2 electrons: MP2 {hf.mp2():.10f}, RHF -> RCCD {e:.10f} in {ccd.iterations} iterations, "
          f"GHF -> CCD {e_so:.10f}")
    assert so.converged and abs(e_so - e) <= 10 * TOL
    hf.change_system_basis()
    with pytest.raises(RuntimeError, match="coupled_cluster.RCCD"):
        hf.ccd()
    assert abs(RCCD(spatial).solve(tol=TOL) - e) <= 10 * TOL
