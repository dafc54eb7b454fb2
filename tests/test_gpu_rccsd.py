"""``coupled_cluster.RCCSD`` on the GPU against the NumPy reference of tests/_ccsd_ref.py (a full ``einsum`` dressing and
the literal residuals; tests/test_ccsd_ref_host.py pins that reference to ``<mu| e^{-T} H e^{T} |0>`` on the Fock space,
to the determinant definition of (T) and to the exact two-electron energy).

Tolerances (derived, not tuned):
  * one residual: the margin of tests/test_gpu_rccd.py.  The fp64 ``einsum`` reference deviates from its own
    ``numpy.longdouble`` evaluation by ``d`` on this input (the larger of the two residuals', measured before the device
    is looked at); the device may deviate by 4 d.  Far inside 1e-11 of the largest residual element, which is asserted
    beside it;
  * energies: every run stops at a residual below ``tol``, and an amplitude error of that order moves the energy by the
    same order at most: all energies, the reference's included, within 10 tol of one another;
  * (T): the recipe of tests/test_gpu_triples.py for each part -- 16 times the difference of the fp64 working form
    from its long-double evaluation, plus ``kernel_bound`` (``singles_bound`` for the singles part) summed over the
    triples with their weights -- on the device's own amplitudes."""

import numpy as np
import pytest
import torch

import _ccsd_ref as cs
import _rccd_ref as rc
import _triples_ref as tr

pytestmark = pytest.mark.gpu
TOL = 1e-9
E_NUC = 0.25
SHAPES = [(6, 2, False), (7, 3, False), (7, 2, True)]
IDS = ["l6-o2-f64", "l7-o3-f64", "l7-o2-c128"]


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


def problem(l, ns, complex_, rotated, seed):
    """``(h, u, C, eps, ho, uo)``: the system's tensors, the orbitals (a random orthonormal non-Hartree-Fock ``C``, or
    None for the basis as it is), the diagonal of the Fock matrix in them, and the tensors in the orbitals."""
    h, u, _ = rc.closed_shell_problem(l, seed, complex_=complex_)
    if rotated:
        # (a smaller rotation than that of closed_shell_problem: the plain iteration with singles converges from it)
        rng = np.random.default_rng(seed + 1)
        g = 0.04 * (rng.standard_normal((l, l)) + (1j * rng.standard_normal((l, l)) if complex_ else 0.0))
        C = np.linalg.qr(np.eye(l) + g - g.conj().T)[0]
        ho, uo = cs.orbital_basis(h, u, C)
    else:
        C, ho, uo = None, h, u
    f, _ = rc.orbital_tensors(ho, uo, np.eye(l), ns)
    assert np.abs(f[ns:, :ns]).max() > 1e-2                                  # not Hartree-Fock orbitals: f_ai drives t1
    return h, u, C, np.real(np.diagonal(f)).copy(), ho, uo


def make(cls, ns, h, u, C, eps, **kw):
    from quantum_systems_amd import hip

    if C is None:
        return cls(spatial_system(ns, h, u), **kw)
    return cls(spatial_system(ns, h, u), hip.asarray(C), hip.asarray(eps), **kw)


def amplitudes(l, ns, complex_, seed):
    rng = np.random.default_rng(seed)
    t2 = rc.closed_shell_amplitudes(rng, l - ns, ns, complex_=complex_)
    t1 = 0.1 * rng.standard_normal((l - ns, ns))
    if complex_:
        t1 = t1 + 0.1j * rng.standard_normal((l - ns, ns))
    return t1, t2


@pytest.mark.parametrize("rotated", [True, False], ids=["C", "no-C"])
@pytest.mark.parametrize("l, ns, complex_", SHAPES, ids=IDS)
def test_one_residual_evaluation(l, ns, complex_, rotated):
    from quantum_systems_amd import RCCD, RCCSD, hip, kernels

    h, u, C, eps, ho, uo = problem(l, ns, complex_, rotated, 40 + l)
    t1, t2 = amplitudes(l, ns, complex_, 9)
    w1, w2 = cs.residuals(ho, uo, ns, t1, t2, extended=True)
    o1, o2 = cs.residuals(ho, uo, ns, t1, t2)
    own = max(float(np.abs(o1 - w1).max()), float(np.abs(o2 - w2).max()))
    top = max(float(np.abs(w1).max()), float(np.abs(w2).max()))
    ccsd = make(RCCSD, ns, h, u, C, eps)
    kernels.dispatch_log = log = []
    try:
        R1, R2 = ccsd.residual(hip.asarray(t1), hip.asarray(t2))
    finally:
        kernels.dispatch_log = None
    got = max(float(np.abs(H(R1) - w1).max()), float(np.abs(H(R2) - w2).max()))
    print(f"l = {l}, o = {ns}, {'complex' if complex_ else 'real'}, {'C' if rotated else 'no C'}: device deviation "
          f"{got:.3e}, fp64 einsum reference {own:.3e}, ratio {got / own:.2f}, largest element {top:.3e}")
    assert np.abs(w1).max() > 1e-2 and np.abs(w2).max() > 1e-2
    assert got <= 1e-11 * top
    assert got <= 4 * own
    passes = [e for e in log if "pair_contract" in e]
    assert len(passes) == 1 and "pair_contract_exchange_kernel" in passes[0]      # ONE pass over half of u
    if not complex_:
        assert R1.dtype == torch.float64 and R2.dtype == torch.float64

    # t1 = 0: the doubles residual of RCCD, and R1 = f_ai + the terms linear in t
    z1, z2 = cs.residuals(ho, uo, ns, np.zeros_like(t1), t2, extended=True)
    f, ut = rc.orbital_tensors(ho, uo, np.eye(l), ns, extended=True)
    plain = rc.residual(f, ut, rc._wide(t2), ns)
    assert float(np.abs(z2 - plain).max()) <= 1e-17 * top                         # (the reference: the same formula)
    d0 = float(np.abs(rc.residual(*rc.orbital_tensors(ho, uo, np.eye(l), ns), t2, ns) - plain).max())
    S1, S2 = ccsd.residual(hip.asarray(np.zeros_like(t1)), hip.asarray(t2))
    doubles = H(make(RCCD, ns, h, u, C, eps).residual(hip.asarray(t2)))
    print(f"t1 = 0: RCCSD {np.abs(H(S2) - plain).max():.3e}, RCCD {np.abs(doubles - plain).max():.3e}, reference {d0:.3e}")
    assert float(np.abs(H(S2) - plain).max()) <= 4 * d0 and float(np.abs(doubles - plain).max()) <= 4 * d0
    assert float(np.abs(H(S2) - doubles).max()) <= 8 * d0
    assert float(np.abs(H(S1) - z1).max()) <= 4 * max(d0, float(np.abs(cs.residuals(ho, uo, ns, 0 * t1, t2)[0] - z1).max()))


@pytest.mark.parametrize("rotated", [True, False], ids=["C", "no-C"])
@pytest.mark.parametrize("l, ns, complex_", SHAPES, ids=IDS)
def test_solve_against_the_reference(l, ns, complex_, rotated):
    from quantum_systems_amd import RCCD, RCCSD

    h, u, C, eps, ho, uo = problem(l, ns, complex_, rotated, 20 + l)
    want, t1_ref, t2_ref, its = cs.solve(ho, uo, ns, tol=1e-11)
    ccsd = make(RCCSD, ns, h, u, C, eps)
    got = ccsd.solve(tol=TOL, max_iter=200)
    doubles = make(RCCD, ns, h, u, C, eps).solve(tol=TOL, max_iter=200)
    print(f"reference {want:.12f} ({its} iterations), device {got:.12f} ({ccsd.iterations}), RCCD {doubles:.12f}")
    assert ccsd.converged and ccsd.residuals[-1] < TOL and len(ccsd.residuals) == ccsd.iterations + 1
    assert abs(got - want) <= 10 * TOL
    assert abs(got - doubles) > 1e-4                                              # singles matter in these orbitals
    np.testing.assert_allclose(H(ccsd.t1), t1_ref, atol=1e-7)
    np.testing.assert_allclose(H(ccsd.t), t2_ref, atol=1e-7)
    assert abs(ccsd.energy() - got) == 0.0
    if not complex_:
        assert ccsd._t1.dtype == torch.float64 and ccsd._t.dtype == torch.float64


@pytest.mark.parametrize("complex_", [False, True], ids=["real", "complex"])
def test_two_electrons_are_exact(complex_):
    from quantum_systems_amd import RCCD, RCCSD

    l, ns = 6, 1
    h, u, C, eps, ho, uo = problem(l, ns, complex_, False, 7)
    exact = cs.two_electron_ground_state(h, u)
    e_ref = float(np.real(cs.reference_energy(h, u, ns)))
    ccsd = make(RCCSD, ns, h, u, None, None)
    got = ccsd.solve(tol=TOL)
    doubles = make(RCCD, ns, h, u, None, None).solve(tol=TOL)
    print(f"E_ref {e_ref:.12f} + E_CCSD {got:.12f} = {e_ref + got:.12f}, exact {exact:.12f}; with CCD {e_ref + doubles:.12f}")
    assert ccsd.converged and abs(e_ref + got - exact) <= 10 * TOL
    assert abs(e_ref + doubles - exact) > 1e-6                                    # CCD is not


# -- (T)


def triples_reference(u, eps, ns, t1, t2):
    """The long-double working form of both parts and the tolerance of the module docstring for each."""
    wide, wide_s = (float(x) for x in cs.pt_working(u, eps, ns, t1, t2, extended=True))
    own, own_s = cs.pt_working(u, eps, ns, t1, t2)
    X = tr.packed_blocks(tr.blocks(u, ns, t2))
    A, G = cs.singles_factors(u, ns, t1)
    todo = tr.triples(ns)
    slots = np.array([tr.slot_row(ns, *ijk) for ijk in todo])
    sslots = np.array([cs.singles_slot_row(ns, *ijk) for ijk in todo])
    eo3 = np.array([eps[i] + eps[j] + eps[k] for i, j, k in todo])
    weights = np.array([tr.weight(*ijk) for ijk in todo])
    summed = float((weights * tr.kernel_bound(X, slots, eo3, eps[ns:])).sum())
    summed_s = float((weights * cs.singles_bound(X, slots, A, G, sslots, eo3, eps[ns:])).sum())
    return wide, wide_s, 16 * abs(float(own) - wide) + summed, 16 * abs(float(own_s) - wide_s) + summed_s, summed + summed_s


@pytest.fixture(scope="module")
def solved():
    """Canonical problems (l, o) = (6, 2) complex and (7, 3) real, the device's own converged amplitudes and (T)."""
    from quantum_systems_amd import RCCSD

    out = {}
    for l, ns, complex_ in ((6, 2, True), (7, 3, False)):
        h, u, eps = tr.canonical_problem(l, ns, 50 + l, complex_=complex_)
        ccsd = RCCSD(spatial_system(ns, h, u))
        ccsd.solve(tol=TOL)
        assert ccsd.converged
        out[l] = (ns, u, eps, ccsd, ccsd.triples(), tuple(ccsd.triples_parts), list(ccsd.triples_passes))
    return out


@pytest.mark.parametrize("l", [6, 7])
def test_triples_against_working_form(solved, l):
    ns, u, eps, ccsd, got, parts, passes = solved[l]
    t1, t2 = H(ccsd.t1), H(ccsd.t)
    assert np.abs(t1).max() > 1e-4                                                # the doubles drive singles
    wide, wide_s, tol, tol_s, _ = triples_reference(u, eps, ns, t1, t2)
    print(f"l = {l}, o = {ns}: E_[T] {parts[0]:.15e} (reference {wide:.15e}, deviation {abs(parts[0] - wide):.3e}, tolerance "
          f"{tol:.3e}), E_ST {parts[1]:.15e} (reference {wide_s:.15e}, deviation {abs(parts[1] - wide_s):.3e}, tolerance "
          f"{tol_s:.3e})")
    assert isinstance(got, float) and got == parts[0] + parts[1]
    assert abs(parts[0] - wide) <= tol and abs(parts[1] - wide_s) <= tol_s
    assert abs(wide) > 1e6 * tol and abs(wide_s) > 1e3 * tol_s                    # the tolerances are checks
    assert len(passes) == 1 and passes[0][:2] == (len(tr.triples(ns)), ns ** 3)
    assert "qs::triples_energy_singles_kernel" in passes[0][2] and "qs::triples_energy_kernel" not in passes[0][2]
    # the connected part is RCCD's correction on the same doubles
    from quantum_systems_amd import RCCD

    h, _, _ = tr.canonical_problem(l, ns, 50 + l, complex_=np.iscomplexobj(u))
    plain = RCCD(spatial_system(ns, h, u)).triples(ccsd.t)
    assert abs(plain - wide) <= tol


def test_passes_under_a_small_budget(solved):
    from quantum_systems_amd import kernels

    l = 7
    ns, u, eps, ccsd, one, parts, _ = solved[l]
    _, _, _, _, summed = triples_reference(u, eps, ns, H(ccsd.t1), H(ccsd.t))
    block = (l - ns) ** 3 * 8
    with kernels.tuning(triples_bytes=3 * block):                                 # one triple per pass
        passes = ccsd.triples()
        record, passes_parts = list(ccsd.triples_passes), tuple(ccsd.triples_parts)
    with kernels.tuning(triples_bytes=13 * block):                                # groups of several triples
        groups = ccsd.triples()
        assert 1 < len(ccsd.triples_passes) < len(record) and all(p[1] <= 13 for p in ccsd.triples_passes)
    todo = tr.triples(ns)
    print(f"one launch {one:.15e}, one triple per pass {passes:.15e}, groups {groups:.15e}, summed bounds {summed:.3e}")
    assert [p[:2] for p in record] == [(1, len(set(tr.slot_row(ns, *ijk)))) for ijk in todo]
    assert all("qs::triples_energy_singles_kernel<1>" in p[2] for p in record)
    assert abs(passes - one) <= summed and abs(groups - one) <= summed
    assert abs(passes_parts[1] - parts[1]) <= summed and passes_parts[1] != 0.0


def test_refusals_and_hartree_fock_entry_point():
    import quantum_systems_amd as qsa
    from quantum_systems_amd import RCCSD, HartreeFock, hip

    l, ns = 6, 2
    h, u, C, eps, _, _ = problem(l, ns, False, True, 3)                           # a rotated, non-canonical C
    ccsd = make(RCCSD, ns, h, u, C, eps)
    with pytest.raises(ValueError, match="RCCSD.triples needs canonical"):
        ccsd.triples()
    with pytest.raises(ValueError, match="v, o"):
        ccsd.residual(hip.asarray(np.zeros((ns, l - ns))), None)
    with pytest.raises(ValueError, match="mixing"):
        ccsd.solve(mixing=1.0)
    with pytest.raises(ValueError, match="both C and epsilon"):
        RCCSD(spatial_system(ns, h, u), hip.asarray(C))
    with pytest.raises(TypeError, match="SpatialOrbitalSystem"):
        RCCSD(spatial_system(ns, h, u).construct_general_orbital_system(anti_symmetrize=True))

    spatial = qsa.SpatialOrbitalSystem(4, qsa.ODQD(8, 8.0, 201, potential=qsa.ODQD.HOPotential(omega=1.0), np=hip))
    hf = HartreeFock(spatial)
    hf.scf(tol=1e-10)
    assert hf.converged
    ccsd = hf.ccsd()
    assert isinstance(ccsd, RCCSD) and ccsd.ladder == "exchange"
    e = ccsd.solve(tol=TOL)
    e_t = ccsd.triples()
    e_ccd = hf.ccd().solve(tol=TOL)
    print(f"ODQD l = 8, 4 electrons: RCCD {e_ccd:.10f}, RCCSD {e:.10f}, (T) {e_t:.3e} = {ccsd.triples_parts}")
    assert ccsd.converged and e < 0.0 and abs(e - e_ccd) < 0.1 * abs(e_ccd) and e != e_ccd
    assert e_t < 0.0 and abs(e_t) < abs(e)
    with pytest.raises(TypeError, match="SpatialOrbitalSystem"):
        HartreeFock(spatial.construct_general_orbital_system(anti_symmetrize=True)).ccsd()
