"""What ``determinant_ci.DeterminantCI`` derives from the densities of its solved states -- ``transition_density``,
``two_body_density``, ``energy_from_densities``, ``expectation_one_body``, ``transition_dipole``, ``spin_squared``,
``natural_orbitals`` -- on small ``GeneralOrbitalSystem``s, against the Jordan-Wigner oracles of
tests/_det_ci_ref.py and tests/_det_ci_density_ref.py.

The systems of the energy and natural-orbital tests hold ``ht`` and the anti-symmetrised ``ut`` of
``_det_ci_ref.random_hamiltonian`` in an orthonormal basis (s = 1, C = None): the solver's transform by the identity is
exact, so the oracle's H is built from the very numbers the solver holds and the tolerances below cover everything.

Tolerances (derived, not tuned):
  * ``energy_from_densities``: sum ht rho + 1/4 sum ut G is a sum of m^2 + m^4 products of stored numbers with density
    elements that are themselves sums of at most dim products: gamma_(dim + m^4 + 4) (sum |ht||rho| + 1/4 sum |ut||G|),
    times 2 sqrt 2 when the vectors are complex; the exact value is c^H H c in ``numpy.longdouble``;
  * ``c_k^H H c_l`` for k != l, contracted on the host in long double from the computed densities: every density element
    is within ``pair_bound(c_k, c_l)`` = gamma_(dim+2) |c_k| |c_l| (2 sqrt 2) of the exact one, hence the value within
    pair_bound (sum |ht| + 1/4 sum |ut|).  The densities are also compared element by element (same bound): the value
    itself is near zero for eigenvectors whichever way round bra and ket are;
  * ``spin_squared`` of a non-degenerate eigenvector of a spin-independent H inside an S_z sector: the vector is within
    residual / gap <= 1e-9 / gap of a simultaneous eigenvector of S^2, and the expectation value of S^2 is stationary
    there, so the error is of second order (1e-18 / gap^2 times |S^2|) plus rounding (1e-13): 1e-8 holds with a wide
    margin for the gaps asserted below (> 1e-3).  Against the oracle's c^H S^2 c (fp64 on both sides):
    2 gamma_(dim + m^4 + 4) 2 sqrt 2 (sum |s2| + sum_i (sum |s_i|)^2);
  * natural orbitals: two solves with residuals below 1e-9 give vectors within 1e-9 / gap of the eigenvector each, a
    density is of first order in that (factor 2): 4e-9 / gap + 1e-12 per element; a Ritz value is of second order."""

import functools
from math import comb

import numpy as np
import pytest
import torch

import _det_ci_density_ref as dref
import _det_ci_ref as ref
import _mean_field_ref as mf
from test_gpu_det_ci import E_NUC, FORMS, H, TOL

pytestmark = pytest.mark.gpu
CF = 2.0 * np.sqrt(2.0)


@functools.lru_cache(maxsize=None)
def problem(m, N, cplx):
    """(ht, ut, position, H longdouble) of a seeded Hamiltonian and a Hermitian 2-d position stack; never modified."""
    ht, ut = ref.random_hamiltonian(m, 700 * m + N, cplx)
    rng = np.random.default_rng(m + N)
    x = rng.standard_normal((2, m, m)) + (1j * rng.standard_normal((2, m, m)) if cplx else 0.0)
    out = ht, ut, 0.5 * (x + x.conj().transpose(0, 2, 1)), ref.dense_hamiltonian(ht, ut, N, extended=True)
    for a in out:
        a.setflags(write=False)
    return out


def plain_system(m, N, cplx):
    """N particles on m orthonormal spin orbitals given as they are: s = 1, u anti-symmetrised already, no spin matrices."""
    import quantum_systems_amd as qsa
    from quantum_systems_amd import hip

    ht, ut, pos, _ = problem(m, N, cplx)
    bs = qsa.setup_basis_set(N, m, hip.asarray(np.eye(m)), hip.asarray(np.array(ht)), hip.asarray(np.array(ut)), 2, -1, hip,
                             True, True, nuclear_repulsion_energy=E_NUC, position=hip.asarray(np.array(pos)))
    return qsa.GeneralOrbitalSystem(N, bs, anti_symmetrize=False)


def spaces():
    from quantum_systems_amd import truncated_space

    full = ref.sector(8, 3)
    cisd = truncated_space(8, 0b00000111, 2)
    keep = np.searchsorted(full, cisd)
    assert (full[keep] == cisd).all() and 1 < len(cisd) < len(full)
    return [(7, 3, None), (8, 3, keep)]


def solved(m, N, keep, cplx, n_roots):
    from quantum_systems_amd import DeterminantCI

    dets = None if keep is None else ref.sector(m, N)[keep]
    solver = DeterminantCI(plain_system(m, N, cplx), dets=dets)
    solver.solve(n_roots, tol=TOL)
    assert solver.converged and solver.dim == (comb(m, N) if keep is None else len(keep))
    return solver


@pytest.mark.parametrize("form", list(FORMS))
def test_energy_from_densities_is_the_rayleigh_quotient(form):
    cplx = FORMS[form]
    for m, N, keep in spaces():
        ht, ut, _, Hx = problem(m, N, cplx)
        Hs = Hx if keep is None else Hx[np.ix_(keep, keep)]
        solver = solved(m, N, keep, cplx, 3)
        c = H(solver.c)
        assert c.dtype == (np.complex128 if cplx else np.float64)
        worst = 0.0
        for k in range(3):
            got = solver.energy_from_densities(k)
            assert isinstance(got, float)
            cw = ref._wide(c[k])
            want = (cw.conj() @ (Hs @ cw)).real + E_NUC
            rho, G = dref.jw_densities(c[k], c[k], m, N, keep)
            scale = float(np.sum(np.abs(ht) * np.abs(rho.T)) + 0.25 * np.sum(np.abs(ut) * np.abs(G)))
            tol = ref.gamma(solver.dim + m ** 4 + 4) * scale * (CF if cplx else 1.0)
            worst = max(worst, abs(got - float(want)) / tol)
            print(f"{form} m={m} N={N} dim={solver.dim} root {k}: |E[rho, G] - c H c| / bound = {abs(got - float(want)) / tol:.3f}, "
                  f"E[rho, G] - Ritz value = {got - float(H(solver.E)[k]):.2e}")
            assert abs(got - float(want)) <= tol
            assert abs(got - float(H(solver.E)[k])) <= 1e-8 * max(1.0, abs(got))       # the residual bounds this one


@pytest.mark.parametrize("form", list(FORMS))
def test_transition_densities_between_two_roots(form):
    cplx = FORMS[form]
    for m, N, keep in spaces():
        ht, ut, _, Hx = problem(m, N, cplx)
        Hs = Hx if keep is None else Hx[np.ix_(keep, keep)]
        solver = solved(m, N, keep, cplx, 3)
        c = H(solver.c)
        for k, l in ((0, 1), (1, 0), (2, 0)):
            rho, G = H(solver.transition_density(k, l)), H(solver.two_body_density(k, l))
            rho_x, G_x = dref.jw_densities(c[k], c[l], m, N, keep)
            bound = dref.pair_bound(c[k], c[l])
            e1, e2 = float(np.abs(rho - rho_x).max()), float(np.abs(G - G_x).max())
            got = dref.energy(ht, ut, ref._wide(rho), ref._wide(G))
            want = ref._wide(c[k]).conj() @ (Hs @ ref._wide(c[l]))
            tol = bound * float(np.sum(np.abs(ht)) + 0.25 * np.sum(np.abs(ut)))
            print(f"{form} m={m} N={N} ({k}, {l}): rho {e1 / bound:.3f}, G {e2 / bound:.3f} of the bound; c_k H c_l = {complex(got):.2e}, "
                  f"off the oracle by {abs(got - want) / tol:.3f} of its bound")
            assert e1 <= bound and e2 <= bound and abs(got - want) <= tol
            assert float(np.abs(G_x).max()) > 1e-3 and abs(complex(want)) < 1e-7       # large densities, a value near zero
        # two_body_density(k) is the state's density and one call of the new kernel (a memset is no kernel of the package)
        from quantum_systems_amd import kernels

        kernels.dispatch_log = log = []
        try:
            G = solver.two_body_density(1)
        finally:
            kernels.dispatch_log = None
        assert len(log) == 1
        parts = [p.strip() for p in log[0].split(";") if p.strip()]
        assert len(parts) == 1 and parts[0].startswith(f"qs::det_ci_density2_kernel<{2 if cplx else 1}>"), log
        G_x = dref.jw_densities(c[1], c[1], m, N, keep)[1]
        assert float(np.abs(H(G) - G_x).max()) <= dref.pair_bound(c[1], c[1])
        assert torch.equal(torch.as_tensor(solver.transition_density(1, 1)), torch.as_tensor(solver.one_body_density(1)))


# ---- spin and one-body observables: l = 4 spatial orbitals, spin-doubled, an orthonormal basis ---------------------------


@functools.lru_cache(maxsize=None)
def spatial_problem(cplx):
    """(h, u, position) of four orthonormal spatial orbitals; the overlap of ``hermitian_problem`` is dropped (s = 1),
    so that ``spin_2 = sum_i S_i s S_i`` IS the one-body part of S^2."""
    h, u, _ = mf.hermitian_problem(4, seed=404, scale=0.2, complex_=cplx)
    rng = np.random.default_rng(44)
    x = rng.standard_normal((2, 4, 4)) + (1j * rng.standard_normal((2, 4, 4)) if cplx else 0.0)
    out = h, u, 0.5 * (x + x.conj().transpose(0, 2, 1))
    for a in out:
        a.setflags(write=False)
    return out


def spin_system(cplx, n):
    import quantum_systems_amd as qsa
    from quantum_systems_amd import hip

    h, u, pos = spatial_problem(cplx)
    spatial = qsa.construct_custom_system(2, 4, hip.asarray(np.eye(4)), hip.asarray(np.array(h)), hip.asarray(np.array(u)),
                                          dim=2, np=hip, system_type="spatial", nuclear_repulsion_energy=E_NUC,
                                          position=hip.asarray(np.array(pos)))
    base = spatial.construct_general_orbital_system(anti_symmetrize=True)
    return qsa.GeneralOrbitalSystem(n, base._basis_set, anti_symmetrize=False)


@pytest.mark.parametrize("form", list(FORMS))
def test_spin_squared_in_every_sz_sector(form):
    from quantum_systems_amd import DeterminantCI, sz_sector

    cplx = FORMS[form]
    m, n = 8, 4
    system = spin_system(cplx, n)
    sx, sy, sz, s2 = (H(getattr(system, name)) for name in ("spin_x", "spin_y", "spin_z", "spin_2"))
    ht, ut = ref.orbital_hamiltonian(H(system.h), H(system.u), np.eye(m), True)
    full = ref.sector(m, n)
    Hd = ref.dense_hamiltonian(ht, ut, n)
    S2 = dref.spin_squared_matrix(sx, sy, sz, s2, m, n)
    weight = float(np.abs(s2).sum() + sum(np.abs(a).sum() ** 2 for a in (sx, sy, sz)))
    checked = 0
    for two_sz in (-4, -2, 0, 2, 4):
        dets = sz_sector(m, n, two_sz)
        keep = np.searchsorted(full, dets)
        lam = np.linalg.eigvalsh(Hd[np.ix_(keep, keep)])
        n_roots = min(len(dets), 4)
        solver = DeterminantCI(system, dets=dets)
        solver.solve(n_roots, tol=TOL)
        assert solver.converged
        c = H(solver.c)
        tol = 2 * ref.gamma(len(dets) + m ** 4 + 4) * CF * weight
        for k in range(n_roots):
            got = solver.spin_squared(k)
            want = (c[k].conj() @ (S2[np.ix_(keep, keep)] @ c[k])).real
            assert isinstance(got, float) and abs(got - want) <= tol, (two_sz, k, got, want)
            gaps = [abs(lam[k] - lam[j]) for j in (k - 1, k + 1) if 0 <= j < len(lam)]
            if gaps and min(gaps) <= 1e-3:
                continue                                                                # (nearly) degenerate: any mixture
            S = round((-1 + np.sqrt(1 + 4 * got)) / 2)
            print(f"{form} 2 S_z = {two_sz:+d} root {k}: <S^2> = {got:.12f}, S = {S}, off S (S + 1) by {abs(got - S * (S + 1)):.1e}; "
                  f"off the oracle by {abs(got - want) / tol:.3f} of the bound")
            assert S >= abs(two_sz) / 2 and abs(got - S * (S + 1)) <= 1e-8
            checked += 1
    assert checked >= 12                                                                # 1 + 4 + 4 + 4 + 1 roots, few skipped


@pytest.mark.parametrize("form", list(FORMS))
def test_dipoles_and_one_body_expectation_values(form):
    from quantum_systems_amd import DeterminantCI, sz_sector

    cplx = FORMS[form]
    m, n = 8, 4
    system = spin_system(cplx, n)
    dets = sz_sector(m, n, 0)
    keep = np.searchsorted(ref.sector(m, n), dets)
    solver = DeterminantCI(system, dets=dets)
    solver.solve(3, tol=TOL)
    c = H(solver.c)
    D = H(system.dipole_moment)
    assert D.shape == (2, m, m)
    for k, l in ((0, 0), (1, 1), (0, 1), (2, 1)):
        mu = H(solver.transition_dipole(k, l))
        rho_x = dref.jw_densities(c[k], c[l], m, n, keep)[0]
        want = np.array([np.sum(ref._wide(D[i]) * rho_x.T) for i in range(2)])
        tol = (dref.pair_bound(c[k].astype(np.complex128), c[l]) + ref.gamma(m * m + 2) * CF) * float(np.abs(D).sum(axis=(1, 2)).max())
        print(f"{form} dipole ({k}, {l}) = {mu}, off the oracle by {np.abs(mu - want).max() / tol:.3f} of the bound")
        assert mu.shape == (2,) and np.abs(mu - want).max() <= tol
        back = H(solver.transition_dipole(l, k))
        assert np.abs(mu - back.conj()).max() <= 2 * tol
        if k == l:
            assert np.array_equal(mu, H(solver.expectation_one_body(system.dipole_moment, k)))
            assert np.abs(mu.imag).max() <= tol                                         # a Hermitian operator
    one = H(solver.expectation_one_body(system.dipole_moment[1], 0, 1))                 # a single matrix
    assert one.shape == () and abs(one - H(solver.transition_dipole(0, 1))[1]) <= tol
    with pytest.raises(ValueError):
        solver.expectation_one_body(system.dipole_moment[:, :5, :5])


# ---- natural orbitals and errors ---------------------------------------------------------------------------------------------


@pytest.mark.parametrize("form", list(FORMS))
def test_natural_orbitals_diagonalise_the_density(form):
    from quantum_systems_amd import DeterminantCI

    cplx = FORMS[form]
    m, N = 7, 3
    lam = np.linalg.eigvalsh(problem(m, N, cplx)[3].astype(np.complex128 if cplx else np.float64))
    gap = lam[1] - lam[0]
    assert gap > 1e-3
    first = solved(m, N, None, cplx, 1)
    n, C_nat = first.natural_orbitals(0)
    n, C_host = H(n), H(C_nat)
    assert n.shape == (m,) and C_host.shape == (m, m) and (np.diff(n) <= 0).all()
    r_bound = m * dref.pair_bound(H(first.c)[0], H(first.c)[0])                         # eigenvalues move by at most |d rho|_2
    assert n.min() >= -r_bound and n.max() <= 1 + r_bound and abs(n.sum() - N) <= m * r_bound
    assert np.abs(C_host.conj().T @ C_host - np.eye(m)).max() <= 1e-13
    second = DeterminantCI(plain_system(m, N, cplx), C_nat)
    E2, _ = second.solve(1, tol=TOL)
    assert second.converged
    dE = abs(float(H(E2)[0]) - float(H(first.E)[0]))
    rho = H(second.one_body_density(0))
    tol = 4 * TOL / gap + 1e-12
    print(f"{form}: occupations {n}, |dE| = {dE:.1e}, |rho - diag(n)| = {np.abs(rho - np.diag(n)).max():.1e} (bound {tol:.1e})")
    assert dE <= 1e-10 and np.abs(rho - np.diag(n)).max() <= tol


def test_observables_need_a_solve_and_spin_matrices():
    from quantum_systems_amd import DeterminantCI

    system = plain_system(6, 3, False)
    solver = DeterminantCI(system)
    for call in (lambda: solver.transition_density(0, 0), lambda: solver.two_body_density(), lambda: solver.two_body_density(0, 0),
                 solver.energy_from_densities, lambda: solver.expectation_one_body(system.dipole_moment),
                 lambda: solver.transition_dipole(0, 0), solver.spin_squared, solver.natural_orbitals):
        with pytest.raises(RuntimeError, match="solve"):
            call()
    solver.solve(1, tol=TOL)
    assert system.spin_x is None
    with pytest.raises(ValueError, match="spin"):
        solver.spin_squared(0)
    assert H(solver.two_body_density()).shape == (6, 6, 6, 6) and H(solver.transition_dipole(0, 0)).shape == (2,)
