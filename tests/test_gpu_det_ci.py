"""``kernels.det_ci_diagonal`` / ``det_ci_sigma`` / ``det_ci_density1`` and ``determinant_ci.DeterminantCI`` on the GPU
against the dense Hamiltonian of tests/_det_ci_ref.py (Jordan-Wigner matrices: no Slater-Condon rule is shared with the
kernels).

Tolerances (derived, not tuned):
  * sigma: |sigma - sigma_exact| <= gamma_(n+2) (|H| |c|) elementwise, n = 1 + N (m - N) + C(N,2) C(m-N,2) + N terms,
    sigma_exact from the oracle in ``numpy.longdouble``, a factor 2 sqrt 2 for complex products
    (``_det_ci_ref.error_bound``);
  * the diagonal: a sum of N + C(N,2) stored numbers, gamma_(N + C(N,2)) times the sum of their moduli;
  * the density: a sum of at most dim products c*_I c_J, gamma_(dim+2) |c|^2 (``_det_ci_ref.density_bound``);
  * the solver: for a Hermitian matrix an eigenvalue lies within ||r|| of each Ritz value, so with the Davidson
    ``tol = 1e-9`` the energies are asserted to ``1e-8 * max(1, max |lambda|)``; the factor 10 covers the rounding of
    the sigma products (the reasoning of tests/test_gpu_two_particle.py).  ``||H_dense c - E c||`` has the same bound.
    A solve that stops early still gives upper bounds: Ritz values of a subspace interlace the spectrum from above.
Larger spaces, orbital indices up to 62 and padded rows of ``c`` are in tests/test_gpu_det_ci_scale.py.
Every comparison prints its worst ratio to the bound before it asserts."""

import functools
import re
from math import comb

import numpy as np
import pytest
import torch

import _det_ci_ref as ref
import _mean_field_ref as mf

pytestmark = pytest.mark.gpu
TOL = 1e-9
E_NUC = 0.25
SHAPES = [(4, 2), (6, 3), (7, 3), (8, 4), (7, 1), (7, 6), (5, 5)]                 # dims 6, 20, 35, 70, 7, 7, 1
FORMS = {"fp64": False, "complex128": True}


def H(x):
    return torch.as_tensor(x).cpu().numpy() if not isinstance(x, (complex, float, np.ndarray, np.generic)) else x


def dev(x):
    return torch.from_numpy(np.array(x)).cuda()                                    # a copy: the cached problems are read-only


@functools.lru_cache(maxsize=None)
def problem(m, N, cplx):
    """(ht, ut, masks, H fp64, H longdouble) of a seeded Hamiltonian; computed once, never modified."""
    ht, ut = ref.random_hamiltonian(m, 100 * m + N, cplx)
    out = ht, ut, ref.sector(m, N), ref.dense_hamiltonian(ht, ut, N), ref.dense_hamiltonian(ht, ut, N, extended=True)
    for a in out:
        a.setflags(write=False)
    return out


def vectors(K, dim, cplx, seed):
    rng = np.random.default_rng(seed)
    c = rng.standard_normal((K, dim))
    return c + 1j * rng.standard_normal((K, dim)) if cplx else c


def launches(entry):
    total = 0
    for part in entry.split(";"):
        if "qs::det_ci_sigma_kernel<" in part:
            hit = re.search(r" x(\d+)$", part.strip())
            total += int(hit.group(1)) if hit else 1
    return total


def shipped_group(cplx):
    """G of the form, read from what a 16-vector call launches."""
    from quantum_systems_amd import kernels

    ht, ut, dets, Hd, _ = problem(4, 2, cplx)
    kernels.dispatch_log = log = []
    try:
        run_sigma(ht, ut, dets, 2, vectors(16, 6, cplx, 0))
    finally:
        kernels.dispatch_log = None
    entry = [e for e in log if "det_ci_sigma" in e][-1]
    return max(int(g) for g in re.findall(r"qs::det_ci_sigma_kernel<\d+, (\d+)>", entry))


def run_sigma(ht, ut, dets, N, c, **kw):
    from quantum_systems_amd import kernels

    d_ht, d_ut, d_dets = dev(ht), dev(ut), dev(dets)
    diag = kernels.det_ci_diagonal(d_ht, d_ut, d_dets, N)
    return H(kernels.det_ci_sigma(d_ht, d_ut, d_dets, N, diag, dev(c), **kw))


def check_sigma(got, Hx, Hd, c, m, N, what):
    exact = ref.sigma(Hx, c, extended=True)
    bound = ref.error_bound(Hd, c, m, N)
    err = np.abs(got - exact).astype(np.float64)
    ratio = float((err / np.where(bound > 0, bound, 1.0)).max())
    print(f"{what}: worst |sigma - exact| / bound = {ratio:.3f}")
    assert (err <= bound).all(), what
    return ratio


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"m{s[0]}_N{s[1]}")
@pytest.mark.parametrize("form", list(FORMS))
def test_sigma_diagonal_and_density_against_the_dense_oracle(form, shape):
    from quantum_systems_amd import kernels

    cplx = FORMS[form]
    m, N = shape
    ht, ut, dets, Hd, Hx = problem(m, N, cplx)
    dim = len(dets)
    assert dim == comb(m, N)
    d_ht, d_ut, d_dets = dev(ht), dev(ut), dev(dets)

    # the diagonal
    D = H(kernels.det_ci_diagonal(d_ht, d_ut, d_dets, N))
    assert D.dtype == np.float64 and D.shape == (dim,)
    occ = [[p for p in range(m) if x >> p & 1] for x in dets.tolist()]
    moduli = np.array([sum(abs(ht[p, p].real) for p in o) + sum(abs(ut[p, q, p, q].real) for p in o for q in o if p < q)
                       for o in occ])
    d_bound = ref.gamma(N + comb(N, 2)) * moduli
    d_err = np.abs(D - np.diag(Hx).real).astype(np.float64)
    print(f"{form} m={m} N={N}: worst |D - exact| / bound = {(d_err / d_bound).max():.3f}")
    assert (d_err <= d_bound).all()

    # sigma for K = 1, G - 1, G, G + 1, 2 G + 3
    G = shipped_group(cplx)
    for K in (1, G - 1, G, G + 1, 2 * G + 3):
        c = vectors(K, dim, cplx, 1000 + K)
        kernels.dispatch_log = log = []
        try:
            got = run_sigma(ht, ut, dets, N, c)
        finally:
            kernels.dispatch_log = None
        assert got.shape == (K, dim) and got.dtype == (np.complex128 if cplx else np.float64)
        check_sigma(got, Hx, Hd, c, m, N, f"{form} m={m} N={N} K={K}")
        assert launches([e for e in log if "det_ci_sigma" in e][-1]) == -(-K // G)
    one = run_sigma(ht, ut, dets, N, c[0])                                          # a 1-D vector
    assert one.shape == (dim,) and np.array_equal(one, got[0])

    # the one-body density of one normalised vector
    v = vectors(1, dim, cplx, 7)[0]
    v = v / np.linalg.norm(v)
    rho = H(kernels.det_ci_density1(d_dets, dev(v), m, N))
    exact = ref.one_body_density(v, m, N)
    r_bound = ref.density_bound(v, m, N)
    r_err = float(np.abs(rho - exact).max())
    print(f"{form} m={m} N={N}: worst |rho - exact| / bound = {r_err / r_bound:.3f}")
    assert rho.shape == (m, m) and r_err <= r_bound
    assert abs(np.trace(rho) - N) <= m * r_bound and np.abs(rho - rho.conj().T).max() <= 2 * r_bound


@pytest.mark.parametrize("form", list(FORMS))
def test_bits_do_not_depend_on_the_batch_or_the_group(form):
    from quantum_systems_amd import kernels

    cplx = FORMS[form]
    for m, N in ((7, 3), (8, 4), (4, 2)):
        ht, ut, dets, _, _ = problem(m, N, cplx)
        dim = len(dets)
        c = vectors(19, dim, cplx, 5)
        base = run_sigma(ht, ut, dets, N, c)
        assert np.array_equal(base, run_sigma(ht, ut, dets, N, c))                 # repeatable
        for k in (0, 7, 8, 18):
            assert np.array_equal(run_sigma(ht, ut, dets, N, c[k:k + 1])[0], base[k]), k
        assert np.array_equal(run_sigma(ht, ut, dets, N, c[::-1].copy()), base[::-1])
        assert np.array_equal(run_sigma(ht, ut, dets, N, c[3:14])[4], base[7])
        for g in (1, 2, 4, 8):
            with kernels.tuning(det_ci_g=g):
                kernels.dispatch_log = log = []
                try:
                    got = run_sigma(ht, ut, dets, N, c)
                finally:
                    kernels.dispatch_log = None
            assert np.array_equal(got, base), g
            assert launches([e for e in log if "det_ci_sigma" in e][-1]) == -(-19 // g)


@pytest.mark.parametrize("form", list(FORMS))
def test_bytes_around_the_outputs_are_untouched(form):
    from quantum_systems_amd import kernels

    cplx = FORMS[form]
    dt = torch.complex128 if cplx else torch.float64
    pad, mark = 64, 7.25
    for m, N in ((7, 3), (8, 4), (5, 5)):
        ht, ut, dets, Hd, _ = problem(m, N, cplx)
        dim, K = len(dets), 11
        d_ht, d_ut, d_dets = dev(ht), dev(ut), dev(dets)

        def framed(n, dtype):
            buf = torch.full((n + 2 * pad,), mark, dtype=dtype, device="cuda")
            return buf, buf[pad:pad + n]

        buf_d, out_d = framed(dim, torch.float64)
        kernels.det_ci_diagonal(d_ht, d_ut, d_dets, N, out=out_d)
        buf_s, out_s = framed(K * dim, dt)
        c = vectors(K, dim, cplx, 9)
        kernels.det_ci_sigma(d_ht, d_ut, d_dets, N, out_d, dev(c), out=out_s.view(K, dim))
        buf_r, out_r = framed(m * m, dt)
        kernels.det_ci_density1(d_dets, dev(c[0]), m, N, out=out_r.view(m, m))
        for buf, n in ((buf_d, dim), (buf_s, K * dim), (buf_r, m * m)):
            b = H(buf)
            assert (b[:pad] == mark).all() and (b[pad + n:] == mark).all()
        np.testing.assert_allclose(H(out_s).reshape(K, dim), c @ Hd.T, rtol=1e-11, atol=1e-11)
        assert np.array_equal(H(out_d), H(kernels.det_ci_diagonal(d_ht, d_ut, d_dets, N)))


@pytest.mark.parametrize("form", list(FORMS))
def test_a_subset_is_the_projection_of_the_full_space(form):
    from quantum_systems_amd import truncated_space

    cplx = FORMS[form]
    cases = []
    m, N = 7, 3
    keep = np.sort(np.random.default_rng(73).permutation(35)[:17])                 # a seeded random half, with holes
    cases.append((m, N, keep))
    m, N = 8, 3
    cisd = truncated_space(m, 0b00000111, 2)
    full = ref.sector(m, N)
    keep = np.searchsorted(full, cisd)
    assert (full[keep] == cisd).all() and 1 < len(cisd) < len(full)
    cases.append((m, N, keep))
    for m, N, keep in cases:
        ht, ut, dets, Hd, Hx = problem(m, N, cplx)
        sub, subx = Hd[np.ix_(keep, keep)], Hx[np.ix_(keep, keep)]
        for K in (1, 9):
            c = vectors(K, len(keep), cplx, 40 + K)
            got = run_sigma(ht, ut, dets[keep], N, c)
            check_sigma(got, subx, sub, c, m, N, f"{form} m={m} N={N} subset of {len(keep)} K={K}")


def general_system(n, h, u, s, anti_symmetrized_u=False, anti_symmetrize=True):
    """n particles on spin orbitals given as they are (no spin doubling)."""
    import quantum_systems_amd as qsa
    from quantum_systems_amd import hip

    bs = qsa.setup_basis_set(n, h.shape[0], hip.asarray(s), hip.asarray(h), hip.asarray(u), 2, -1, hip, True,
                             anti_symmetrized_u, nuclear_repulsion_energy=E_NUC)
    return qsa.GeneralOrbitalSystem(n, bs, anti_symmetrize=anti_symmetrize)


def spin_doubled_system(h, u, s, anti):
    import quantum_systems_amd as qsa
    from quantum_systems_amd import hip

    spatial = qsa.construct_custom_system(2, h.shape[0], hip.asarray(s), hip.asarray(h), hip.asarray(u), dim=2, np=hip,
                                          system_type="spatial", nuclear_repulsion_energy=E_NUC)
    return spatial.construct_general_orbital_system(anti_symmetrize=anti)


def check_solver(solver, dense, n_roots, G):
    from quantum_systems_amd import kernels

    lam = np.linalg.eigvalsh(dense)
    kernels.dispatch_log = log = []
    try:
        E, c = solver.solve(n_roots, tol=TOL)
    finally:
        kernels.dispatch_log = None
    E, c = H(E), H(c)
    bound = 1e-8 * max(1.0, np.abs(lam).max())
    print(f"m={solver.m} N={solver.N} dim={solver.dim}: max |dE| = {np.abs(E - E_NUC - lam[:n_roots]).max():.2e} "
          f"(bound {bound:.1e}), {solver.iterations} iterations, vectors per step {solver.sigma_history}, "
          f"residuals {max(solver.residuals):.1e}")
    assert solver.converged and len(solver.residuals) == n_roots and max(solver.residuals) < TOL
    assert E.shape == (n_roots,) and c.shape == (n_roots, solver.dim) and (np.diff(E) >= 0).all()
    assert np.abs(E - E_NUC - lam[:n_roots]).max() <= bound
    for k in range(n_roots):
        assert abs(np.linalg.norm(c[k]) - 1.0) <= 1e-12
        assert np.linalg.norm(dense @ c[k] - (E[k] - E_NUC) * c[k]) <= bound, k
    # one Davidson iteration = one det_ci_sigma call of ceil(vectors / G) launches and no other kernel of the package
    assert len(log) == solver.iterations == len(solver.sigma_history)
    for entry, nvec in zip(log, solver.sigma_history):
        parts = [p for p in entry.split(";") if p.strip()]
        assert parts and all("qs::det_ci_sigma_kernel<" in p for p in parts), entry
        assert launches(entry) == -(-nvec // G), (entry, nvec)
    return E


def n_particles(system, n):
    """The same basis with another particle number."""
    import quantum_systems_amd as qsa

    return qsa.GeneralOrbitalSystem(n, system._basis_set, anti_symmetrize=False)


@pytest.mark.parametrize("form", list(FORMS))
def test_solver_against_the_dense_spectrum(form):
    from quantum_systems_amd import DeterminantCI, hip
    import _two_particle_ref as tp

    cplx = FORMS[form]
    G = shipped_group(cplx)
    # (7, 3): seven spin orbitals as they are, non-orthonormal s, Loewdin orbitals; the system anti-symmetrises u
    h, u, s = mf.hermitian_problem(7, seed=407, scale=0.2, complex_=cplx)
    X = ref.loewdin(s)
    assert np.abs(s - np.eye(7)).max() > 1e-2
    system = general_system(3, h, u, s)
    u_before = H(system.u).copy()
    solver = DeterminantCI(system, hip.asarray(X))
    assert (solver.m, solver.N, solver.dim) == (7, 3, 35)
    ht, ut = ref.orbital_hamiltonian(h, u, X, False)
    check_solver(solver, ref.dense_hamiltonian(ht, ut, 3), 3, G)
    assert np.array_equal(H(system.u), u_before)                                    # system.u is never modified
    # (8, 4) and (8, 3): l = 4 spatial orbitals spin-doubled, u anti-symmetrised by the system or left plain
    h, u, s = mf.hermitian_problem(4, seed=404, scale=0.2, complex_=cplx)
    X = tp.loewdin(s)
    for anti in (True, False):
        h2, u2, C2, _ = tp.spin_double(h, u, X, anti)
        base = spin_doubled_system(h, u, s, anti)
        np.testing.assert_allclose(H(base.u), u2, atol=1e-14)                       # the oracle's spin order is the package's
        assert base._basis_set._anti_symmetrized_u == anti
        ht, ut = ref.orbital_hamiltonian(h2, u2, C2, anti)
        for n in (4, 3):
            system = n_particles(base, n)
            u_before = H(system.u).copy()
            solver = DeterminantCI(system, hip.asarray(C2))
            assert (solver.m, solver.N, solver.dim) == (8, n, comb(8, n))
            check_solver(solver, ref.dense_hamiltonian(ht, ut, n), 3, G)
            assert np.array_equal(H(system.u), u_before)


@functools.lru_cache(maxsize=None)
def spin_doubled_problem(cplx):
    """The l = 4 spin-doubled problem of ``test_solver_against_the_dense_spectrum`` (u anti-symmetrised by the system):
    (h, u, s, C2, ht, ut), host arrays, computed once and never modified."""
    import _two_particle_ref as tp

    h, u, s = mf.hermitian_problem(4, seed=404, scale=0.2, complex_=cplx)
    h2, u2, C2, _ = tp.spin_double(h, u, tp.loewdin(s), True)
    return (h, u, s, C2) + tuple(ref.orbital_hamiltonian(h2, u2, C2, True))


@pytest.mark.parametrize("form", list(FORMS))
def test_solver_collapses_to_the_ritz_vectors(form, monkeypatch):
    """``max_space = 2 n_guess = 12``, the smallest the function allows, on 70 determinants: the space collapses every
    other step.  The size of every projected problem is read from the ``torch.linalg.eigh`` calls of the loop: it never
    exceeds ``max_space`` and it shrinks at least once; without a collapse it would grow past 12 at the fourth step."""
    from quantum_systems_amd import DeterminantCI, hip

    cplx = FORMS[form]
    h, u, s, C2, ht, ut = spin_doubled_problem(cplx)
    solver = DeterminantCI(n_particles(spin_doubled_system(h, u, s, True), 4), hip.asarray(C2))
    assert solver.dim == 70
    n_roots, max_space = 3, 12
    sizes, eigh = [], torch.linalg.eigh

    def spy(a, *args, **kw):
        sizes.append(a.shape[-1])
        return eigh(a, *args, **kw)

    monkeypatch.setattr(torch.linalg, "eigh", spy)
    solver.solve = functools.partial(solver.solve, max_space=max_space)             # check_solver as it is
    check_solver(solver, ref.dense_hamiltonian(ht, ut, 4), n_roots, shipped_group(cplx))
    print(f"{form}: projected sizes {sizes}")
    assert len(sizes) == solver.iterations and sizes[0] == 2 * n_roots
    assert max(sizes) <= max_space and any(b < a for a, b in zip(sizes, sizes[1:]))
    assert sum(solver.sigma_history) > max_space                                    # more vectors than the space ever held


@pytest.mark.parametrize("form", list(FORMS))
def test_solver_on_sz_sectors(form):
    """``sz_sector`` lists against ``eigvalsh`` of the oracle's H restricted to those masks (same bound as the full
    space).  The spin-doubled H conserves S_z, so the lowest root over all sectors is the full-space ground energy
    (two solves: twice the bound)."""
    from quantum_systems_amd import DeterminantCI, hip, sz_sector

    cplx = FORMS[form]
    G = shipped_group(cplx)
    h, u, s, C2, ht, ut = spin_doubled_problem(cplx)
    base = spin_doubled_system(h, u, s, True)
    for n, two_sz in ((4, 0), (3, 1)):
        dets = sz_sector(8, n, two_sz)
        full = ref.sector(8, n)
        keep = np.searchsorted(full, dets)
        assert (full[keep] == dets).all() and len(dets) == comb(4, (n + two_sz) // 2) * comb(4, (n - two_sz) // 2)
        solver = DeterminantCI(n_particles(base, n), hip.asarray(C2), dets=dets)
        assert (solver.m, solver.N, solver.dim) == (8, n, len(dets)) and np.array_equal(solver.dets, dets)
        check_solver(solver, ref.dense_hamiltonian(ht, ut, n)[np.ix_(keep, keep)], 3, G)
    lam = np.linalg.eigvalsh(ref.dense_hamiltonian(ht, ut, 4))
    bound = 1e-8 * max(1.0, np.abs(lam).max())
    lowest = []
    for two_sz in (-4, -2, 0, 2, 4):
        solver = DeterminantCI(n_particles(base, 4), hip.asarray(C2), dets=sz_sector(8, 4, two_sz))
        lowest.append(float(H(solver.solve(1, tol=TOL)[0])[0]) - E_NUC)
        assert solver.converged
    print(f"{form}: lowest root per S_z sector {lowest}, full space {lam[0]}: |dE| = {abs(min(lowest) - lam[0]):.2e} "
          f"(bound {2 * bound:.1e})")
    assert abs(min(lowest) - lam[0]) <= 2 * bound and int(np.argmin(lowest)) == 2


@pytest.mark.parametrize("form", list(FORMS))
def test_solver_that_runs_out_of_iterations(form):
    """``max_iter = 1`` on 70 determinants from 6 guesses: not converged, and the Ritz values of a subspace are upper
    bounds of the eigenvalues (Cauchy interlacing), whatever the residuals."""
    from quantum_systems_amd import DeterminantCI, hip

    cplx = FORMS[form]
    h, u, s, C2, ht, ut = spin_doubled_problem(cplx)
    solver = DeterminantCI(n_particles(spin_doubled_system(h, u, s, True), 4), hip.asarray(C2))
    lam = np.linalg.eigvalsh(ref.dense_hamiltonian(ht, ut, 4))
    bound = 1e-8 * max(1.0, np.abs(lam).max())
    E, c = solver.solve(3, tol=TOL, max_iter=1)
    E = H(E) - E_NUC
    print(f"{form}: after one iteration E - lambda = {E - lam[:3]}, residuals {solver.residuals}")
    assert solver.converged is False and solver.iterations == 1 and solver.sigma_history == [6]
    assert len(solver.residuals) == 3 and np.isfinite(solver.residuals).all() and min(solver.residuals) >= TOL
    assert E.shape == (3,) and np.isfinite(E).all() and (E >= lam[:3] - bound).all()
    assert np.abs(np.linalg.norm(H(c), axis=1) - 1.0).max() <= 1e-12


def test_the_whole_space_ends_in_one_iteration_and_the_filled_shell_is_the_identity():
    from quantum_systems_amd import DeterminantCI, hip
    import _two_particle_ref as tp

    h, u, s = mf.hermitian_problem(2, seed=402, scale=0.2, complex_=True)
    X = tp.loewdin(s)
    h2, u2, C2, _ = tp.spin_double(h, u, X, True)
    ht, ut = ref.orbital_hamiltonian(h2, u2, C2, True)
    base = spin_doubled_system(h, u, s, True)
    solver = DeterminantCI(n_particles(base, 2), hip.asarray(C2))
    check_solver(solver, ref.dense_hamiltonian(ht, ut, 2), 6, shipped_group(True))
    assert solver.iterations == 1 and solver.sigma_history == [6]
    filled = DeterminantCI(n_particles(base, 4), hip.asarray(C2))                   # N = m: one determinant
    E, c = filled.solve(1)
    assert filled.dim == 1 and filled.iterations == 1
    want = ref.dense_hamiltonian(ht, ut, 4)[0, 0].real
    assert abs(float(H(E)[0]) - E_NUC - want) <= 1e-12 * max(1.0, abs(want))
    assert np.abs(H(filled.one_body_density(0)) - np.eye(4)).max() <= 1e-15


def test_two_particles_agree_with_two_particle_ci_and_the_density_with_the_oracle():
    from quantum_systems_amd import DeterminantCI, TwoParticleCI, hip
    import _two_particle_ref as tp

    h, u, s = mf.hermitian_problem(4, seed=414, scale=0.2, complex_=True)
    X = tp.loewdin(s)
    h2, u2, C2, f = tp.spin_double(h, u, X, True)
    base = spin_doubled_system(h, u, s, True)
    pair = TwoParticleCI(base, hip.asarray(C2))
    e_pair = H(pair.solve(3, tol=TOL)[0])
    solver = DeterminantCI(n_particles(base, 2), hip.asarray(C2))
    e_det = H(solver.solve(3, tol=TOL)[0])
    assert pair.converged and solver.converged
    lam = tp.spectrum(h2, u2, C2, -1, f)
    bound = 1e-8 * max(1.0, np.abs(lam).max())
    print(f"n = 2: max |E_det - E_pair| = {np.abs(e_det - e_pair).max():.2e} (bound {2 * bound:.1e})")
    assert np.abs(e_det - e_pair).max() <= 2 * bound
    # the density of a solved state of three particles
    three = DeterminantCI(n_particles(base, 3), hip.asarray(C2))
    E, c = three.solve(2, tol=TOL)
    for k in (0, 1):
        rho, v = H(three.one_body_density(k)), H(c)[k]
        r_bound = ref.density_bound(v, 8, 3)
        err = np.abs(rho - ref.one_body_density(v, 8, 3)).max()
        print(f"state {k}: worst |rho - exact| / bound = {err / r_bound:.3f}")
        assert err <= r_bound
        assert abs(np.trace(rho) - 3) <= 8 * r_bound + 3e-12 and np.abs(rho - rho.conj().T).max() <= 2 * r_bound


def test_masks_beyond_bit_31():
    """The (6, 3) problem embedded into m = 40 at the orbitals {0, 5, 31, 32, 33, 39}; every other orbital has
    ht_ii = 1e3 and no coupling, so the blocks decouple exactly and the lowest 20 energies of the FULL C(40, 3) = 9880
    space are the small oracle's spectrum.  20 roots are asked for (40 guesses hold the whole block: one iteration);
    the test took 0.29 s on an MI355X."""
    from quantum_systems_amd import DeterminantCI

    ht6, ut6, _, H6, _ = problem(6, 3, False)
    where = np.array([0, 5, 31, 32, 33, 39])
    m = 40
    ht = np.diag(np.full(m, 1.0e3))
    ht[np.ix_(where, where)] = ht6
    ut = np.zeros((m, m, m, m))
    ut[np.ix_(where, where, where, where)] = ut6
    system = general_system(3, ht, ut, np.eye(m), anti_symmetrized_u=True)
    solver = DeterminantCI(system)
    assert (solver.m, solver.N, solver.dim) == (40, 3, 9880) and int(solver.dets.max()) > 1 << 32
    E, c = solver.solve(20, tol=TOL)
    lam = np.linalg.eigvalsh(H6)
    bound = 1e-8 * max(1.0, np.abs(lam).max())
    E = H(E) - E_NUC
    print(f"m = 40: max |dE| = {np.abs(E - lam).max():.2e} (bound {bound:.1e}), {solver.iterations} iterations, "
          f"vectors per step {solver.sigma_history}")
    assert solver.converged and np.abs(E - lam).max() <= bound
    # the states live on the 20 determinants of the embedded orbitals
    inside = np.array([all((x >> p) & 1 == 0 for p in range(m) if p not in where) for x in solver.dets.tolist()])
    assert inside.sum() == 20 and np.abs(H(c)[:, ~inside]).max() <= 1e-12


def test_refusals():
    import quantum_systems_amd as qsa
    from quantum_systems_amd import DeterminantCI, hip
    from quantum_systems_amd.sharded_module import ShardedTensor4

    h, u, s = mf.hermitian_problem(6, seed=5, scale=0.2, complex_=False)
    X = hip.asarray(ref.loewdin(s))
    spatial = qsa.construct_custom_system(2, 6, hip.asarray(s), hip.asarray(h), hip.asarray(u), dim=2, np=hip,
                                          system_type="spatial")
    with pytest.raises(TypeError, match="construct_general_orbital_system"):
        DeterminantCI(spatial)
    with pytest.raises(TypeError):
        DeterminantCI(object())
    system = general_system(3, h, u, s)
    with pytest.raises(ValueError, match="orthonormal"):
        DeterminantCI(system)
    with pytest.raises(ValueError):
        DeterminantCI(system, hip.asarray(np.eye(5)))
    with pytest.raises(ValueError, match="63"):
        DeterminantCI(system, hip.asarray(np.zeros((6, 64))))                      # m = 64 does not fit a mask
    full = qsa.full_space(6, 3)
    for bad in (full[::-1].copy(), np.concatenate([full[:3], full[2:]]), np.array([3, 7]), np.array([7, 1 << 6 | 3]),
                np.array([-7]), np.zeros(0, dtype=np.int64), full.astype(np.float64)):
        with pytest.raises(ValueError):
            DeterminantCI(system, X, dets=bad)
    solver = DeterminantCI(system, X, dets=full[:7])
    with pytest.raises(ValueError):
        solver.solve(8)                                                             # n_roots > dim
    with pytest.raises(ValueError):
        solver.solve(0)
    with pytest.raises(RuntimeError):
        solver.one_body_density(0)
    plain = torch.as_tensor(system.u).as_subclass(torch.Tensor)
    system._basis_set.u = ShardedTensor4(plain.contiguous(), 6, 0, 0, 1)
    with pytest.raises(NotImplementedError, match="sharded"):
        DeterminantCI(system, X)
