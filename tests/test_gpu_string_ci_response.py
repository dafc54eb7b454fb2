"""The Lanczos response on the GPU: ``response.lanczos`` on ``kernels.string_ci_sigma`` from ``kernels.string_ci_one_body``,
and ``StringCI.apply_one_body`` / ``spectral_function`` / ``dipole_spectrum`` / ``polarizability`` on them.

The kernel-level runs go against the dense spectrum of tests/_string_ci_response_ref.py on its three shared cases, with the
sums and scales of tests/test_string_ci_response_ref_host.py: moments relative to ``sum_j w_j |omega_j|^p``, the response
relative to ``sum_j w_j (1 / |omega_j - omega| + 1 / (omega_j + omega))``.  The tolerance 1e-10 is the issue's: the host
recurrence alone stays below 4e-14 on these inputs, the four orders of margin cover the other summation order of the GPU
sigma, and a wrong sign, a missing projection or a wrong normalisation shows at 1e-2 or worse.  No assertion depends on the
step count at the exhaustion of a Krylov space."""

import numpy as np
import pytest
import torch

import _det_ci_ref as dref
import _string_ci_ref as ref
import _string_ci_response_ref as rref

pytestmark = pytest.mark.gpu
TOL = 1e-10


def H(x):
    return torch.as_tensor(x).cpu().numpy()


def dev(x):
    return torch.from_numpy(np.array(x)).cuda()


def kernel_level(ht, ut, m, Na, Nb):
    """(sigma on row vectors, apply A to a vector (na, nb), (na, nb)) on the string kernels."""
    from quantum_systems_amd import kernels

    k, W = ref.kh_operands(ht, ut)
    sa, sb = ref.strings(m, Na), ref.strings(m, Nb)
    na, nb = len(sa), len(sb)
    ta, tb = kernels.string_ci_table(dev(sa), m, Na), kernels.string_ci_table(dev(sb), m, Nb)
    dk, dW = dev(k), dev(W)

    def sigma(V):
        return kernels.string_ci_sigma(dk, dW, ta, tb, V.reshape(V.shape[0], na, nb)).reshape(V.shape[0], na * nb)

    return sigma, (lambda A, c: kernels.string_ci_one_body(A, ta, tb, m, c)), (na, nb)


def kernel_level_start(apply, A, c0, shape):
    c = dev(c0).reshape(shape)
    Ac = apply(dev(A), c)
    c = c.to(Ac.dtype)
    return Ac - torch.vdot(c.reshape(-1), Ac.reshape(-1)) * c


@pytest.mark.parametrize("m,Na,Nb,cplx", rref.CASES)
def test_kernel_level_driver_against_the_dense_spectrum(m, Na, Nb, cplx):
    from quantum_systems_amd import response

    ht, ut, Hd, A, Aop, c0, om, w = rref.case(m, Na, Nb, cplx)
    dim = Hd.shape[0]
    E0 = float(np.vdot(c0, Hd @ c0).real)
    sigma, apply, shape = kernel_level(ht, ut, m, Na, Nb)
    phi = kernel_level_start(apply, A, c0, shape)
    worst = 0.0
    for n in (6, 12):
        alpha, beta, norm2 = response.lanczos(sigma, phi, n)
        assert len(alpha) == n and len(beta) == n - 1
        S = response.SpectralFunction(alpha, beta, norm2, E0)
        err = rref.worst_moment_error(om, w, S.poles, S.weights, range(2 * n))
        print(f"({m},{Na},{Nb}) complex={cplx} n={n}: worst moment error / {TOL:.0e} = {err / TOL:.2e}")
        worst = max(worst, err)
    alpha, beta, norm2 = response.lanczos(sigma, phi, dim, reorthogonalize=True)
    S = response.SpectralFunction(alpha, beta, norm2, E0)
    err = rref.worst_moment_error(om, w, S.poles, S.weights, range(2 * dim))
    freq = rref.kept_frequencies(om)
    want, scale = rref.response(om, w, freq)
    rerr = float((np.abs(S.response(freq) - want) / scale).max())
    print(f"({m},{Na},{Nb}) complex={cplx} n=dim={dim} reorthogonalised: worst moment error / {TOL:.0e} = {err / TOL:.2e}, "
          f"response {rerr / TOL:.2e} on {len(freq)} frequencies")
    assert len(freq) >= 15 and abs(norm2 - w.sum()) <= 1e-12 * w.sum()
    assert max(worst, err) <= TOL and rerr <= TOL


def random_spatial_system(l, n, seed, cplx, on_device=True):
    """A seeded RandomBasisSet made physical (s positive definite near 1, u with the symmetries of <pq|rs>) with 2 n
    electrons: ``system.n`` = n doubly occupied orbitals."""
    import quantum_systems_amd as qsa

    np.random.seed(seed)
    bs = qsa.RandomBasisSet(l, 2)
    part = (lambda x: x) if cplx else (lambda x: np.ascontiguousarray(x.real))
    bs.h = part(bs.h)
    s = part(bs.s)
    bs.s = np.eye(l) + 0.1 * (s - np.diag(np.diag(s)))
    u = 0.3 * part(bs.u)
    u = u + u.conj().transpose(2, 3, 0, 1)
    bs.u = u + u.transpose(1, 0, 3, 2)
    system = qsa.SpatialOrbitalSystem(2 * n, bs)
    assert system.n == n
    host = (np.array(bs.h), np.array(bs.s), np.array(bs.u), float(bs.nuclear_repulsion_energy))
    if on_device:
        system.change_module(qsa.hip)
    return system, host


@pytest.mark.parametrize("cplx", [False, True])
def test_string_ci_level(cplx):
    import quantum_systems_amd as qsa
    from quantum_systems_amd import StringCI, hip, kernels, response

    l, n = 6, 2
    system, (h, s, u, e_nuc) = random_spatial_system(l, n, 7117, cplx)
    X = dref.loewdin(s)
    ci = StringCI(system, hip.asarray(X))
    na, nb, dim = ci.na, ci.nb, ci.dim
    assert (na, nb) == (15, 15)
    ht = X.conj().T @ h @ X
    ht = 0.5 * (ht + ht.conj().T)
    ut = np.einsum("pa,qb,pqrs,rc,sd->abcd", X.conj(), X.conj(), u, X, X, optimize=True)
    rng = np.random.default_rng(3)
    B = rng.standard_normal((3, l, l)) + (1j * rng.standard_normal((3, l, l)) if cplx else 0.0)
    A = B + B.conj().transpose(0, 2, 1)                                            # three Hermitian operators in the basis
    At = np.einsum("pa,xpq,qb->xab", X.conj(), A, X)
    sigma, apply, _ = kernel_level(ht, ut, l, n, n)

    # apply_one_body is the kernel-level call with C^H A C, for every shape of A and c
    c = rng.standard_normal((2, na, nb)) + (1j * rng.standard_normal((2, na, nb)) if cplx else 0.0)
    scale = float(np.abs(At).sum(axis=(1, 2)).max() * np.abs(c).max())
    for a_, t_ in ((A, At), (A[1], At[1])):
        for c_ in (c, c[0]):
            got, want = ci.apply_one_body(hip.asarray(a_), dev(c_)), apply(dev(t_), dev(c_))
            assert isinstance(got, torch.Tensor) and got.is_cuda and tuple(got.shape) == tuple(want.shape)
            assert float((got - want).abs().max()) <= 1e-13 * scale
    up = ci.apply_one_body(hip.asarray(A[0]), dev(c), A_down=hip.asarray(A[2]))
    want = kernels.string_ci_one_body(dev(At[0]), ci._ta, ci._tb, l, dev(c), A_down=dev(At[2]))
    assert float((up - want).abs().max()) <= 1e-13 * scale and float((up - ci.apply_one_body(hip.asarray(A[0]), dev(c))).abs().max()) > 1e-3

    # spectral_function on a given state is the kernel-level run
    # 12 spin orbitals are past the dense Jordan-Wigner oracle: the dense H is the Knowles-Handy sum on E_pq = E^a_pq x 1 + 1 x E^b_pq
    # of the ladder oracle's one-spin E (the sum that tests/test_string_ci_ref_host.py pins to the Jordan-Wigner H)
    E1, eye = ref.list_E(ref.strings(l, n), l), np.eye(na)
    Ef = (np.einsum("pqij,ab->pqiajb", E1, eye) + np.einsum("ij,pqab->pqiajb", eye, E1)).reshape(l, l, dim, dim)
    Hd = ref.kh_hamiltonian(*ref.kh_operands(ht, ut), Ef)
    Hd = 0.5 * (Hd + Hd.conj().T)
    lam, V = np.linalg.eigh(Hd)
    c0 = V[:, 0]
    om, w = rref.dense_spectrum(Hd, np.einsum("pq,pqij->ij", At[0], Ef), c0)
    nst = 12
    S = ci.spectral_function(hip.asarray(A[0]), n_steps=nst, state=dev(3.0 * c0.reshape(na, nb)))         # normalised inside
    assert isinstance(S, response.SpectralFunction) and ci._c is None
    phi = kernel_level_start(apply, At[0], c0, (na, nb))
    a2, b2, n2 = response.lanczos(sigma, phi, nst)
    S2 = response.SpectralFunction(a2, b2, n2, lam[0])
    # the same run up to the rounding of ht and ut (formed on the device there, on the host here): its first coefficients
    # and, what the later ones are for, its moments
    assert len(S.alpha) == nst and len(S.beta) == nst - 1
    for got, want in ((S.alpha[:2], a2[:2]), (S.beta[:1], b2[:1]), (S.norm2, n2), (S.E_state, lam[0])):
        assert np.abs(np.asarray(got) - np.asarray(want)).max() <= 1e-11 * max(1.0, np.abs(np.asarray(want)).max())
    same = rref.worst_moment_error(S2.poles, S2.weights, S.poles, S.weights, range(2 * nst))
    print(f"complex={cplx}: spectral_function(state=) against the kernel-level run, worst moment difference / {TOL:.0e} = {same / TOL:.2e}")
    assert same <= TOL
    err = rref.worst_moment_error(om, w, S.poles, S.weights, range(2 * nst))
    print(f"complex={cplx}: spectral_function(state=) against the dense spectrum, worst moment error / {TOL:.0e} = {err / TOL:.2e}")
    assert err <= TOL

    # a solved state
    E, _ = ci.solve(n_roots=1, tol=1e-11, max_iter=300)
    assert ci.converged
    S = ci.spectral_function(hip.asarray(A[0]), k=0, n_steps=nst)
    c = ci._c[0]
    Ac = ci.apply_one_body(hip.asarray(A[0]), c)
    phi = Ac - torch.vdot(c.reshape(-1), Ac.reshape(-1)) * c
    m0 = float(torch.vdot(phi.reshape(-1), phi.reshape(-1)).real.item())
    m1 = float(torch.vdot(phi.reshape(-1), ci.sigma(phi).reshape(-1)).real.item()) - (float(H(E)[0]) - e_nuc) * m0
    print(f"complex={cplx}: moment(0) {S.moment(0):.12e} against |phi|^2 {m0:.12e}, moment(1) {S.moment(1):.12e} against "
          f"<phi|(H - E)|phi> {m1:.12e}")
    assert abs(S.moment(0) - m0) <= 1e-12 * m0 and abs(S.moment(1) - m1) <= 1e-12 * abs(m1)
    err = rref.worst_moment_error(om, w, S.poles, S.weights, range(2 * nst))
    assert err <= 1e-8                                                            # the solver's tol, not rounding

    spectra = ci.dipole_spectrum(0, n_steps=nst)
    assert len(spectra) == H(system.dipole_moment).shape[0] == 2 and all(isinstance(x, response.SpectralFunction) for x in spectra)
    pol = ci.polarizability(0.0, n_steps=nst)
    assert isinstance(pol, qsa.DeviceArray) and tuple(pol.shape) == (2,)
    want = np.array([2.0 * np.sum(x.weights / x.poles) for x in spectra])
    assert np.abs(H(pol) - want).max() <= 1e-12 * np.abs(want).max()
    grid = np.array([0.0, 0.1, 0.2])
    damped = ci.polarizability(grid, n_steps=nst, eta=0.05)
    assert tuple(damped.shape) == (2, 3) and H(damped).dtype == np.complex128
    assert np.abs(H(damped)[1] - spectra[1].response(grid, 0.05)).max() <= 1e-12 * np.abs(H(damped)).max()

    # refusals
    with pytest.raises(ValueError):
        ci.apply_one_body(hip.asarray(A[0][:5, :5]), c)
    with pytest.raises(ValueError):
        ci.apply_one_body(hip.asarray(A[0]), c[:-1])
    with pytest.raises(ValueError):
        ci.spectral_function(hip.asarray(A))                                      # one operator at a time
    with pytest.raises(ValueError):
        ci.spectral_function(hip.asarray(A[0][:5, :5]))
    with pytest.raises(ValueError):
        ci.spectral_function(hip.asarray(A[0]), state=c.reshape(-1))
    # the budget in force is read to 32 bytes: the basis of nst - 1 steps, rounded up to that
    with kernels.tuning(string_ci_bytes=-(-(nst - 1) * dim * c.element_size() // 32) * 32):
        with pytest.raises(ValueError, match="budget"):
            ci.spectral_function(hip.asarray(A[0]), n_steps=nst, reorthogonalize=True)
        assert len(ci.spectral_function(hip.asarray(A[0]), n_steps=nst - 1, reorthogonalize=True).poles) == nst - 1
    assert len(ci.spectral_function(hip.asarray(A[0]), n_steps=nst, reorthogonalize=True).poles) == nst
    # an operator that gives phi = 0 exactly: the empty spectrum
    S = ci.spectral_function(hip.asarray(0.0 * A[0]), n_steps=nst)
    assert S.poles.shape == (0,) and S.moment(0) == 0.0 and S.response(0.3) == 0.0

    # on numpy arrays the observable comes back as numpy
    system_np, _ = random_spatial_system(l, n, 7117, cplx, on_device=False)
    ci_np = StringCI(system_np, X)
    ci_np.solve(n_roots=1, tol=1e-11, max_iter=300)
    pol_np = ci_np.polarizability(0.0, n_steps=nst)
    assert isinstance(pol_np, np.ndarray) and np.abs(pol_np - H(pol)).max() <= 1e-8 * np.abs(H(pol)).max()


def test_spin_parity_keeps_the_spectrum_of_the_singlet_ground_state():
    from quantum_systems_amd import StringCI, hip

    l, n, nst = 6, 2, 10
    system, (h, s, u, e_nuc) = random_spatial_system(l, n, 7117, False)
    X = hip.asarray(dref.loewdin(s))
    rng = np.random.default_rng(4)
    B = rng.standard_normal((l, l))
    A = hip.asarray(B + B.T)
    plain, even = StringCI(system, X), StringCI(system, X, spin_parity=+1)
    Ep, _ = plain.solve(n_roots=1, tol=1e-11, max_iter=300)
    Ee, _ = even.solve(n_roots=1, tol=1e-11, max_iter=300)
    assert abs(plain.spin_squared(0)) <= 1e-8 and abs(float(H(Ep)[0]) - float(H(Ee)[0])) <= 1e-9      # the ground state is a singlet
    Sp, Se = plain.spectral_function(A, n_steps=nst), even.spectral_function(A, n_steps=nst)
    dp = np.abs(Sp.poles - Se.poles).max() / np.abs(Sp.poles).max()
    dw = np.abs(Sp.weights - Se.weights).max() / Sp.weights.sum()
    print(f"spin_parity=+1 against none: poles differ by {dp:.2e}, weights by {dw:.2e} (tolerance 1e-8, the solver's)")
    assert dp <= 1e-8 and dw <= 1e-8
    # the result of a spin-free operator keeps the parity; an A_down does not and is refused
    c = even._c[0]
    Ac = even.apply_one_body(A, c)
    assert float((Ac - Ac.transpose(0, 1)).abs().max()) <= 1e-13 * float(Ac.abs().max())
    with pytest.raises(ValueError, match="spin"):
        even.apply_one_body(A, c, A_down=A)
    with pytest.raises(ValueError, match="spin"):
        even.spectral_function(A, A_down=A)
