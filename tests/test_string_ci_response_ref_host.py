"""The host reference of the one-body kernel and of the Lanczos response (tests/_string_ci_response_ref.py) against dense
linear algebra, and ``response.lanczos`` / ``response.SpectralFunction`` on host tensors against that reference.  No GPU.

Cases: (4,2,2) real, (4,2,2) complex, (4,2,1) real; ``A = B + B^T`` with ``B`` from ``default_rng(5)``; the state is the dense
ground vector.  Errors are relative to ``sum_j w_j |omega_j|^p`` (moments) and to
``sum_j w_j (1 / |omega_j - omega| + 1 / (omega_j + omega))`` (response); the tolerance 1e-12 is the issue's, the measured
errors are a few 1e-14.  At (4,2,2) the Krylov space of the singlet ground state has 19 dimensions of 36: n = dim runs on
through rounding, which is harmless (and why no assertion here depends on a step count at breakdown)."""

import numpy as np
import pytest

import _string_ci_ref as ref
import _string_ci_response_ref as rref

TOL = 1e-12


@pytest.mark.parametrize("m,Na,Nb,cplx", rref.CASES)
def test_one_body_helper_is_the_dense_operator(m, Na, Nb, cplx):
    ht, ut, H, A, Aop, c0, om, w = rref.case(m, Na, Nb, cplx)
    sa, sb = ref.strings(m, Na), ref.strings(m, Nb)
    Ea, Eb = ref.list_E(sa, m), ref.list_E(sb, m)
    rng = np.random.default_rng(m + Na)
    c = rng.standard_normal((2, len(sa), len(sb))) + (1j * rng.standard_normal((2, len(sa), len(sb))) if cplx else 0.0)
    got = rref.one_body(A[None], A[None], Ea, Eb, c)
    assert got.shape == (1, 2, len(sa), len(sb))
    want = c.reshape(2, -1) @ Aop.T
    assert np.abs(got[0].reshape(2, -1) - want).max() <= 1e-13 * np.abs(want).max()
    # the two spins apart: alpha alone and beta alone add up to the spin-free operator, and differ from each other
    up = rref.one_body(A[None], 0 * A[None], Ea, Eb, c)
    down = rref.one_body(0 * A[None], A[None], Ea, Eb, c)
    assert np.abs(up + down - got).max() <= 1e-15 * np.abs(want).max() and np.abs(up - down).max() > 1e-3
    bound = rref.one_body_bound(A[None], A[None], Ea, Eb, c)
    assert bound.shape == got.shape and (bound >= 0).all() and bound.max() < 1e-12


@pytest.mark.parametrize("m,Na,Nb,cplx", rref.CASES)
def test_dense_lanczos_reproduces_the_dense_moments_and_response(m, Na, Nb, cplx):
    ht, ut, H, A, Aop, c0, om, w = rref.case(m, Na, Nb, cplx)
    dim = H.shape[0]
    E0 = float(np.vdot(c0, H @ c0).real)
    phi = Aop @ c0
    phi = phi - np.vdot(c0, phi) * c0
    assert abs(w.sum() - np.vdot(phi, phi).real) <= 1e-13 * w.sum() and (om > 0).all()
    worst = 0.0
    for n, reorth in ((6, False), (6, True), (12, False), (12, True)):
        got = rref.poles_weights(*rref.lanczos_dense(H, phi, n, reorth), E0)
        err = rref.worst_moment_error(om, w, *got, range(2 * n))
        print(f"({m},{Na},{Nb}) complex={cplx} n={n} reorth={reorth}: worst moment error {err:.2e}")
        worst = max(worst, err)
    got = rref.poles_weights(*rref.lanczos_dense(H, phi, dim, True), E0)
    err = rref.worst_moment_error(om, w, *got, range(2 * dim))
    freq = rref.kept_frequencies(om)
    rerr = rref.worst_response_error(om, w, *got, freq)
    print(f"({m},{Na},{Nb}) complex={cplx} n=dim={dim}: worst moment error {err:.2e}, response {rerr:.2e} on {len(freq)} frequencies")
    assert len(freq) >= 15
    assert max(worst, err) <= TOL and rerr <= TOL


@pytest.fixture(scope="module")
def response():
    import __graft_entry__ as entry

    entry.build()
    from quantum_systems_amd import response

    return response


@pytest.mark.parametrize("m,Na,Nb,cplx", rref.CASES)
def test_the_driver_on_host_tensors_is_the_dense_recurrence(response, m, Na, Nb, cplx):
    """``response.lanczos`` is generic: with a dense product on host tensors as ``sigma`` it is ``lanczos_dense``, and
    ``SpectralFunction`` is ``poles_weights`` with the sums written out."""
    import torch

    ht, ut, H, A, Aop, c0, om, w = rref.case(m, Na, Nb, cplx)
    dim = H.shape[0]
    E0 = float(np.vdot(c0, H @ c0).real)
    phi = Aop @ c0
    phi = phi - np.vdot(c0, phi) * c0
    Ht = torch.from_numpy(np.array(H))
    calls = []

    def sigma(V):
        calls.append(tuple(V.shape))
        return V @ Ht.transpose(0, 1)

    for n, reorth in ((6, False), (12, False), (dim, True)):
        del calls[:]
        alpha, beta, norm2 = response.lanczos(sigma, torch.from_numpy(np.array(phi)), n, reorthogonalize=reorth)
        assert calls == [(1, dim)] * n and alpha.dtype == beta.dtype == np.float64 and len(alpha) == n and len(beta) == n - 1
        assert abs(norm2 - np.vdot(phi, phi).real) <= 1e-14 * norm2
        S = response.SpectralFunction(alpha, beta, norm2, E0)
        assert (np.diff(S.poles) >= 0).all() and S.poles.shape == S.weights.shape == (n,)
        err = rref.worst_moment_error(om, w, S.poles, S.weights, range(2 * n))
        print(f"({m},{Na},{Nb}) complex={cplx} n={n}: worst moment error of the driver {err:.2e}")
        assert err <= TOL
        for p in (0, 1, 3):
            assert abs(S.moment(p) - np.sum(S.weights * S.poles ** p)) <= 1e-15 * np.sum(S.weights * np.abs(S.poles) ** p)
    freq = rref.kept_frequencies(om)
    want, scale = rref.response(om, w, freq)
    got = S.response(freq)
    assert got.dtype == np.float64 and (np.abs(got - want) / scale).max() <= TOL
    assert abs(S.response(0.0) - 2.0 * np.sum(S.weights / S.poles)) <= 1e-13 * abs(S.response(0.0))
    eta = 0.05
    damped = S.response(freq, eta)
    z = freq[:, None] + 1j * eta
    assert np.iscomplexobj(damped) and np.abs(damped - np.sum(S.weights * (1 / (S.poles - z) + 1 / (S.poles + z)), axis=1)).max() <= 1e-12
    # Im alpha(omega + i eta) = pi (S_eta(omega) - S_eta(-omega)) with the Lorentzians of `broadened`
    assert np.abs(damped.imag - np.pi * (S.broadened(freq, eta) - S.broadened(-freq, eta))).max() <= 1e-12 * np.abs(damped).max()
    assert np.allclose(S.oscillator_strengths(), 2.0 * S.poles * S.weights, rtol=0, atol=0)


def test_the_driver_stops_only_where_it_is_told_to(response):
    import torch

    from quantum_systems_amd import kernels

    # a 3-dimensional invariant subspace of a diagonal operator: beta_3 is rounding next to the others
    Hd = torch.diag(torch.tensor([1.0, 2.0, 4.0, 8.0, 16.0], dtype=torch.float64))
    start = torch.tensor([1.0, 1.0, 1.0, 0.0, 0.0], dtype=torch.float64)
    assert len(response.lanczos(lambda V: V @ Hd, start, 2)[0]) == 2
    alpha, beta, norm2 = response.lanczos(lambda V: V @ Hd, start, 5, beta_tol=1e-10)
    assert len(alpha) == 3 and len(beta) == 2 and norm2 == 3.0
    # the kept basis of a reorthogonalised run is under the byte budget of the string kernels
    assert kernels.string_ci_budget() == kernels.STRING_CI_BYTES
    with kernels.tuning(string_ci_bytes=64):
        assert kernels.string_ci_budget() == 64
        with pytest.raises(ValueError, match="budget"):
            response.lanczos(lambda V: V @ Hd, start, 5, reorthogonalize=True)
        assert len(response.lanczos(lambda V: V @ Hd, start, 1, reorthogonalize=True)[0]) == 1
        assert len(response.lanczos(lambda V: V @ Hd, start, 5)[0]) >= 3
    S = response.SpectralFunction(alpha, beta, norm2, 0.0)
    assert np.abs(S.poles - [1.0, 2.0, 4.0]).max() <= 1e-14 and np.abs(S.weights - 1.0).max() <= 1e-14
    # a tolerance that the first beta does not pass ends the run after one step
    alpha, beta, _ = response.lanczos(lambda V: V @ Hd, start, 5, beta_tol=10.0)
    assert len(alpha) == 1 and len(beta) == 0
    # a zero start is the empty spectrum
    alpha, beta, norm2 = response.lanczos(lambda V: V @ Hd, 0 * start, 5)
    S = response.SpectralFunction(alpha, beta, norm2, 0.0)
    assert len(alpha) == len(beta) == 0 and norm2 == 0.0 and S.poles.shape == (0,) and S.moment(0) == 0.0 and S.response(1.0) == 0.0
    with pytest.raises(ValueError):
        response.SpectralFunction([1.0, 2.0], [], 1.0, 0.0)
