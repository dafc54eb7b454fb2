"""Cholesky vectors of the two-body tensor on the GPU: ``kernels.cholesky_two_body`` (qs_cholesky.hip),
``cholesky.decompose`` / ``CholeskyTwoBody`` and ``HartreeFock(system, two_body=...)``.

Tolerance of a reconstruction.  The residual of a pivoted Cholesky decomposition is positive semidefinite, so in exact
arithmetic every element of ``u - reconstruct()`` is bounded by the largest residual diagonal, which is ``<= tau``; on
top of that comes rounding.  Allowed: ``tau + 8 max(E_ref, eps max|u|)`` with ``E_ref`` the reconstruction error of the
NumPy reference (tests/_cholesky_ref.py) on the same input and threshold; the factor 8 covers the GPU's different
summation order and its fused multiply-adds, it does not come from the code under test.

Pivots and vectors are NOT compared with the CPU: the diagonal has exact ties, ``d[(r,p)] = d[(p,r)]``, which rounding
may break differently there.  Invariants only: rank, reconstruction, residual extremes, bits between runs.
(tests/test_gpu_cholesky_scale.py compares them: with a replay of the GPU's own pivots in extended precision, and
exactly on integer input; it also holds the ranks past 512 and the non-finite input.)

Every test prints its measured figures (``pytest -s``)."""

import functools

import numpy as np
import pytest
import torch

from oracle import coulomb_oracle, qs_oracle

import _cholesky_ref as ref

pytestmark = pytest.mark.gpu
EPS = np.finfo(np.float64).eps


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def host(t):
    return torch.as_tensor(t).cpu().numpy()


def block_steps():
    from quantum_systems_amd import _lib

    return int(_lib.load().qs_cholesky_two_body_block())


@functools.lru_cache(maxsize=None)
def problem(name):
    """``(u, expected rank)`` of a named input, made once."""
    if name.startswith("dot"):
        l = int(name[3:])
        return coulomb_oracle.coulomb_elements(l), {15: 45, 21: 66}[l]
    m, r, cplx = {"f64_6_9": (6, 9, False), "f64_17_23": (17, 23, False), "c128_5_7": (5, 7, True),
                  "f64_9_long": (9, max(70, block_steps() + 6), False)}[name]
    return ref.seeded_low_rank(m, r, cplx, seed=100 * m + r), r


@functools.lru_cache(maxsize=None)
def reference(name, rel_tau):
    """``(tau, E_ref, reference rank)`` of the NumPy recipe on a named input, computed once."""
    u, _ = problem(name)
    tau = rel_tau * np.abs(u).max()
    L, _, _ = ref.pivoted_cholesky(u, tau)
    return tau, np.abs(ref.recon(ref.dagger(L), L) - u).max(), L.shape[0]


def allowed(name, rel_tau):
    u, _ = problem(name)
    tau, e_ref, _ = reference(name, rel_tau)
    return tau + 8 * max(e_ref, EPS * np.abs(u).max())


def run(u, tau, max_rank=None, state=None):
    from quantum_systems_amd import kernels

    L, piv, (dmax, dmin), state = kernels.cholesky_two_body(dev(u) if isinstance(u, np.ndarray) else u, tau,
                                                            max_rank=max_rank, state=state)
    return host(L), host(piv), dmax, dmin, state


def check_vectors(name, rel_tau, L, piv, dmax, dmin, rank):
    u, _ = problem(name)
    tau = reference(name, rel_tau)[0]
    m = u.shape[0]
    err = np.abs(ref.recon(ref.dagger(L), L) - u).max()
    print(f"{name} tau {tau:.2e}: rank {L.shape[0]}, error {err:.2e} allowed {allowed(name, rel_tau):.2e} "
          f"(E_ref {reference(name, rel_tau)[1]:.2e}), residual max {dmax:.2e} min {dmin:.2e}")
    assert L.shape == (rank, m, m) and L.dtype == u.dtype
    assert piv.shape == (rank,) and len(set(piv.tolist())) == rank and piv.min() >= 0 and piv.max() < m * m
    assert dmax <= tau
    assert err <= allowed(name, rel_tau)
    return err


@pytest.mark.parametrize("name", ["f64_6_9", "f64_17_23", "c128_5_7", "f64_9_long"])
def test_synthetic_exact_rank(name):
    from quantum_systems_amd import kernels

    u, r = problem(name)
    m = u.shape[0]
    assert reference(name, 1e-10)[2] == r
    if name == "f64_9_long":
        assert r > block_steps() and r <= m * m            # past one host read-back block
    L, piv, dmax, dmin, state = run(u, reference(name, 1e-10)[0], max_rank=m * m)
    ran = kernels.last_dispatch()
    w = 2 if np.iscomplexobj(u) else 1
    assert f"qs::cholesky_start_kernel<{w}>" in ran and "qs::cholesky_pivot_kernel x" in ran, ran
    assert f"qs::cholesky_update_kernel<{w}> x" in ran and "gemm" not in ran, ran
    check_vectors(name, 1e-10, L, piv, dmax, dmin, r)
    # (a finished pivot's diagonal is 0 exactly when it is used, and moves by later steps' rounding like every other)
    assert state.rank == r and -allowed(name, 1e-10) <= dmin <= 0.0
    # the residual diagonal the kernel keeps is the diagonal of the true residual
    R = u - ref.recon(ref.dagger(L), L)
    d = host(state.diag)
    assert np.abs(np.real(np.diagonal(ref.gram(R))) - d).max() <= allowed(name, 1e-10)
    assert d.max() == dmax and d.min() == dmin


@pytest.mark.parametrize("l", [15, 21])
def test_quantum_dot_coulomb(l):
    name = f"dot{l}"
    u, rank = problem(name)
    assert reference(name, 1e-9)[2] == rank
    L, piv, dmax, dmin, _ = run(u, reference(name, 1e-9)[0])
    check_vectors(name, 1e-9, L, piv, dmax, dmin, rank)


def test_quantum_dot_rank_survives_a_change_of_basis():
    from quantum_systems_amd import kernels

    u, rank = problem("dot15")
    C = ref.random_unitary(15, seed=7)
    ut = kernels.transform_two_body(dev(u), dev(C))
    uh = host(ut)
    tau = 1e-9 * np.abs(uh).max()
    Lr, _, _ = ref.pivoted_cholesky(uh, tau)
    e_ref = np.abs(ref.recon(ref.dagger(Lr), Lr) - uh).max()
    L, piv, dmax, dmin, _ = run(ut, tau)
    err = np.abs(ref.recon(ref.dagger(L), L) - uh).max()
    print(f"dot15 rotated: rank {L.shape[0]} (reference {Lr.shape[0]}), error {err:.2e}, E_ref {e_ref:.2e}, residual max {dmax:.2e}")
    assert L.shape[0] == rank and L.dtype == np.complex128
    assert dmax <= tau and err <= tau + 8 * max(e_ref, EPS * np.abs(uh).max())


def test_truncation_by_threshold_and_by_max_rank():
    from quantum_systems_amd import cholesky

    name = "f64_17_23"
    u, r = problem(name)
    tau, _, rank_ref = reference(name, 0.3)
    assert 0 < rank_ref < r
    L, piv, dmax, dmin, _ = run(u, tau, max_rank=17 * 17)
    assert 0 < L.shape[0] < r
    check_vectors(name, 0.3, L, piv, dmax, dmin, L.shape[0])

    chol = cholesky.decompose(dev(u), reference(name, 1e-10)[0], max_rank=10)
    assert chol.converged is False and chol.rank == 10 and tuple(chol.L.shape) == (10, 17, 17)
    assert chol.residual[0] > reference(name, 1e-10)[0]
    # the truncated vectors still bound their own error: |R_ij| <= the largest residual diagonal
    Lh = host(chol.L)
    assert np.abs(ref.recon(ref.dagger(Lh), Lh) - u).max() <= chol.residual[0] + 8 * EPS * np.abs(u).max() * r
    full = cholesky.decompose(dev(u), reference(name, 1e-10)[0])
    assert full.converged is True and full.rank == r and full.M is None and full.tol == reference(name, 1e-10)[0]


def test_repeatable_and_resumable():
    name = "f64_6_9"
    u, r = problem(name)
    tau = reference(name, 1e-10)[0]
    ud = dev(u)
    L1, p1, dmax1, dmin1, s1 = run(ud, tau, max_rank=36)
    L2, p2, dmax2, dmin2, s2 = run(ud, tau, max_rank=36)
    assert np.array_equal(L1, L2) and np.array_equal(p1, p2) and (dmax1, dmin1) == (dmax2, dmin2)
    assert np.array_equal(host(s1.diag), host(s2.diag))
    # capacity 4, then growth: the bits of the uninterrupted run
    La, pa, dmaxa, _, st = run(ud, tau, max_rank=4)
    assert La.shape[0] == 4 and st.rank == 4 and dmaxa > tau
    assert np.array_equal(La, L1[:4]) and np.array_equal(pa, p1[:4])
    Lb, pb, _, _, st = run(ud, tau, max_rank=8, state=st)
    assert Lb.shape[0] == 8 and np.array_equal(Lb, L1[:8])
    Lc, pc, dmaxc, dminc, st = run(ud, tau, max_rank=36, state=st)
    assert Lc.shape[0] == r and np.array_equal(Lc, L1) and np.array_equal(pc, p1)
    assert (dmaxc, dminc) == (dmax1, dmin1) and np.array_equal(host(st.diag), host(s1.diag))
    # a call on a finished run changes nothing
    Ld, pd, dmaxd, _, st = run(ud, tau, max_rank=36, state=st)
    assert np.array_equal(Ld, L1) and np.array_equal(pd, p1) and dmaxd == dmax1


def test_decompose_grows_its_buffer_to_the_bits_of_one_run():
    from quantum_systems_amd import cholesky

    # m = 9: the first buffer holds 8 m = 72 vectors, fewer than the rank -- one doubling (clipped to m^2 = 81)
    u = ref.seeded_low_rank(9, 78, False, seed=978)
    tau = 1e-10 * np.abs(u).max()
    chol = cholesky.decompose(dev(u), tau)
    L, piv, dmax, dmin, _ = run(u, tau, max_rank=81)
    assert chol.rank == L.shape[0] > 72 and chol.converged
    assert np.array_equal(host(chol.L), L)


@functools.lru_cache(maxsize=None)
def dot15_vectors():
    from quantum_systems_amd import cholesky

    u, rank = problem("dot15")
    chol = cholesky.decompose(dev(u), reference("dot15", 1e-9)[0])
    assert chol.rank == rank and chol.converged
    return chol


def product_bound(Lh):
    """Two evaluations of ``sum_x M_x[p,r] L_x[q,s]`` from the SAME real vectors, in any order and with or without fused
    multiply-adds, each lie within gamma_(rank + 2) sum_x |M_x[p,r]| |L_x[q,s]| of the exact sum: twice that apart."""
    g = (Lh.shape[0] + 2) * EPS
    return 2 * g / (1 - g) * ref.recon(np.abs(ref.dagger(Lh)), np.abs(Lh)).max()


def test_reconstruct_is_the_sum_over_the_vectors():
    chol = dot15_vectors()
    u, _ = problem("dot15")
    Lh = host(chol.L)
    want = ref.recon(ref.dagger(Lh), Lh)
    got = host(chol.reconstruct())
    bound = product_bound(Lh)
    print(f"reconstruct vs NumPy on the same vectors: {np.abs(got - want).max():.2e} (bound {bound:.2e})")
    assert got.shape == u.shape and np.abs(got - want).max() <= bound
    assert np.abs(got - u).max() <= allowed("dot15", 1e-9)
    out = torch.empty_like(chol.reconstruct())
    assert chol.reconstruct(out=out) is out and np.array_equal(host(out), got)


def _basis(kind, m):
    rng = np.random.default_rng(31)
    if kind == "unitary":
        return ref.random_unitary(m, seed=5), None
    if kind == "biorthogonal":
        C = np.eye(m) + 0.3 * (rng.standard_normal((m, m)) + 1j * rng.standard_normal((m, m))) / np.sqrt(m)
        return C, np.linalg.inv(C)
    return np.ascontiguousarray(ref.random_unitary(m, seed=6)[:, : m - 2]), None


@pytest.mark.parametrize("kind", ["unitary", "biorthogonal", "rectangular"])
def test_transform(kind):
    from quantum_systems_amd import kernels

    chol = dot15_vectors()
    u, _ = problem("dot15")
    C, Ct = _basis(kind, 15)
    new = chol.transform(dev(C), None if Ct is None else dev(Ct))
    mp = C.shape[1]
    assert new is not chol and new.rank == chol.rank and tuple(new.L.shape) == (chol.rank, mp, mp)
    assert (new.M is None) == (Ct is None)
    want_gpu = host(kernels.transform_two_body(dev(u), dev(C), None if Ct is None else dev(Ct)))
    got = host(new.reconstruct())
    # E: the same comparison in NumPy, on the GPU's own vectors against the CPU oracle
    Lh = host(chol.L)
    oracle = qs_oracle.transform_two_body(u, C, Ct)
    E = np.abs(ref.recon(ref.transform_stack(ref.dagger(Lh), C, Ct), ref.transform_stack(Lh, C, Ct)) - oracle).max()
    tol = 8 * max(E, EPS * np.abs(oracle).max())
    err = np.abs(got - want_gpu).max()
    print(f"transform {kind}: error {err:.2e}, allowed {tol:.2e} (E {E:.2e})")
    assert err <= tol
    if kind == "unitary":       # C~ = C^H given explicitly is recognised: M stays implicit
        assert chol.transform(dev(C), dev(np.conj(C.T))).M is None


MEAN_FIELD_FORMS = {"real": ("f64_17_23", False), "complex_d": ("f64_17_23", True), "complex": ("c128_5_7", True)}


@pytest.mark.parametrize("form", list(MEAN_FIELD_FORMS))
@pytest.mark.parametrize("cj, ck", [(1.0, -0.5), (0.3, 0.7)])
def test_mean_field(form, cj, ck):
    from quantum_systems_amd import cholesky, kernels

    name, complex_d = MEAN_FIELD_FORMS[form]
    u, r = problem(name)
    m = u.shape[0]
    chol = cholesky.decompose(dev(u), reference(name, 1e-10)[0])
    rng = np.random.default_rng(17)
    D = rng.standard_normal((m, m)) + (1j * rng.standard_normal((m, m)) if complex_d else 0)
    want = host(kernels.mean_field(dev(u), dev(D), cj=cj, ck=ck))
    got = host(chol.mean_field(dev(D), cj=cj, ck=ck))
    tol = allowed(name, 1e-10) * np.abs(D).max() * m * m
    err = np.abs(got - want).max()
    print(f"mean field {form} ({cj}, {ck}): error {err:.2e}, allowed {tol:.2e}")
    assert got.shape == (m, m) and got.dtype == want.dtype
    assert err <= tol
    if ck == 0.7:       # either term alone
        for a, b in [(cj, 0.0), (0.0, ck)]:
            w = host(kernels.mean_field(dev(u), dev(D), cj=a, ck=b))
            assert np.abs(host(chol.mean_field(dev(D), cj=a, ck=b)) - w).max() <= tol


def test_block():
    from quantum_systems_amd import kernels

    chol = dot15_vectors()
    u, _ = problem("dot15")
    Lh = host(chol.L)
    full = host(chol.reconstruct())
    bound = product_bound(Lh)
    for P, Q, R, S in [(slice(0, 3), slice(0, 3), slice(3, 15), slice(3, 15)), (range(2, 7), slice(None), range(14, 15), slice(1, 12)),
                       (slice(0, 15), slice(0, 15), slice(0, 15), slice(0, 15))]:
        got = host(chol.block(P, Q, R, S))
        want = full[tuple(x if isinstance(x, slice) else slice(x.start, x.stop) for x in (P, Q, R, S))]
        assert got.shape == want.shape and np.abs(got - want).max() <= bound

    # <ij|ab> in another basis: occupied rows and virtual columns of a seeded C
    C = ref.random_unitary(15, seed=9)
    o, v = slice(0, 3), slice(3, 15)
    bra = np.ascontiguousarray(np.conj(C[:, o].T))
    ket = np.ascontiguousarray(C[:, v])
    want = host(kernels.transform_two_body_blocks(dev(u), dev(bra), dev(bra), dev(ket), dev(ket)))
    got = host(chol.transform(dev(C)).block(o, o, v, v))
    oracle = qs_oracle.transform_two_body(u, C)[o, o, v, v]
    Lt = ref.transform_stack(Lh, C)
    E = np.abs(ref.recon(ref.dagger(Lt), Lt)[o, o, v, v] - oracle).max()
    tol = 8 * max(E, EPS * np.abs(qs_oracle.transform_two_body(u, C)).max())
    err = np.abs(got - want).max()
    print(f"block <ij|ab>: error {err:.2e}, allowed {tol:.2e} (E {E:.2e})")
    assert got.shape == (3, 3, 12, 12) and err <= tol


def _dot_system(l, n):
    import quantum_systems_amd as qsa
    from quantum_systems_amd import hip

    u, _ = problem(f"dot{l}")
    return qsa.construct_custom_system(n, l, hip.asarray(np.eye(l)), hip.asarray(coulomb_oracle.one_body_elements(l)),
                                       hip.asarray(u), dim=2, np=hip, system_type="spatial")


@pytest.mark.parametrize("n", [2, 6])
def test_hartree_fock_on_vectors(n):
    from quantum_systems_amd import CholeskyTwoBody, HartreeFock, kernels

    system = _dot_system(15, n)
    before = HartreeFock(system)
    before.scf(tol=1e-10)
    chol = system.cholesky_two_body(reference("dot15", 1e-9)[0])
    assert isinstance(chol, CholeskyTwoBody) and chol.rank == 45 and chol.converged

    hf = HartreeFock(system, two_body=chol)
    kernels.dispatch_log = []
    try:
        hf.scf(tol=1e-10)
        log = list(kernels.dispatch_log)
    finally:
        kernels.dispatch_log = None
    assert all("mean_field_kernel" not in entry for entry in log)         # u is not read
    plain = HartreeFock(system)
    plain.scf(tol=1e-10)
    diff = max(abs(a - b) for a, b in zip(hf.energies, plain.energies))
    print(f"RHF n = {n}: {hf.iterations} iterations on vectors, {plain.iterations} on u, largest energy difference {diff:.2e}")
    assert hf.converged and plain.converged and hf.iterations == plain.iterations
    assert len(hf.energies) == len(plain.energies) and diff <= 1e-9
    # the default path is what it was before the vectors existed, bit for bit
    assert plain.energies == before.energies and plain.two_body is None


def test_refusals():
    import quantum_systems_amd as qsa
    from quantum_systems_amd import HartreeFock, cholesky, kernels

    u, _ = problem("dot15")
    tau = reference("dot15", 1e-9)[0]
    with pytest.raises(ValueError, match="positive semidefinite"):
        cholesky.decompose(dev(-u), tau)
    anti = kernels.antisymmetrize(dev(u))
    with pytest.raises(ValueError, match="positive semidefinite"):
        cholesky.decompose(anti, tau)
    system = _dot_system(15, 2)
    gos = system.construct_general_orbital_system()
    with pytest.raises(ValueError, match="anti-symmetrised"):
        cholesky.decompose(gos, tau)
    chol = dot15_vectors()
    with pytest.raises(TypeError, match="SpatialOrbitalSystem"):
        HartreeFock(gos, two_body=chol)
    with pytest.raises(TypeError):
        HartreeFock(system, two_body=host(chol.L))
    with pytest.raises(ValueError):
        kernels.cholesky_two_body(dev(u), -1.0)
    assert isinstance(qsa.cholesky.decompose(system, tau), qsa.CholeskyTwoBody)
