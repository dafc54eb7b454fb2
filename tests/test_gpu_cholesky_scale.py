"""``kernels.cholesky_two_body`` (qs_cholesky.hip) where ``tests/test_gpu_cholesky.py`` does not reach: past one and two
coefficient chunks of the update kernel (512 steps each), vectors and pivots against a reference, the tie rule at
exact positions, and a NaN on the residual diagonal.

Vectors and pivots against a reference.  The diagonal has exact ties, so the CPU recipe may take other pivots than the
GPU and there is no pivot sequence to compare with.  Instead the GPU's OWN pivots ``P`` are replayed on the CPU
(``ref.replay``): in extended precision (``np.longdouble``, 64-bit significand) as the reference ``Lq``, and in the
input's precision as the yardstick ``L64`` of what fp64 rounding does to this recurrence on these pivots.  With
``E_j = max_i |L64_j[i] - Lq_j[i]|`` a vector is allowed

    max_i |L_gpu_j[i] - Lq_j[i]|  <=  8 max_{k <= j} max(E_k, eps max|Lq|)

-- the running maximum, because the error of a step is inherited by every later one and the per-step ``E_j`` of ONE
summation order fluctuates; 8 is the margin of tests/test_gpu_cholesky.py for another summation order and fused
multiply-adds.  None of it comes from the kernel.  A pivot is legitimate when, on the reference's diagonal ``dq`` before
the step, ``max(dq) - dq[P_j]`` is within 8 times the running maximum of ``max(|d64 - dq|, eps max(d at start))``.

Exact arithmetic.  ``ref.exact_blocks`` gives a tensor whose decomposition is small integers throughout, so pivots
(the tie rule, over 1089 steps and 5 workgroups) and vectors (every coefficient of the second and third chunk at its
exact row) are compared with ``array_equal`` against values derived without running a decomposition.

Every test prints its measured figures (``pytest -s``)."""

import functools

import numpy as np
import pytest
import torch

import _cholesky_ref as ref

pytestmark = pytest.mark.gpu
EPS = np.finfo(np.float64).eps

CASES = {"f64_23_520": (23, 520, False), "c128_23_517": (23, 517, True), "f64_33_1030": (33, 1030, False),
         "f64_17_23": (17, 23, False), "c128_5_7": (5, 7, True)}


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def host(t):
    return torch.as_tensor(t).cpu().numpy()


@functools.lru_cache(maxsize=None)
def problem(name):
    """``u`` of a named input, made once (the large ranks through one matrix product, the small ones as in
    tests/test_gpu_cholesky.py)."""
    m, r, cplx = CASES[name]
    return ref.seeded_low_rank(m, r, cplx, seed=100 * m + r, product=r > 100)


@functools.lru_cache(maxsize=None)
def reference(name):
    """``(tau, E_ref, reference rank)`` of the NumPy recipe at ``tau = 1e-10 max|u|``, computed once."""
    u = problem(name)
    tau = 1e-10 * np.abs(u).max()
    L, _, _ = ref.pivoted_cholesky(u, tau)
    return tau, np.abs(ref.recon_product(ref.dagger(L), L) - u).max(), L.shape[0]


def allowed(name):
    tau, e_ref, _ = reference(name)
    return tau + 8 * max(e_ref, EPS * np.abs(problem(name)).max())


def run(u, tau, max_rank=None, state=None):
    from quantum_systems_amd import kernels

    L, piv, (dmax, dmin), state = kernels.cholesky_two_body(dev(u) if isinstance(u, np.ndarray) else u, tau,
                                                            max_rank=max_rank, state=state)
    return host(L), host(piv), dmax, dmin, state


@functools.lru_cache(maxsize=None)
def full_run(name):
    """The uninterrupted GPU run of a named input with room for every vector, made once:
    ``(L, pivots, dmax, dmin, diag, dispatch record)``."""
    from quantum_systems_amd import kernels

    m = CASES[name][0]
    L, piv, dmax, dmin, state = run(problem(name), reference(name)[0], max_rank=m * m)
    return L, piv, dmax, dmin, host(state.diag), kernels.last_dispatch()


@pytest.mark.parametrize("name", ["f64_23_520", "c128_23_517", "f64_33_1030"])
def test_exact_rank_past_one_and_two_chunks(name):
    m, r, cplx = CASES[name]
    u = problem(name)
    tau, e_ref, rank_ref = reference(name)
    assert rank_ref == r and r > 512 * (2 if m == 33 else 1)
    L, piv, dmax, dmin, d, ran = full_run(name)
    w = 2 if cplx else 1
    assert f"qs::cholesky_start_kernel<{w}>" in ran and "qs::cholesky_pivot_kernel x" in ran, ran
    assert f"qs::cholesky_update_kernel<{w}> x" in ran and "gemm" not in ran, ran
    recon = ref.recon_product(ref.dagger(L), L)
    err = np.abs(recon - u).max()
    print(f"{name} tau {tau:.2e}: rank {L.shape[0]}, error {err:.2e} allowed {allowed(name):.2e} (E_ref {e_ref:.2e}), "
          f"residual max {dmax:.2e} min {dmin:.2e}")
    assert L.shape == (r, m, m) and L.dtype == u.dtype
    assert piv.shape == (r,) and len(set(piv.tolist())) == r and piv.min() >= 0 and piv.max() < m * m
    assert dmax <= tau
    assert err <= allowed(name)
    assert -allowed(name) <= dmin <= 0.0
    # the residual diagonal the kernel keeps is the diagonal of the true residual
    assert np.abs(np.real(np.diagonal(ref.gram(u - recon))) - d).max() <= allowed(name)
    assert d.max() == dmax and d.min() == dmin


@pytest.mark.parametrize("name", ["f64_23_520", "c128_23_517", "f64_17_23", "c128_5_7"])
def test_vectors_and_pivots_against_the_extended_precision_replay(name):
    ref.require_extended_precision()
    m, r, cplx = CASES[name]
    u = problem(name)
    L, P, _, _, _, _ = full_run(name)
    assert L.shape[0] == r
    Lq, Dq, gapq = ref.replay(u, P, np.clongdouble if cplx else np.longdouble)
    L64, D64, _ = ref.replay(u, P, u.dtype)
    floor = EPS * np.abs(Lq).max()
    E = np.abs(L64 - Lq).reshape(r, -1).max(axis=1)
    yard = np.maximum.accumulate(np.maximum(E, floor))
    err = np.abs(L - Lq).reshape(r, -1).max(axis=1)
    worst = int(np.argmax(err / yard))
    print(f"{name}: vectors, worst |L_gpu - Lq| / running max(E, eps max|Lq|) = {float(err[worst] / yard[worst]):.3f} at "
          f"step {worst} (error {float(err[worst]):.2e}, largest E {float(E.max()):.2e}, allowed factor 8)")
    assert np.all(err <= 8 * yard), (worst, float(err[worst]), float(yard[worst]))
    # every pivot is a maximum of the reference's diagonal, to what fp64 rounding has done to that diagonal so far
    dyard = np.maximum.accumulate(np.maximum(np.abs(D64[:r] - Dq[:r]).max(axis=1), EPS * Dq[0].max()))
    worst = int(np.argmax(gapq / dyard))
    print(f"{name}: pivots, worst (max(dq) - dq[P_j]) / running max(|d64 - dq|, eps max d) = "
          f"{float(gapq[worst] / dyard[worst]):.3f} at step {worst} (gap {float(gapq[worst]):.2e}, allowed factor 8)")
    assert np.all(gapq <= 8 * dyard), (worst, float(gapq[worst]), float(dyard[worst]))


@pytest.mark.parametrize("stops", [(510, 512, 513, 529), (512, 529)])
def test_interruption_across_the_chunk_boundary(stops):
    name = "f64_23_520"
    tau = reference(name)[0]
    L1, p1, dmax1, dmin1, d1, _ = full_run(name)
    ud = dev(problem(name))
    st = None
    for cap in stops[:-1]:
        # ends on the capacity (512: the pivot-only launch j == capacity, on the edge of the first chunk)
        La, pa, dmaxa, _, st = run(ud, tau, max_rank=cap, state=st)
        assert La.shape[0] == cap and st.rank == cap and dmaxa > tau
        assert np.array_equal(La, L1[:cap]) and np.array_equal(pa, p1[:cap])
    Lb, pb, dmaxb, dminb, st = run(ud, tau, max_rank=stops[-1], state=st)
    assert Lb.shape[0] == 520 and np.array_equal(Lb, L1) and np.array_equal(pb, p1)
    assert (dmaxb, dminb) == (dmax1, dmin1) and np.array_equal(host(st.diag), d1)


@pytest.mark.parametrize("cplx", [False, True])
def test_exact_arithmetic_pins_pivots_and_vectors(cplx):
    from quantum_systems_amd import cholesky

    m, n = 33, 33 * 33
    u, piv_want, L_want = ref.exact_blocks(m, cplx, seed=33 + cplx)
    ud = dev(u)
    L, piv, dmax, dmin, st = run(ud, 0.5, max_rank=n)
    wrong = np.flatnonzero(piv != piv_want[: len(piv)])
    print(f"exact blocks {'c128' if cplx else 'f64'}: rank {L.shape[0]}, first wrong pivot at step "
          f"{wrong[0] if len(wrong) else None}, residual max {dmax} min {dmin}")
    assert L.shape == (n, m, m) and L.dtype == u.dtype and st.rank == n
    assert np.array_equal(piv, piv_want)
    bad = np.flatnonzero((L != L_want).reshape(n, -1).any(axis=1))
    assert len(bad) == 0, f"vectors differ from the derived integers first at step {bad[0]} ({len(bad)} steps)"
    assert not host(st.diag).any() and dmax == 0.0 and dmin == 0.0
    # the default growth of decompose (264 -> 528 -> 1056 -> 1089 vectors): the same bits
    chol = cholesky.decompose(ud, 0.5)
    assert chol.rank == n and chol.converged and chol.residual == (0.0, 0.0)
    assert np.array_equal(host(chol.L), L_want)


def _nan_input(m, cplx):
    r = {17: 23, 6: 9}[m]
    u = ref.seeded_low_rank(m, r, cplx, seed=100 * m + r)
    return u, 1e-10 * np.abs(u).max()


@pytest.mark.parametrize("cplx", [False, True])
@pytest.mark.parametrize("m", [17, 6])
def test_nan_on_the_diagonal_stops_the_run_at_rank_zero(m, cplx):
    from quantum_systems_amd import cholesky

    u, tau = _nan_input(m, cplx)
    n = m * m
    # (lane 0 / another lane / the last lane of the first workgroup, lane 0 of the second, the last element)
    for i in [i for i in (0, 1, 255, 256, n - 1) if i < n]:
        r, p = divmod(i, m)
        bad = u.copy()
        bad[p, r, r, p] = np.nan                                        # d[(r,p)] = Re u[p,r,r,p]
        L, piv, dmax, dmin, st = run(bad, tau, max_rank=n)
        print(f"m = {m} {'c128' if cplx else 'f64'}, NaN at d[{i}]: rank {st.rank}, residual max {dmax} min {dmin}")
        assert L.shape[0] == 0 and st.rank == 0 and np.isnan(dmax), (i, st.rank, dmax)
        with pytest.raises(ValueError, match="non-finite residual"):
            cholesky.decompose(dev(bad), tau)


@pytest.mark.parametrize("cplx", [False, True])
def test_nan_in_the_first_pivot_column_stops_the_run_at_rank_one(cplx):
    from quantum_systems_amd import cholesky

    m = 17
    u, tau = _nan_input(m, cplx)
    _, clean, _, _, _ = run(u, tau, max_rank=m * m)
    qs, ss = divmod(int(clean[0]), m)
    r, p = divmod((int(clean[0]) + 300) % (m * m), m)                   # an element of another workgroup than the pivot's
    assert (r, p) != (qs, ss) and not (ss == p and r == qs)             # the column's element of (r,p): off the diagonal
    bad = u.copy()
    bad[ss, r, qs, p] = np.nan                                          # G[(r,p),(q*,s*)] is read as conj(u[s*,r,q*,p])
    L, piv, dmax, dmin, st = run(bad, tau, max_rank=m * m)
    print(f"{'c128' if cplx else 'f64'}, NaN in the column of pivot {int(clean[0])}: rank {st.rank}, residual max {dmax}")
    assert st.rank == 1 and L.shape[0] == 1 and piv[0] == clean[0] and np.isnan(dmax)
    with pytest.raises(ValueError, match="non-finite residual"):
        cholesky.decompose(dev(bad), tau)
