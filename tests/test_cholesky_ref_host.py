"""CPU checks of the conventions of the Cholesky vectors of the two-body tensor, on the NumPy reference
(``tests/_cholesky_ref.py``) and the CPU oracles: the ranks of the quantum-dot Coulomb tensor, the change of basis, the
mean field, the bound of a truncated run, and the two in-place reads the kernel does instead of forming G."""

import numpy as np
import pytest

from oracle import coulomb_oracle, qs_oracle

import _cholesky_ref as ref

EPS = np.finfo(np.float64).eps


@pytest.fixture(scope="module")
def dot21():
    u = coulomb_oracle.coulomb_elements(21)
    L, piv, d = ref.pivoted_cholesky(u, 1e-9 * np.abs(u).max())
    return u, L, d


@pytest.mark.parametrize("l, rank", [(6, 15), (10, 28), (15, 45), (21, 66)])
def test_quantum_dot_ranks(l, rank):
    # R closed shells: orbital products span the oscillator functions of 2R - 1 shells, (2R - 1)(2R) / 2 of them
    u = coulomb_oracle.coulomb_elements(l)
    scale = np.abs(u).max()
    L, piv, d = ref.pivoted_cholesky(u, 1e-9 * scale)
    assert L.shape == (rank, l, l) and len(set(piv.tolist())) == rank
    assert np.abs(ref.recon(ref.dagger(L), L) - u).max() <= 1e-11 * scale
    assert d.min() >= -1e-11 * scale


def test_in_place_reads_are_the_diagonal_and_the_pivot_column():
    rng = np.random.default_rng(5)
    m = 5
    B = rng.standard_normal((7, m, m)) + 1j * rng.standard_normal((7, m, m))
    u = ref.recon(ref.dagger(B), B)
    G = ref.gram(u)
    assert np.abs(G - G.conj().T).max() <= 64 * EPS * np.abs(u).max()
    # d[(r,p)] = Re u[p,r,r,p]
    d = np.real(np.einsum("prrp->rp", u)).reshape(-1)
    assert np.array_equal(d, np.real(np.diagonal(G)))
    # column (q*, s*) = the conjugated row: G[(r,p),(q*,s*)] = conj(u[s*, r, q*, p]), contiguous in p
    for qs, ss in [(0, 0), (1, 3), (4, 2)]:
        col = np.conj(u[ss, :, qs, :]).reshape(-1)
        assert np.abs(col - G[:, qs * m + ss]).max() <= 64 * EPS * np.abs(u).max()


def test_transform_identity_unitary_and_biorthogonal(dot21):
    u, L, _ = dot21
    l = u.shape[0]
    rng = np.random.default_rng(11)
    C = ref.random_unitary(l, 3)
    Lt = ref.transform_stack(L, C)
    want = qs_oracle.transform_two_body(u, C)
    assert np.abs(ref.recon(ref.dagger(Lt), Lt) - want).max() <= 1e-11 * np.abs(want).max()
    # bi-orthogonal: C~ = C^-1 is not C^H, so M' = L'^H fails and both stacks are kept
    C = np.eye(l) + 0.3 * (rng.standard_normal((l, l)) + 1j * rng.standard_normal((l, l))) / np.sqrt(l)
    Ct = np.linalg.inv(C)
    Lt = ref.transform_stack(L, C, Ct)
    Mt = ref.transform_stack(ref.dagger(L), C, Ct)
    want = qs_oracle.transform_two_body(u, C, Ct)
    assert np.abs(ref.recon(Mt, Lt) - want).max() <= 1e-10 * np.abs(want).max()
    assert np.abs(ref.recon(ref.dagger(Lt), Lt) - want).max() > 1e-3 * np.abs(want).max()


@pytest.mark.parametrize("complex_d", [False, True])
def test_mean_field_identity(dot21, complex_d):
    u, L, _ = dot21
    l = u.shape[0]
    rng = np.random.default_rng(2)
    D = rng.standard_normal((l, l)) + (1j * rng.standard_normal((l, l)) if complex_d else 0)
    for cj, ck in [(1.0, -0.5), (0.3, 0.7)]:
        want = cj * np.einsum("prqs,sr->pq", u, D) + ck * np.einsum("prsq,sr->pq", u, D)
        got = ref.mean_field(ref.dagger(L), L, D, cj, ck)
        assert np.abs(got - want).max() <= 1e-11 * np.abs(u).max() * np.abs(D).max() * l * l


def test_truncated_run_is_bounded_by_its_largest_residual_diagonal():
    u = ref.seeded_low_rank(6, 20, False, 9)
    scale = np.abs(u).max()
    full, _, _ = ref.pivoted_cholesky(u, 1e-10 * scale)
    assert full.shape[0] == 20
    tau = 0.3 * scale
    L, _, d = ref.pivoted_cholesky(u, tau)
    assert 0 < L.shape[0] < 20
    R = u - ref.recon(ref.dagger(L), L)
    # the residual is positive semidefinite: |R_ij| <= sqrt(R_ii R_jj) <= max d <= tau
    assert d.max() <= tau
    assert np.abs(R).max() <= d.max() + 64 * EPS * scale
    assert np.abs(np.real(np.diagonal(ref.gram(R))) - d).max() <= 64 * EPS * scale


@pytest.mark.parametrize("m, r, cplx", [(6, 9, False), (5, 7, True), (9, 78, False)])
def test_replay_on_the_pivots_of_the_reference_is_the_reference(m, r, cplx):
    u = ref.seeded_low_rank(m, r, cplx, seed=100 * m + r)
    L, piv, d = ref.pivoted_cholesky(u, 1e-10 * np.abs(u).max())
    assert L.shape[0] == r
    Lr, D, gap = ref.replay(u, piv, u.dtype)
    assert Lr.dtype == L.dtype and np.array_equal(Lr, L)
    assert D.shape == (r + 1, m * m) and np.array_equal(D[r], d) and np.array_equal(D[0], np.real(np.diagonal(ref.gram(u))))
    assert gap.shape == (r,) and not gap.any()
    # a pivot that is NOT the maximum shows in the gap: the first two pivots swapped
    swapped = piv.copy()
    swapped[[0, 1]] = swapped[[1, 0]]
    assert ref.replay(u, swapped, u.dtype)[2][0] > 0
    # extended precision: 64 bits of significand, and the same decomposition to the rounding of the fp64 run
    ref.require_extended_precision()
    Lq, Dq, gapq = ref.replay(u, piv, np.clongdouble if cplx else np.longdouble)
    assert Lq.dtype == (np.clongdouble if cplx else np.longdouble) and Dq.dtype == np.longdouble
    assert 0 < np.abs(Lq - L).max() <= 1e-9 * np.abs(L).max()


@pytest.mark.parametrize("cplx", [False, True])
def test_exact_blocks_decompose_to_the_derived_integers(cplx):
    m = 33
    n = m * m
    u, piv, L = ref.exact_blocks(m, cplx, seed=7)
    assert u.dtype == (np.complex128 if cplx else np.float64) and L.dtype == u.dtype
    assert sorted(piv.tolist()) == list(range(n))
    G = ref.gram(u)
    assert np.array_equal(G, G.conj().T) and np.array_equal(G, np.rint(G.real) + 1j * np.rint(G.imag) if cplx else np.rint(G))
    V = np.conj(L).reshape(n, n)
    assert np.array_equal(V.T @ np.conj(V), G)                  # integers: the product is exact
    Lr, pr, d = ref.pivoted_cholesky(u, 0.5)
    assert Lr.shape[0] == n and np.array_equal(pr, piv) and np.array_equal(Lr, L) and not d.any()
    if cplx:
        assert np.abs(L.imag).max() == 2                        # z = +-i is drawn
    # the tie rule is asked across the order of a pair: pairs with i2 < i1 exist, and so do pairs with i1 < i2
    half = n // 2
    below = np.argmax(np.abs(V[:half]) == 2, axis=1) < piv[:half]
    assert below.any() and not below.all()
    # the second coefficient chunk of the kernel (512 coefficients at a time): a step j >= 513 whose ONLY non-zero
    # coefficient conj(L_x[piv_j]) sits at an x >= 512, in each of the four summation chains x & 3
    chains = set()
    for j in range(513, n):
        (x,) = np.nonzero(V[:j, piv[j]])
        if len(x) == 1 and x[0] >= 512:
            chains.add(int(x[0]) & 3)
    print(f"exact_blocks(33, {cplx}): chains {sorted(chains)}")
    assert chains == {0, 1, 2, 3}
