"""The two density oracles of tests/_det_ci_density_ref.py against each other and against identities that hold for
any bra and ket, on the host: the string oracle (what the GPU tests use past m = 8) equals the Jordan-Wigner one on
every shape both reach, for a random complex bra != ket, on full sectors and on random halves of them.

Both run in ``numpy.longdouble`` on the same +-1 signs, so they differ only by the order of at most dim products per
element: gamma_(dim+2) of the long double format times |bra| |ket| (times 2 sqrt 2, complex) bounds the difference.
The identities are sums of m or m^2 such elements and get that many bounds."""

from math import comb

import numpy as np
import pytest

import _det_ci_density_ref as dref
import _det_ci_ref as ref

SHAPES = [(4, 2), (6, 3), (7, 3), (8, 4), (7, 1), (7, 6), (5, 5)]
EPS_LD = float(np.finfo(np.longdouble).eps)


def pair(dim, seed, cplx=True):
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(2):
        v = rng.standard_normal(dim) + (1j * rng.standard_normal(dim) if cplx else 0.0)
        out.append(v / np.linalg.norm(v))
    return out


def wide_bound(dim, terms=1):
    """gamma_(dim+2) in long double for unit vectors, complex products, ``terms`` elements summed."""
    return terms * (dim + 2) * EPS_LD * 2.0 * np.sqrt(2.0) * 1.01 + terms * EPS_LD


def lists(m, N):
    full = np.arange(comb(m, N))
    yield "full", full
    if len(full) > 1:
        yield "half", np.sort(np.random.default_rng(10 * m + N).permutation(len(full))[:(len(full) + 1) // 2])


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"m{s[0]}_N{s[1]}")
def test_string_oracle_equals_the_jordan_wigner_oracle(shape):
    m, N = shape
    sec = ref.sector(m, N)
    for name, keep in lists(m, N):
        bra, ket = pair(len(keep), 100 * m + N)
        assert abs(np.vdot(bra, ket)) > 1e-3 or len(keep) == 1                     # not orthogonal
        rho_j, G_j = dref.jw_densities(bra, ket, m, N, keep)
        rho_s, G_s = dref.string_densities(bra, ket, sec[keep], m)
        tol = wide_bound(len(keep))
        d1, d2 = float(np.abs(rho_j - rho_s).max()), float(np.abs(G_j - G_s).max())
        print(f"m={m} N={N} {name}: |rho_jw - rho_string| = {d1:.2e}, |G_jw - G_string| = {d2:.2e} (bound {tol:.2e})")
        assert rho_j.shape == (m, m) and G_j.shape == (m,) * 4 and d1 <= tol and d2 <= tol
        assert np.abs(G_j).max() > 0.01 or N == 1
        if N == 1:
            assert not G_j.any() and not G_s.any()


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"m{s[0]}_N{s[1]}")
def test_traces_of_the_oracle(shape):
    """sum_pq G[p,q,p,q] = N (N - 1) <bra|ket>,  sum_q G[p,q,r,q] = (N - 1) rho[r,p],  sum_p rho[p,p] = N <bra|ket>."""
    m, N = shape
    sec = ref.sector(m, N)
    for name, keep in lists(m, N):
        bra, ket = pair(len(keep), 200 * m + N)
        overlap = np.vdot(ref._wide(bra), ref._wide(ket))
        for rho, G in (dref.jw_densities(bra, ket, m, N, keep), dref.string_densities(bra, ket, sec[keep], m)):
            assert abs(np.einsum("pqpq->", G) - N * (N - 1) * overlap) <= wide_bound(len(keep), m * m)
            assert abs(np.trace(rho) - N * overlap) <= wide_bound(len(keep), m)
            assert np.abs(np.einsum("pqrq->pr", G) - (N - 1) * rho.T).max() <= wide_bound(len(keep), m + 1) * max(1, N)
            # anti-symmetry of the operator string
            assert np.abs(G + G.transpose(1, 0, 2, 3)).max() <= 2 * wide_bound(len(keep))
            assert np.abs(G + G.transpose(0, 1, 3, 2)).max() <= 2 * wide_bound(len(keep))


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"m{s[0]}_N{s[1]}")
@pytest.mark.parametrize("cplx", [False, True], ids=["real_h", "complex_h"])
def test_energy_functional_is_the_matrix_element_of_h(cplx, shape):
    """sum ht rho + 1/4 sum ut G = bra^H H ket with ``dense_hamiltonian`` on the full sector and ``string_hamiltonian`` on
    a subset.  Both sides are sums over the same (m^2 + m^4) dim products in another order: the bound is
    gamma_(dim + m^4 + 4) (sum |ht||rho| + 1/4 sum |ut||G|) in long double, doubled for the two sides."""
    m, N = shape
    ht, ut = ref.random_hamiltonian(m, 300 * m + N, cplx)
    sec = ref.sector(m, N)
    Hx = ref.dense_hamiltonian(ht, ut, N, extended=True)
    for name, keep in lists(m, N):
        bra, ket = pair(len(keep), 400 * m + N)
        Hs = Hx[np.ix_(keep, keep)] if name == "full" else ref.string_hamiltonian(ht, ut, sec[keep])
        want = ref._wide(bra).conj() @ (Hs.astype(np.clongdouble) @ ref._wide(ket))
        for rho, G in (dref.jw_densities(bra, ket, m, N, keep), dref.string_densities(bra, ket, sec[keep], m)):
            got = dref.energy(ht, ut, rho, G)
            scale = float(np.sum(np.abs(ht) * np.abs(rho.T)) + 0.25 * np.sum(np.abs(ut) * np.abs(G)))
            tol = 2 * (len(keep) + m ** 4 + 4) * EPS_LD * 2.0 * np.sqrt(2.0) * 1.01 * max(scale, 1.0)
            print(f"m={m} N={N} {name}: |E[rho, G] - bra H ket| = {abs(got - want):.2e} (bound {tol:.2e})")
            assert abs(got - want) <= tol


def test_pair_bound_is_the_density_bound_for_one_vector():
    v = pair(35, 5)[0] * 1.7
    assert dref.pair_bound(v, v) == pytest.approx(ref.density_bound(v, 7, 3), rel=1e-14)
    assert dref.pair_bound(v.real, v.real) == pytest.approx(ref.density_bound(v.real, 7, 3), rel=1e-14)
