"""CPU restatement of the mean-field contraction, for the tests of ``qs_mean_field`` / ``kernels.mean_field``:

    W[p,q] = cj * sum_{r,s} u[p,r,q,s] D[s,r]  +  ck * sum_{r,s} u[p,r,s,q] D[s,r]

by ``numpy.einsum`` in fp64 and in ``numpy.longdouble`` (the exact side of the parity bound), the bound itself, the
reference-determinant densities, and a plain NumPy SCF (no DIIS) for the driver's energies.  Nothing here imports the
package under test."""

import numpy as np

EPS = 2.0 ** -53


def jk(u_slab, D, r_lo=0, extended=False):
    """The two sums on their own, (J, K), for a (P, R, L, L) slab whose second index starts at ``r_lo``."""
    R = u_slab.shape[1]
    Dr = D[:, r_lo:r_lo + R]
    if extended:
        cplx = np.iscomplexobj(u_slab) or np.iscomplexobj(D)
        big = np.clongdouble if cplx else np.longdouble
        Dr = Dr.astype(big)
        u_slab = u_slab.astype(np.clongdouble if np.iscomplexobj(u_slab) else np.longdouble)
    return np.einsum("prqs,sr->pq", u_slab, Dr), np.einsum("prsq,sr->pq", u_slab, Dr)


def mean_field(u_slab, D, cj=1.0, ck=0.0, r_lo=0, extended=False):
    J, K = jk(u_slab, D, r_lo, extended)
    return cj * J + ck * K


def gamma(k):
    return k * EPS / (1.0 - k * EPS)


def error_bound(u_slab, D, cj, ck, r_lo=0, extra_terms=0):
    """Any summation order of the n = 2 R L products of an element of W satisfies |W - W_exact| <= gamma_(n+2) * A,
    A = the formula on |u|, |D|, |cj|, |ck|; complex products cost a further factor 2 sqrt 2."""
    P, R, L = u_slab.shape[0], u_slab.shape[1], u_slab.shape[3]
    A = mean_field(np.abs(u_slab), np.abs(D), abs(cj), abs(ck), r_lo)
    cplx = np.iscomplexobj(u_slab) or np.iscomplexobj(D)
    return gamma(2 * R * L + 2 + extra_terms) * A * (2.0 * np.sqrt(2.0) if cplx else 1.0)


def reference_density(l, n_occ, occupation):
    """The reference determinant in the current basis: ``occupation`` on the first ``n_occ`` diagonal entries."""
    rho = np.zeros((l, l))
    rho[np.arange(n_occ), np.arange(n_occ)] = occupation
    return rho


def fock_from_density(h, u, rho, cj, ck):
    return h + mean_field(u, rho, cj, ck)


def energy_from_density(h, u, rho, cj, ck, e_nuc=0.0):
    W = mean_field(u, rho, cj, ck)
    return np.einsum("pq,qp->", h, rho) + 0.5 * np.einsum("pq,qp->", W, rho) + e_nuc


def hermitian_problem(l, seed, scale=0.02, complex_=True):
    """Seeded (h, u, s) with the symmetries of a physical Hamiltonian -- h and s Hermitian, s positive definite and
    not the identity, u[pqrs] = u[qpsr] = conj(u[rspq]) -- and an interaction weak enough for plain SCF iterations."""
    rng = np.random.default_rng(seed)

    def rand(*shape):
        x = rng.standard_normal(shape)
        return x + 1j * rng.standard_normal(shape) if complex_ else x

    a = rand(l, l)
    h = np.diag(np.arange(l, dtype=float)) + 0.1 * (a + a.conj().T)
    b = rand(l, l)
    s = np.eye(l) + 0.05 * (b + b.conj().T)
    v = scale * rand(l, l, l, l)
    u = v + v.transpose(1, 0, 3, 2)
    u = u + u.transpose(2, 3, 0, 1).conj()
    return h, np.ascontiguousarray(u), s


def plain_scf(h, u, s, n_occ, occupation, cj, ck, e_nuc=0.0, tol=1e-10, max_iter=500):
    """Independent SCF: core guess, Loewdin orthogonalisation, fixed-point iteration (no DIIS) to
    max |X^H (F rho s - s rho F) X| < tol.  Returns (energy, energy of the core guess, iterations)."""
    sv, sU = np.linalg.eigh(s)
    X = (sU / np.sqrt(sv)) @ sU.conj().T

    def density(F):
        _, Cp = np.linalg.eigh(X.conj().T @ F @ X)
        Co = (X @ Cp)[:, :n_occ]
        return occupation * Co @ Co.conj().T

    rho = density(h)
    first = None
    for it in range(1, max_iter + 1):
        W = mean_field(u, rho, cj, ck)
        F = h + W
        energy = (np.einsum("pq,qp->", h + 0.5 * W, rho) + e_nuc).real
        first = energy if first is None else first
        err = X.conj().T @ (F @ rho @ s - s @ rho @ F) @ X
        if np.abs(err).max() < tol:
            return energy, first, it
        rho = density(F)
    raise RuntimeError("plain SCF did not converge")
