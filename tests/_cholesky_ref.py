"""NumPy reference of the pivoted Cholesky decomposition of the two-body tensor (test infrastructure only).

``G[(r,p),(q,s)] = u[p,q,r,s]`` (flat index ``first * m + second``) is Hermitian positive semidefinite for a positive
interaction; with ``G = V V^H`` and ``L_x = conj(V_x)`` reshaped ``(m, m)``, ``M_x = L_x^H``:

    u[p,q,r,s] = sum_x M_x[p,r] L_x[q,s]
"""

import numpy as np


def gram(u):
    """``G[(r,p),(q,s)] = u[p,q,r,s]`` as an ``(m^2, m^2)`` matrix."""
    m = u.shape[0]
    return np.ascontiguousarray(u.transpose(2, 0, 1, 3)).reshape(m * m, m * m)


def pivoted_cholesky(u, tau, max_rank=None):
    """Left-looking pivoted Cholesky of ``gram(u)``: the pivot is the argmax of the residual diagonal (lowest flat
    index on ties), the run stops when ``d[piv] <= tau`` or at ``max_rank`` vectors.  Returns ``(L, pivots, d)``: the
    vectors ``(rank, m, m)``, the pivots and the residual diagonal at exit."""
    m = u.shape[0]
    n = m * m
    G = gram(u)
    d = np.real(np.diagonal(G)).astype(np.float64).copy()
    cap = n if max_rank is None else min(int(max_rank), n)
    V = np.zeros((cap, n), dtype=G.dtype)
    pivots = []
    for j in range(cap):
        piv = int(np.argmax(d))                       # first occurrence = lowest flat index
        if not d[piv] > tau:
            break
        v = (G[:, piv] - V[:j].T @ np.conj(V[:j, piv])) / np.sqrt(d[piv])
        d -= np.abs(v) ** 2
        d[piv] = 0.0
        V[j] = v
        pivots.append(piv)
    rank = len(pivots)
    return np.conj(V[:rank]).reshape(rank, m, m), np.array(pivots, dtype=np.int64), d


def dagger(L):
    """``M_x = L_x^H`` for a stack."""
    return np.conj(L.transpose(0, 2, 1))


def recon(M, L):
    """``u[p,q,r,s] = sum_x M_x[p,r] L_x[q,s]``."""
    return np.einsum("xpr,xqs->pqrs", M, L)


def transform_stack(L, C, C_tilde=None):
    """``C~ L_x C`` for every matrix of a stack (``C~ = C^H`` by default): the one-body transform."""
    Ct = np.conj(C.T) if C_tilde is None else C_tilde
    return np.matmul(Ct, np.matmul(L, C))


def mean_field(M, L, D, cj, ck):
    """``W = cj sum_x M_x tr(L_x D) + ck sum_x M_x D L_x`` -- the convention of ``kernels.mean_field``:
    ``W[p,q] = cj sum_rs u[p,r,q,s] D[s,r] + ck sum_rs u[p,r,s,q] D[s,r]``."""
    t = np.einsum("xrs,sr->x", L, D)
    return cj * np.einsum("x,xpq->pq", t, M) + ck * np.einsum("xps,sr,xrq->pq", M, D, L)


def seeded_low_rank(m, r, complex_, seed):
    """``u = recon(B^H, B)`` of exact rank ``r`` from a seeded stack ``B`` ``(r, m, m)``."""
    rng = np.random.default_rng(seed)
    B = rng.standard_normal((r, m, m))
    if complex_:
        B = B + 1j * rng.standard_normal((r, m, m))
    return recon(dagger(B), B)


def random_unitary(m, seed):
    rng = np.random.default_rng(seed)
    Q, _ = np.linalg.qr(rng.standard_normal((m, m)) + 1j * rng.standard_normal((m, m)))
    return Q
