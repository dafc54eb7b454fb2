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


def recon_product(M, L):
    """``recon(M, L)`` as ONE matrix product, ``[(p,r),(q,s)] = M^T L`` on the flattened stacks: the same sum in the
    order of the BLAS, for ranks where the ``einsum`` takes seconds.  (Not the same bits: the small cases keep
    ``recon``.)"""
    r, m = L.shape[0], L.shape[1]
    return np.ascontiguousarray((M.reshape(r, m * m).T @ L.reshape(r, m * m)).reshape(m, m, m, m).transpose(0, 2, 1, 3))


def seeded_low_rank(m, r, complex_, seed, product=False):
    """``u = recon(B^H, B)`` of exact rank ``r`` from a seeded stack ``B`` ``(r, m, m)`` (``product``: by
    ``recon_product``)."""
    rng = np.random.default_rng(seed)
    B = rng.standard_normal((r, m, m))
    if complex_:
        B = B + 1j * rng.standard_normal((r, m, m))
    return (recon_product if product else recon)(dagger(B), B)


def replay(u, pivots, dtype):
    """The recurrence of ``pivoted_cholesky`` on a GIVEN pivot sequence, in ``dtype`` (``np.float64`` /
    ``np.complex128``: the same operations on the same operands, hence its bits on its own pivots; ``np.longdouble`` /
    ``np.clongdouble``: the high-precision reference of a run that took these pivots).  No stop test: every pivot is
    used.  Returns ``(L, D, gap)``: the vectors ``(rank, m, m)``; ``D`` ``(rank + 1, m^2)``, row ``j`` the residual
    diagonal BEFORE step ``j`` and the last row the diagonal at exit; ``gap[j] = max(D[j]) - D[j, pivots[j]]``, zero
    where the pivot is a maximum of the diagonal it was taken from."""
    m = u.shape[0]
    n = m * m
    G = gram(u).astype(dtype)
    d = np.real(np.diagonal(G)).copy()
    rank = len(pivots)
    V = np.zeros((rank, n), dtype=G.dtype)
    D = np.empty((rank + 1, n), dtype=d.dtype)
    gap = np.empty(rank, dtype=d.dtype)
    for j, piv in enumerate(int(p) for p in pivots):
        D[j] = d
        gap[j] = d.max() - d[piv]
        v = (G[:, piv] - V[:j].T @ np.conj(V[:j, piv])) / np.sqrt(d[piv])
        d -= np.abs(v) ** 2
        d[piv] = 0.0
        V[j] = v
    D[rank] = d
    return np.conj(V).reshape(rank, m, m), D, gap


def require_extended_precision():
    """``np.longdouble`` must carry a 64-bit significand (x86-64): ``replay`` in it is the tests' reference."""
    assert np.finfo(np.longdouble).nmant >= 63, f"np.longdouble has {np.finfo(np.longdouble).nmant} mantissa bits, need >= 63"


def exact_blocks(m, complex_, seed):
    """A ``u`` whose ``gram(u)`` is block diagonal in small integers, with the pivots and vectors its decomposition
    must give -- derived here, without running one.  A seeded permutation scatters the ``n = m^2`` flat indices into
    pairs ``(i1, i2)`` with the block

        G[i1,i1] = 16     G[i1,i2] = 8 conj(z)
        G[i2,i1] = 8 z    G[i2,i2] = 4 + t^2          z in {1, -1} (complex: {1, -1, i, -i}),  t in {1, 2}

    and a left-over index with the single entry 9.  Step ``i1``: root 4, ``V = 4 e_i1 + 2 z e_i2``, which leaves
    ``d[i2] = t^2``; step ``i2``: root ``t``, ``V = t e_i2``.  Every square root, quotient, product and difference is a
    small (Gaussian) integer: exact in any order, with or without fused multiply-adds.  With "largest diagonal, lowest
    flat index on ties" the pivots are: every ``i1`` ascending (16), the single index (9), the ``i2`` with ``t = 2``
    ascending (4), those with ``t = 1`` ascending (1); the residual diagonal ends at zero.  (``z = +-1 +- i`` would not
    do: ``abs(v) ** 2`` rounds there.)

    Returns ``(u, pivots, L)`` with ``L = conj(V)`` ``(n, m, m)`` in the order of ``pivots``."""
    n = m * m
    rng = np.random.default_rng(seed)
    perm = rng.permutation(n)
    i1, i2 = perm[0 : n - 1 : 2] if n % 2 else perm[0::2], perm[1::2]
    z = rng.choice(np.array([1, -1, 1j, -1j]) if complex_ else np.array([1.0, -1.0]), size=len(i1))
    t = rng.integers(1, 3, size=len(i1))
    dt = np.complex128 if complex_ else np.float64
    G = np.zeros((n, n), dtype=dt)
    G[i1, i1] = 16
    G[i2, i1] = 8 * z
    G[i1, i2] = 8 * np.conj(z)
    G[i2, i2] = 4 + t * t
    single = perm[-1:] if n % 2 else perm[:0]
    G[single, single] = 9
    u = np.ascontiguousarray(G.reshape(m, m, m, m).transpose(1, 2, 0, 3))         # u[p,q,r,s] = G[(r,p),(q,s)]

    first = np.argsort(i1)
    second = [k[np.argsort(i2[k])] for k in (np.flatnonzero(t == 2), np.flatnonzero(t == 1))]
    pivots = np.concatenate([i1[first], single] + [i2[k] for k in second]).astype(np.int64)
    V = np.zeros((n, n), dtype=dt)
    rows = np.arange(len(i1))
    V[rows, i1[first]] = 4
    V[rows, i2[first]] = 2 * z[first]
    row = len(i1)
    for x in single:
        V[row, x] = 3
        row += 1
    for k in second:
        V[row + np.arange(len(k)), i2[k]] = t[k]
        row += len(k)
    return u, pivots, np.conj(V).reshape(n, m, m)


def random_unitary(m, seed):
    rng = np.random.default_rng(seed)
    Q, _ = np.linalg.qr(rng.standard_normal((m, m)) + 1j * rng.standard_normal((m, m)))
    return Q
