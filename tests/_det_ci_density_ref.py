"""NumPy oracles of the one- and two-body (transition) densities of vectors on Slater determinants, for the tests of
``qs_det_ci_transition_density1`` / ``qs_det_ci_density2`` and of the observables of ``determinant_ci.DeterminantCI``:

    rho[q, p]       = <bra| a+_p a_q |ket>
    G[p, q, r, s]   = <bra| a+_p a+_q a_s a_r |ket>
    <bra| H |ket>   = sum_pq ht[p,q] rho[q,p] + 1/4 sum_pqrs ut[p,q,r,s] G[p,q,r,s]

Two independent routes, both on top of tests/_det_ci_ref.py and both in ``numpy.longdouble``:

  * ``jw_densities`` (m <= 8): the Jordan-Wigner matrices of ``annihilators``; ``a_s a_r`` is cut to the
    (N -> N - 2)-particle block, ``G[p,q,r,s] = (a_q a_p bra)^H (a_s a_r ket)``;
  * ``string_densities`` (any ascending list of masks, orbitals up to 62): ``a_r``, ``a_s``, ``a+_q``, ``a+_p`` applied
    factor by factor to the list with ``_ladder`` and matched against it with ``_land``.

Neither holds a Slater-Condon rule or a count of the particles between two orbitals: the sign of every element comes
from the operators themselves.  A vector on a sub-list is the vector on the full list with zeros elsewhere, which is
the projection the kernels promise.  Nothing here imports the package under test."""

import numpy as np

import _det_ci_ref as ref


def pair_bound(bra, ket):
    """An element of rho or G is a sum of at most dim products conj(bra_I) ket_J with I -> J injective, so by
    Cauchy-Schwarz |error| <= gamma_(dim+2) |bra|_2 |ket|_2; complex products cost a further 2 sqrt 2
    (``_det_ci_ref.density_bound`` is the bra = ket case)."""
    dim = len(ket)
    cplx = np.iscomplexobj(bra) or np.iscomplexobj(ket)
    norms = float(np.linalg.norm(np.asarray(bra, dtype=np.complex128)) * np.linalg.norm(np.asarray(ket, dtype=np.complex128)))
    return ref.gamma(dim + 2) * norms * (2.0 * np.sqrt(2.0) if cplx else 1.0)


def _padded(v, keep, dim):
    v = ref._wide(np.asarray(v))
    if keep is None:
        assert len(v) == dim
        return v
    out = np.zeros(dim, dtype=v.dtype)
    out[np.asarray(keep)] = v
    return out


def jw_densities(bra, ket, m, N, keep=None):
    """(rho, G) of ``bra`` and ``ket`` on ``sector(m, N)`` -- or, with ``keep``, on its positions ``keep`` -- from the
    Jordan-Wigner matrices; rho (m, m), G (m, m, m, m), longdouble."""
    ops, sec = ref.annihilators(m), ref.sector(m, N)
    b, k = _padded(bra, keep, len(sec)), _padded(ket, keep, len(sec))
    dt = np.result_type(b.dtype, k.dtype)
    b, k = b.astype(dt), k.astype(dt)
    cut = [op[:, sec].astype(dt) for op in ops]                        # a_p from N to N - 1 particles, all rows kept
    low_b = np.array([c @ b for c in cut])                             # a_p |bra>
    low_k = np.array([c @ k for c in cut])
    rho = np.einsum("px,qx->qp", low_b.conj(), low_k)                  # rho[q,p] = (a_p bra)^H (a_q ket)
    G = np.zeros((m, m, m, m), dtype=dt)
    if N >= 2:
        low = ref.sector(m, N - 2)
        A = np.array([[(ops[s] @ ops[r])[np.ix_(low, sec)] for s in range(m)] for r in range(m)]).astype(dt)   # A[r,s] = a_s a_r
        G = np.einsum("pqx,rsx->pqrs", (A @ b).conj(), A @ k)         # a+_p a+_q = (a_q a_p)^H = A[p,q]^H
    return rho, G


def string_densities(bra, ket, dets, m):
    """(rho, G) of ``bra`` and ``ket`` on the ascending masks ``dets`` from operator strings applied to the list, in
    longdouble; a string that leaves the list contributes nothing."""
    dets, start = ref._start(dets)
    b, k = ref._wide(np.asarray(bra)), ref._wide(np.asarray(ket))
    dt = np.result_type(b.dtype, k.dtype)
    bc, k = b.astype(dt).conj(), k.astype(dt)

    def element(state, live=None):
        col, row, sign = ref._land(dets, state)                        # string |dets[col]> = sign |dets[row]>
        return np.sum(bc[row] * sign * k[col if live is None else live[col]])

    rho = np.zeros((m, m), dtype=dt)
    G = np.zeros((m, m, m, m), dtype=dt)
    for r in range(m):
        first = ref._ladder(start, r, False)                           # a_r
        for p in range(m):
            rho[r, p] = element(ref._ladder(first, p, True))           # a+_p a_r
        for s in range(m):
            lowered = ref._ladder(first, s, False)                     # a_s a_r
            live = np.nonzero(lowered[2])[0]                           # only the determinants that survived go on
            if not len(live):
                continue
            lowered = tuple(x[live] for x in lowered)
            for q in range(m):
                raised = ref._ladder(lowered, q, True)                 # a+_q a_s a_r
                for p in range(m):
                    G[p, q, r, s] = element(ref._ladder(raised, p, True), live)
    return rho, G


def energy(ht, ut, rho, G):
    """sum ht[p,q] rho[q,p] + 1/4 sum ut[p,q,r,s] G[p,q,r,s] in longdouble."""
    ht, ut = ref._wide(ht), ref._wide(ut)
    return np.sum(ht * rho.T) + np.longdouble(0.25) * np.sum(ut * G)


def spin_squared_matrix(sx, sy, sz, s2, m, N):
    """S^2 = sum_pq s2[p,q] a+_p a_q + sum_i sum_pqrs s_i[p,r] s_i[q,s] a+_p a+_q a_s a_r on ``sector(m, N)`` from the
    Jordan-Wigner matrices (complex128): the operator the reference's ``setup_spin_squared_operator`` describes."""
    ops, sec = ref.annihilators(m), ref.sector(m, N)
    E = ref.one_body_operators(m, N)
    S2 = np.tensordot(np.asarray(s2, dtype=np.complex128), E.astype(np.complex128), axes=((0, 1), (0, 1)))
    if N >= 2:
        low = ref.sector(m, N - 2)
        A = np.array([[(ops[s] @ ops[r])[np.ix_(low, sec)] for s in range(m)] for r in range(m)])
        A = A.reshape(m * m, len(low), len(sec)).astype(np.complex128)
        for si in (sx, sy, sz):
            si = np.asarray(si, dtype=np.complex128)
            w = np.einsum("pr,qs->pqrs", si, si).reshape(m * m, m * m)
            S2 = S2 + np.einsum("axi,axj->ij", A, np.tensordot(w, A, axes=((1,), (0,))))
    return S2
