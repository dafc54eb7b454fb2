"""NumPy oracle of the spin-summed two-body density and of S^2 on alpha and beta occupation strings, for the tests of
``kernels.string_ci_density2`` / ``string_ci_spin_squared`` and of ``StringCI``'s observables on them:

    X[(pr),(qs)]   = <bra| E_pr E_qs |ket> = sum_K conj((E_rp bra)[K]) (E_qs ket)[K]
    Gamma[p,q,r,s] = sum_spins <bra| a+_p a+_q a_s a_r |ket> = X[(pr),(qs)] - delta_qr <bra| E_ps |ket>
    rho[q, p]      = <bra| E_pq |ket>
    S^2            = S_- S_+ + S_z (S_z + 1),     S_+ = sum_p a+_(2p) a_(2p+1)      (spin orbital 2 p + sigma, alpha = 0)

``E`` is either the dense ``ref.dense_E(m, Na, Nb)`` (m, m, dim, dim) on the (Ia, Ib) sector, or a pair ``(Ea, Eb)`` of
one-spin operators from ``ref.list_E`` on two string lists: then ``E_pq c = Ea[p,q] c + c Eb[p,q]^T`` with the
intermediate cut to the lists, which is what the kernels compute on a truncated list.  Every sum runs in
``numpy.longdouble``.  ``dense_spin_squared`` shares nothing with the tables: it is built from the Jordan-Wigner
matrices of ``_det_ci_ref`` on the 2 m spin orbitals and brought to (Ia, Ib) order with ``ref.sector_map``.

Bounds (derived, not tuned).  An element of Gamma is one dot product over the dim determinants of a pass-and-slice
schedule with T partial sums, one subtraction and the additions inside the two expansions: the standard dot-product
bound, valid for any order of accumulation,

    gamma_(dim+T+3) ( sum_K |E_rp bra|[K] |E_qs ket|[K] + delta_qr sum_K |bra[K]| |E_ps ket|[K] ),

times 2 sqrt 2 for complex products.  An element of S^2 c is a sum of at most m^2 + 1 terms:

    gamma_(m^2+2) ( |s0| |c[I]| + sum_pq |c[J_pq(I)]| ),      s0 = S_z (S_z + 1) + N_beta."""

import numpy as np

import _det_ci_ref as dref
import _string_ci_ref as ref

S2 = 2.0 * np.sqrt(2.0)


def _targets(E1):
    """(J, sign) of a one-spin E (m, m, n, n): its rows hold at most one non-zero entry, +-1 at column J."""
    m, n = E1.shape[0], E1.shape[2]
    Ef = E1.reshape(m * m, n, n)
    J = np.abs(Ef).argmax(axis=2)
    return J, np.take_along_axis(Ef, J[:, :, None], axis=2)[:, :, 0]


def expand(E, c, wide=True):
    """(E_pq c)[K] for every pq: (m^2, dim), in longdouble unless ``wide`` is False; ``c`` is (na, nb) or (dim,)."""
    cw = ref._wide(np.asarray(c)) if wide else np.asarray(c)
    if isinstance(E, tuple):
        Ea, Eb = E
        m, na, nb = Ea.shape[0], Ea.shape[2], Eb.shape[2]
        cw = cw.reshape(na, nb)
        (Ja, sa), (Jb, sb) = _targets(Ea), _targets(Eb)
        D = sa[:, :, None] * cw[Ja] + sb[:, None, :] * cw[:, Jb].transpose(1, 0, 2)
        return D.reshape(m * m, na * nb)
    m, dim = E.shape[0], E.shape[2]
    return np.einsum("aij,j->ai", E.reshape(m * m, dim, dim).astype(cw.dtype), cw.reshape(dim))


def _m_of(E):
    return (E[0] if isinstance(E, tuple) else E).shape[0]


def dense_X(E, bra, ket):
    """X[(pr),(qs)] = <bra| E_pr E_qs |ket> (m^2, m^2): row (pr) is the expansion of the bra at (rp)."""
    m = _m_of(E)
    Db, Dk = expand(E, bra), expand(E, ket)
    G = Db.conj() @ Dk.T                                               # G[(rp),(qs)]
    return G.reshape(m, m, m * m).transpose(1, 0, 2).reshape(m * m, m * m)


def dense_gamma(E, bra, ket):
    """``(Gamma, rho)``: Gamma[p,q,r,s] (m, m, m, m) and rho[q, p] = <bra| E_pq |ket> (m, m)."""
    m = _m_of(E)
    e = (ref._wide(np.asarray(bra)).reshape(-1).conj() @ expand(E, ket).T).reshape(m, m)       # e[p, s] = <bra|E_ps|ket>
    G = dense_X(E, bra, ket).reshape(m, m, m, m).transpose(0, 2, 1, 3).copy()                    # X[(pr),(qs)] -> [p,q,r,s]
    for q in range(m):
        G[:, q, q, :] -= e
    return G, e.T.copy()


def gamma_bound(E, bra, ket, T):
    """The elementwise bound of Gamma above (m, m, m, m), float64; ``T`` from ``qs_string_ci_density2_plan``."""
    m = _m_of(E)
    ab, ak = np.abs(expand(E, bra, wide=False)), np.abs(expand(E, ket, wide=False))
    dim = ab.shape[1]
    X = (ab @ ak.T).reshape(m, m, m * m).transpose(1, 0, 2).reshape(m, m, m, m).transpose(0, 2, 1, 3).copy()
    e = (np.abs(np.asarray(bra)).reshape(-1).astype(np.float64) @ ak.T).reshape(m, m)
    for q in range(m):
        X[:, q, q, :] += e
    cplx = np.iscomplexobj(bra) or np.iscomplexobj(ket)
    return ref.gamma(dim + T + 3) * X * (S2 if cplx else 1.0)


def rho_sum_bound(E, bra, ket, T):
    """The same bound for rho[q, p] = <bra| E_pq |ket> (the last row of the product), (m, m) in rho's index order."""
    m = _m_of(E)
    ak = np.abs(expand(E, ket, wide=False))
    e = (np.abs(np.asarray(bra)).reshape(-1).astype(np.float64) @ ak.T).reshape(m, m)
    cplx = np.iscomplexobj(bra) or np.iscomplexobj(ket)
    return ref.gamma(ak.shape[1] + T + 3) * e.T * (S2 if cplx else 1.0)


def dense_spin_squared(m, Na, Nb):
    """S^2 on the (Na, Nb) sector in (Ia, Ib) order, (dim, dim) float64 (its entries are small integers and halves)."""
    N = Na + Nb
    Eso = dref.one_body_operators(2 * m, N)
    dimN = Eso.shape[2]
    Sp = sum(Eso[2 * p, 2 * p + 1] for p in range(m))                  # S_+ = sum_p a+_(p alpha) a_(p beta)
    Sz = 0.5 * sum(Eso[2 * p, 2 * p] - Eso[2 * p + 1, 2 * p + 1] for p in range(m))
    S2m = Sp.T @ Sp + Sz @ (Sz + np.eye(dimN))
    pos, phase = ref.sector_map(m, Na, Nb)
    return S2m[np.ix_(pos, pos)] * phase[:, None] * phase[None, :]


def spin_s0(Na, Nb):
    sz = 0.5 * (Na - Nb)
    return sz * (sz + 1.0) + Nb


def spin_bound(Ea, Eb, Na, Nb, c):
    """The elementwise bound of S^2 c above for ``c`` (K, na, nb), float64."""
    m = Ea.shape[0]
    ca = np.abs(np.asarray(c)).astype(np.float64)
    gathered = np.einsum("qpij,pqbl,kjl->kib", np.abs(Ea), np.abs(Eb), ca, optimize=True)
    return ref.gamma(m * m + 2) * (abs(spin_s0(Na, Nb)) * ca + gathered) * (S2 if np.iscomplexobj(c) else 1.0)


def list_spin_squared(Ea, Eb, Na, Nb, c):
    """S^2 c on two string lists from the one-spin E, longdouble: s0 c - sum_pq Ea[q,p] c Eb[p,q]^T, ``c`` (K, na, nb)."""
    cw = ref._wide(np.asarray(c))
    return spin_s0(Na, Nb) * cw - np.einsum("qpij,pqbl,kjl->kib", Ea.astype(cw.dtype), Eb.astype(cw.dtype), cw, optimize=True)


def spin_sum(G):
    """sum_(sigma, tau) G[2p+sigma, 2q+tau, 2r+sigma, 2s+tau] of a spin-orbital two-body density (2m)^4 -> m^4."""
    return sum(G[a::2, b::2, a::2, b::2] for a in (0, 1) for b in (0, 1))
