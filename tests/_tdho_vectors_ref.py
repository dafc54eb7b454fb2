"""NumPy restatement of the Coulomb vectors of the 2-D harmonic oscillator -- TEST INFRASTRUCTURE ONLY, the
CPU reference of ``qs_tdho_coulomb_vectors``, built on ``_tdho_quadrature_ref.Quadrature``.

    u[p,q,r,s] = delta(m_p + m_q, m_r + m_s) sum_g wt_g F_pr[g] F_qs[g] = sum_x L_x[r,p] L_x[q,s]

    x = j R + g,   mu_j = j - (m_max - m_min),   L_x[q,s] = sqrt(wt_g) F_qs[g] where m_s - m_q == mu_j, +0.0 elsewhere

The delta splits by the transfer mu = m_p - m_r = m_s - m_q; F is symmetric, so M_x = L_x^T carries the band -mu.
"""

import numpy as np

import _tdho_quadrature_ref as qref

ASYMMETRIC = [(0, 0), (0, -1), (1, 0), (0, -2), (0, 3), (2, 1), (1, -1)]


def table(l=None, nm=None):
    return qref.shell_table(l) if nm is None else np.asarray(nm, dtype=np.int64).reshape(-1, 2)


def m_span(nm):
    m = np.asarray(nm)[:, 1]
    return int(m.max() - m.min())


def rank(nm):
    """R (2 (m_max - m_min) + 1)."""
    return qref.max_shell(nm) * (2 * m_span(nm) + 1)


def full_shell_rank(R):
    return R * (4 * R - 3)


def vectors(nm, quadrature=None, x_lo=0, x_hi=None):
    """L (x_hi - x_lo, l, l) of the orbital table nm."""
    quad = qref.Quadrature(nm) if quadrature is None else quadrature
    R, span, m = len(quad.k), m_span(nm), quad.m
    x_hi = rank(nm) if x_hi is None else x_hi
    root = np.sqrt(quad.w)
    transfer = m[None, :] - m[:, None]                       # [q, s] -> m_s - m_q
    out = np.zeros((x_hi - x_lo, len(m), len(m)))
    for x in range(x_lo, x_hi):
        j, g = divmod(x, R)
        out[x - x_lo] = np.where(transfer == j - span, root[g] * quad.F[:, :, g], 0.0)
    return out


def reconstruct(L, M=None):
    """u[p,q,r,s] = sum_x M[x,p,r] L[x,q,s], M_x = L_x^H by default."""
    M = L.conj().transpose(0, 2, 1) if M is None else M
    return np.einsum("xpr,xqs->pqrs", M, L, optimize=True)


def mean_field(L, D, cj, ck):
    """W[p,q] = cj sum_rs u[p,r,q,s] D[s,r] + ck sum_rs u[p,r,s,q] D[s,r] on the vectors."""
    M = L.conj().transpose(0, 2, 1)
    W = cj * np.einsum("x,xpq->pq", np.einsum("xrs,sr->x", L, D), M)
    return W + ck * np.einsum("xps,sr,xrq->pq", M, D, L, optimize=True)


def mean_field_tensor(u, D, cj, ck):
    return cj * np.einsum("prqs,sr->pq", u, D) + ck * np.einsum("prsq,sr->pq", u, D)


def transform(L, C, C_tilde=None):
    """(L', M') in the basis C."""
    Ct = C.conj().T if C_tilde is None else C_tilde
    M = L.conj().transpose(0, 2, 1)
    return np.einsum("pa,xab,bq->xpq", Ct, L, C, optimize=True), np.einsum("pa,xab,bq->xpq", Ct, M, C, optimize=True)


def transform_tensor(u, C, C_tilde=None):
    Ct = C.conj().T if C_tilde is None else C_tilde
    return np.einsum("pa,qb,abcd,cr,ds->pqrs", Ct, Ct, u, C, C, optimize=True)
