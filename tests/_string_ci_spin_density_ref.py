"""NumPy oracle of the spin-resolved one- and two-body densities on alpha and beta occupation strings, for the tests of
``kernels.string_ci_density2_spin`` and of ``StringCI``'s observables on it.  With ``E^s_pq = a+_ps a_qs`` on ONE string
list -- ``E^a c = Ea[p,q] c``, ``E^b c = c Eb[p,q]^T`` from ``ref.list_E`` per spin, the intermediate cut to the lists --

    X^st[(pr),(qs)]   = <bra| E^s_pr E^t_qs |ket> = sum_K conj((E^s_rp bra)[K]) (E^t_qs ket)[K]
    Gamma^st[p,q,r,s] = <bra| a+_ps a+_qt a_st a_rs |ket> = X^st[(pr),(qs)] - delta_st delta_qr <bra| E^s_ps |ket>
    rho^s[q, p]       = <bra| E^s_pq |ket>
    Gamma^ba[p,q,r,s] = Gamma^ab[q,p,s,r]
    <S^2>             = S_z (S_z + 1) + N_b - sum_pq Gamma^ab[q,p,p,q]                          (state)
    <H>               = sum ht[p,q] (rho^a + rho^b)[q,p] + 1/2 sum ut[p,q,r,s] (Gamma^aa + Gamma^bb + 2 Gamma^ab)[p,q,r,s]

Every sum runs in ``numpy.longdouble``.

Bounds (derived, not tuned).  An element of Gamma^st is one dot product over the dim determinants of a pass-and-slice
schedule with T partial sums and one subtraction; the expansion of one spin adds nothing (a signed copy).  The standard
dot-product bound, valid for any order of accumulation, as for the spin sum:

    gamma_(dim+T+3) ( sum_K |E^s_rp bra|[K] |E^t_qs ket|[K] + delta_st delta_qr sum_K |bra[K]| |E^s_ps ket|[K] ),

times 2 sqrt 2 for complex products; rho^s by its own row, gamma_(dim+T+3) sum_K |bra[K]| |E^s_pq ket|[K].  A sum of n
elements is bounded by the sum of their bounds."""

import numpy as np

import _string_ci_density_ref as sref
import _string_ci_ref as ref

S2 = sref.S2
BLOCKS = ("aa", "ab", "bb")


def expand_spin(Ea, Eb, c, wide=True):
    """``(Da, Db)``: (E^a_pq c)[K] and (E^b_pq c)[K] for every pq, (m^2, dim) each; ``c`` is (na, nb) or (dim,)."""
    m, na, nb = Ea.shape[0], Ea.shape[2], Eb.shape[2]
    cw = (ref._wide(np.asarray(c)) if wide else np.asarray(c)).reshape(na, nb)
    (Ja, sa), (Jb, sb) = sref._targets(Ea), sref._targets(Eb)
    Da = sa[:, :, None] * cw[Ja]
    Db = sb[:, None, :] * cw[:, Jb].transpose(1, 0, 2)
    return Da.reshape(m * m, na * nb), Db.reshape(m * m, na * nb)


def _as_pqrs(G, m):
    """G[(rp),(qs)] -> [p,q,r,s]."""
    return G.reshape(m, m, m, m).transpose(1, 2, 0, 3).copy()


def spin_gamma(Ea, Eb, bra, ket):
    """``({"aa", "ab", "bb"} -> Gamma^st (m, m, m, m), (rho^a, rho^b))``, rho^s[q, p] = <bra| E^s_pq |ket>."""
    m = Ea.shape[0]
    Db, Dk = dict(zip("ab", expand_spin(Ea, Eb, bra))), dict(zip("ab", expand_spin(Ea, Eb, ket)))
    bc = ref._wide(np.asarray(bra)).reshape(-1).conj()
    e = {s: (bc @ Dk[s].T).reshape(m, m) for s in "ab"}                  # e[s][p, q] = <bra| E^s_pq |ket>
    G = {}
    for st in BLOCKS:
        s, t = st
        G[st] = _as_pqrs(Db[s].conj() @ Dk[t].T, m)
        if s == t:
            for q in range(m):
                G[st][:, q, q, :] -= e[s]
    return G, (e["a"].T.copy(), e["b"].T.copy())


def spin_gamma_bound(Ea, Eb, bra, ket, T):
    """The elementwise bounds above, float64: ``({"aa", "ab", "bb"} -> (m, m, m, m), (rho^a bound, rho^b bound))``, the
    latter in rho's index order; ``T`` from ``qs_string_ci_density2_spin_plan``."""
    m = Ea.shape[0]
    ab = dict(zip("ab", (np.abs(x).astype(np.float64) for x in expand_spin(Ea, Eb, bra, wide=False))))
    ak = dict(zip("ab", (np.abs(x).astype(np.float64) for x in expand_spin(Ea, Eb, ket, wide=False))))
    dim = ak["a"].shape[1]
    cplx = np.iscomplexobj(bra) or np.iscomplexobj(ket)
    scale = ref.gamma(dim + T + 3) * (S2 if cplx else 1.0)
    b0 = np.abs(np.asarray(bra)).reshape(-1).astype(np.float64)
    e = {s: (b0 @ ak[s].T).reshape(m, m) for s in "ab"}
    B = {}
    for st in BLOCKS:
        s, t = st
        B[st] = _as_pqrs(ab[s] @ ak[t].T, m)
        if s == t:
            for q in range(m):
                B[st][:, q, q, :] += e[s]
        B[st] *= scale
    return B, (scale * e["a"].T, scale * e["b"].T)


def transposed(Gab):
    """Gamma^ba[p,q,r,s] = Gamma^ab[q,p,s,r]."""
    return Gab.transpose(1, 0, 3, 2)


def spin_sum(G):
    """Gamma^aa + Gamma^bb + Gamma^ab + Gamma^ba of a dict of blocks (or of their bounds)."""
    return G["aa"] + G["bb"] + G["ab"] + transposed(G["ab"])


def spin_squared(G, Na, Nb):
    """S_z (S_z + 1) + N_b - sum_pq Gamma^ab[q,p,p,q]."""
    return sref.spin_s0(Na, Nb) - np.einsum("qppq->", G["ab"])


def energy(ht, ut, G, rho):
    """sum ht[p,q] (rho^a + rho^b)[q,p] + 1/2 sum ut[p,q,r,s] (Gamma^aa + Gamma^bb + 2 Gamma^ab)[p,q,r,s], longdouble."""
    ht, ut = ref._wide(ht), ref._wide(ut)
    return np.sum(ht * (rho[0] + rho[1]).T) + np.longdouble(0.5) * np.sum(ut * (G["aa"] + G["bb"] + 2 * G["ab"]))
