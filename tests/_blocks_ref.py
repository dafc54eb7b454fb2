"""CPU restatement of the per-index block transform and of MP2 (imports nothing from the package): the oracle of
tests/test_gpu_transform_blocks.py.

    out[p,q,r,s] = sum_abcd Ct0[p,a] Ct1[q,b] u[a,b,c,d] C2[c,r] C3[d,s]

Bound (derived as _mean_field_ref.error_bound, not tuned): an element of ``out`` is four chained inner products of
length L.  One inner product of length L in ANY order has relative error gamma_(L+1) on its absolute-value sum (L - 1
additions and one multiplication per term, one more for an fma's spare rounding); chaining four gives gamma_(4L+4) on
the absolute-value contraction A, and 4 more cover the conversions at both ends, so
|out - exact| <= gamma_(4L+8) * A element-wise, A = the same contraction on |Ct0|, |Ct1|, |u|, |C2|, |C3|; complex
products cost a further factor 2 sqrt 2.  ``exact`` is the numpy.longdouble evaluation."""

import numpy as np

from _mean_field_ref import EPS, gamma, hermitian_problem, plain_scf  # noqa: F401


def blocks(u, Ct0, Ct1, C2, C3, extended=False):
    """The four contractions in the library's order a, b, d, c."""
    if extended:
        cplx = any(np.iscomplexobj(x) for x in (u, Ct0, Ct1, C2, C3))
        dt = np.clongdouble if cplx else np.longdouble
        u, Ct0, Ct1, C2, C3 = (np.asarray(x).astype(dt) for x in (u, Ct0, Ct1, C2, C3))
    t = np.einsum("pa,abcd->pbcd", Ct0, u)
    t = np.einsum("qb,pbcd->pqcd", Ct1, t)
    t = np.einsum("pqcd,ds->pqcs", t, C3)
    return np.einsum("cr,pqcs->pqrs", C2, t)


def error_bound(u, Ct0, Ct1, C2, C3):
    L = u.shape[0]
    A = blocks(np.abs(u), np.abs(Ct0), np.abs(Ct1), np.abs(C2), np.abs(C3))
    cplx = any(np.iscomplexobj(x) for x in (u, Ct0, Ct1, C2, C3))
    return gamma(4 * L + 8) * A * (2.0 * np.sqrt(2.0) if cplx else 1.0)


def denominators(eps, n_occ):
    eo, ev = eps[:n_occ], eps[n_occ:]
    return eo[:, None, None, None] + eo[None, :, None, None] - ev[None, None, :, None] - ev[None, None, None, :]


def mp2_spatial(g, eps, n_occ):
    """Closed shell: E2 = Re sum g_ijab conj(2 g_ijab - g_jiab) / D."""
    D = denominators(eps, n_occ)
    return float((g * np.conj(2 * g - g.transpose(1, 0, 2, 3)) / D).sum().real)


def mp2_general(g, eps, n_occ, anti_symmetrized):
    """Spin orbitals: E2 = 1/4 sum |G|^2 / D, G = g (anti-symmetrised u) or g_ijab - g_ijba."""
    D = denominators(eps, n_occ)
    G = g if anti_symmetrized else g - g.transpose(0, 1, 3, 2)
    return float((0.25 * np.abs(G) ** 2 / D).sum())


def mp2_tolerance(g, delta, eps, n_occ):
    """The block's element bound ``delta`` through either MP2 formula: a term's numerator is a product of two
    combinations of at most three block elements, so with gm / dm the larger of the two elements (bounds) involved its
    change is at most 3 (2 gm dm + dm^2); plus the rounding of the two final reductions of N terms (any order)."""
    D = np.abs(denominators(eps, n_occ)).astype(np.float64)
    ag = np.abs(g).astype(np.float64)
    delta = np.asarray(delta, dtype=np.float64)
    gm = np.maximum(np.maximum(ag, ag.transpose(1, 0, 2, 3)), ag.transpose(0, 1, 3, 2))
    dm = np.maximum(np.maximum(delta, delta.transpose(1, 0, 2, 3)), delta.transpose(0, 1, 3, 2))
    return float((3.0 * (2.0 * gm * dm + dm * dm) / D).sum() + 2.0 * gamma(g.size + 8) * (3.0 * gm * gm / D).sum())
