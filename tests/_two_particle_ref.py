"""NumPy restatement of the pair contraction and of the exact two-particle problem, for the tests of
``qs_pair_contract`` / ``kernels.pair_contract`` and ``two_particle.TwoParticleCI``:

    S[k,p,q] = sum_rs u[p,q,r,s] T[k,r,s]                                     (no conjugation)

by ``numpy.einsum`` in fp64 and in ``numpy.longdouble`` (the exact side of the parity bound), the bound itself, and the
dense Hamiltonian of two particles on the symmetric or antisymmetric pair basis, built from an EXPLICITLY transformed
``u`` (the route the package avoids).  Nothing here imports the package under test."""

import numpy as np

EPS = 2.0 ** -53


def _wide(a):
    return a.astype(np.clongdouble if np.iscomplexobj(a) else np.longdouble)


def pair_contract(u, T, extended=False):
    """``T`` (K, R, S) -> (K, P, Q), or (R, S) -> (P, Q)."""
    if extended:
        u, T = _wide(u), _wide(T)
    return np.einsum("pqrs,rs->pq", u, T) if T.ndim == 2 else np.einsum("pqrs,krs->kpq", u, T)


def gamma(k):
    return k * EPS / (1.0 - k * EPS)


def error_bound(u, T):
    """Any summation order of the Y = R S products of an element of S satisfies |S - S_exact| <= gamma_(Y+2) * A,
    A = the contraction of |u| with |T|; complex products cost a further factor 2 sqrt 2 (as
    ``_mean_field_ref.error_bound``)."""
    Y = u.shape[2] * u.shape[3]
    A = pair_contract(np.abs(u), np.abs(T))
    cplx = np.iscomplexobj(u) or np.iscomplexobj(T)
    return gamma(Y + 2) * A * (2.0 * np.sqrt(2.0) if cplx else 1.0)


def loewdin(s):
    """``X = s^(-1/2)``: orbitals with ``X^H s X = 1``."""
    sv, sU = np.linalg.eigh(s)
    return (sU / np.sqrt(sv)) @ sU.conj().T


def pair_basis(m, sign):
    """Orthonormal vectors (dim, m, m) that span c = sign * c^T: (e_ab + sign e_ba) / sqrt 2 for a < b, and e_aa for
    the symmetric sector."""
    vecs = []
    for a in range(m):
        for b in range(a if sign > 0 else a + 1, m):
            v = np.zeros((m, m))
            v[a, b] += 1.0
            v[b, a] += sign
            vecs.append(v / np.linalg.norm(v))
    return np.array(vecs).reshape(len(vecs), m, m)


def dense_hamiltonian(h, u, C, sign, f=1.0):
    """H on ``pair_basis(m, sign)`` in the orbitals ``C`` (l, m):
    H[(ab),(cd)] = ht[a,c] d_bd + d_ac ht[b,d] + f u_mo[a,b,c,d], ht = C^H h C, u_mo = u transformed index by index."""
    m = C.shape[1]
    ht = C.conj().T @ h @ C
    u_mo = np.einsum("pa,qb,pqrs,rc,sd->abcd", C.conj(), C.conj(), u, C, C, optimize=True)
    eye = np.eye(m)
    full = np.einsum("ac,bd->abcd", ht, eye) + np.einsum("ac,bd->abcd", eye, ht) + f * u_mo
    B = pair_basis(m, sign).reshape(-1, m * m)
    H = B @ full.reshape(m * m, m * m) @ B.T
    return 0.5 * (H + H.conj().T)


def spectrum(h, u, C, sign, f=1.0):
    return np.linalg.eigvalsh(dense_hamiltonian(h, u, C, sign, f))


def spin_double(h, u, C, anti_symmetrize):
    """Spin orbitals 2 p + sigma: ``(h, u, C, f)`` of the doubled problem, u plain (f = 1) or anti-symmetrised
    (f = 1/2: the sum over (r, s) then counts every pair twice)."""
    e2 = np.eye(2)
    h2, C2 = np.kron(h, e2), np.kron(C, e2)
    u2 = np.kron(u, np.einsum("pr,qs->pqrs", e2, e2))
    if anti_symmetrize:
        return h2, u2 - u2.transpose(0, 1, 3, 2), C2, 0.5
    return h2, u2, C2, 1.0
