"""NumPy restatement of the N-particle problem on Slater determinants, for the tests of ``qs_det_ci_*`` /
``kernels.det_ci_*`` and ``determinant_ci.DeterminantCI``:

    H = sum_pq ht[p,q] a+_p a_q + 1/4 sum_pqrs ut[p,q,r,s] a+_p a+_q a_s a_r

built from the Jordan-Wigner matrices of ``a_p`` on the 2^m Fock space (bit p of a state's index = orbital p occupied)
and restricted to the N-particle states in ascending order of their masks.  No Slater-Condon rule, no phase from a
popcount and no excitation list appears here: a sign or index-order mistake in the kernels is not mirrored.  The pair
operators ``a_s a_r`` are cut to the (N -> N - 2)-particle block before the O(m^4) sum, so m <= 8 takes well under a
second.

Past m = 8 a second oracle, ``string_hamiltonian`` / ``string_density``, applies the same operator strings term by term
to a LIST of masks with the textbook sign of ``a_p`` (462 determinants of 11 orbitals in about a second, orbitals up
to 62); tests/test_det_ci_ref_host.py pins it against the Jordan-Wigner matrices.  Nothing here imports the package
under test."""

from math import comb

import numpy as np

EPS = 2.0 ** -53
M_MAX = 8


def _wide(a):
    return a.astype(np.clongdouble if np.iscomplexobj(a) else np.longdouble)


def gamma(k):
    return k * EPS / (1.0 - k * EPS)


def popcount(x):
    return bin(int(x)).count("1")


def sector(m, N):
    """Masks of the N-particle states of m orbitals, ascending."""
    return np.array([x for x in range(1 << m) if popcount(x) == N], dtype=np.int64)


def annihilators(m):
    """Jordan-Wigner: a_p = 1 x ... x 1 x a x Z x ... x Z with p factors Z on the low-bit side, a = |0><1|."""
    assert 1 <= m <= M_MAX, "the dense Fock space is meant for m <= 8"
    a, z, one = np.array([[0.0, 1.0], [0.0, 0.0]]), np.diag([1.0, -1.0]), np.eye(2)
    ops = []
    for p in range(m):
        op = np.ones((1, 1))
        for k in range(m - 1, -1, -1):                  # the leftmost factor is the highest bit
            op = np.kron(op, a if k == p else (z if k < p else one))
        ops.append(op)
    return ops


def one_body_operators(m, N):
    """E[p, q] = a+_p a_q on the N-particle sector: (m, m, dim, dim), real."""
    ops, sec = annihilators(m), sector(m, N)
    cut = [op[:, sec] for op in ops]                    # N -> N - 1 particles, all rows kept
    return np.array([[cut[p].T @ cut[q] for q in range(m)] for p in range(m)])


def dense_hamiltonian(ht, ut, N, extended=False):
    """H on ``sector(m, N)``; with ``extended`` every sum runs in ``numpy.longdouble``."""
    m = ht.shape[0]
    if extended:
        ht, ut = _wide(ht), _wide(ut)
    ops, sec = annihilators(m), sector(m, N)
    dim = len(sec)
    E = one_body_operators(m, N)
    H = np.tensordot(ht, E.astype(ht.dtype), axes=((0, 1), (0, 1)))
    if N >= 2:
        low = sector(m, N - 2)
        # A[r, s] = a_s a_r from N to N - 2 particles: (m * m, len(low) * dim)
        A = np.array([[(ops[s] @ ops[r])[np.ix_(low, sec)] for s in range(m)] for r in range(m)])
        A = A.reshape(m * m, len(low), dim).astype(ut.dtype)
        B = np.tensordot(ut.reshape(m * m, m * m), A, axes=((1,), (0,)))          # sum_rs ut[pq, rs] a_s a_r
        H = H + 0.25 * np.einsum("axi,axj->ij", A, B)                                 # a+_p a+_q = (a_q a_p)^T
    return H


def random_hamiltonian(m, seed, complex_=False, scale=0.3):
    """Hermitian ``ht`` (m, m) and Hermitian, anti-symmetrised ``ut`` (m, m, m, m):
    ut[pqrs] = -ut[qprs] = -ut[pqsr] = conj(ut[rspq])."""
    rng = np.random.default_rng(seed)

    def draw(*shape):
        x = rng.standard_normal(shape)
        return x + 1j * rng.standard_normal(shape) if complex_ else x

    a = draw(m, m)
    ht = 0.5 * (a + a.conj().T) + np.diag(np.arange(m, dtype=float))
    w = scale * draw(m, m, m, m)
    v = w + w.conj().transpose(2, 3, 0, 1)
    v = v + v.transpose(1, 0, 3, 2)
    return ht, v - v.transpose(0, 1, 3, 2)


def terms(m, N):
    """Products behind one element of sigma: the diagonal, the single and the double excitations, and the N values a
    single excitation's matrix element is summed from."""
    return 1 + N * (m - N) + comb(N, 2) * comb(m - N, 2) + N


def error_bound(H, c, m, N):
    """|sigma - sigma_exact| <= gamma_(n+2) (|H| |c|) elementwise for any order of the n = ``terms(m, N)`` summands;
    complex products cost a further factor 2 sqrt 2 (as ``_two_particle_ref.error_bound``).  ``c`` is (K, dim)."""
    A = np.abs(c).astype(np.float64) @ np.abs(H).astype(np.float64).T
    cplx = np.iscomplexobj(H) or np.iscomplexobj(c)
    return gamma(terms(m, N) + 2) * A * (2.0 * np.sqrt(2.0) if cplx else 1.0)


def sigma(H, c, extended=False):
    """sigma[k, I] = sum_J H[I, J] c[k, J]."""
    if extended:
        H, c = _wide(H), _wide(c)
    return c @ H.T


def one_body_density(c, m, N):
    """rho[q, p] = <c| a+_p a_q |c> for one vector on ``sector(m, N)``, in ``numpy.longdouble``."""
    E = one_body_operators(m, N)
    cw = _wide(c)
    return np.einsum("i,pqij,j->qp", cw.conj(), E.astype(cw.dtype), cw)


def density_bound(c, m, N):
    """Each element is a sum of at most dim products c*_I c_J: gamma_(dim+2) sum_I |c_I| |c_J(I)| <= gamma_(dim+2) |c|^2."""
    dim = len(c)
    return gamma(dim + 2) * float(np.sum(np.abs(c) ** 2)) * (2.0 * np.sqrt(2.0) if np.iscomplexobj(c) else 1.0)


# ---- a second oracle that scales past M_MAX: the operator strings applied to a LIST of masks, term by term ----------
# a_p |I> = (-1)^popcount(I & (2^p - 1)) |I - p>, zero if p is empty; a+_p is its adjoint (the same sign on the state it
# fills).  A state is (mask, sign, alive) per determinant of the list; an operator string is applied factor by factor,
# right to left.  No case analysis, no count between two orbitals, no excitation list, no symmetry of ut.


def _bits(x):
    """Set bits of every non-negative int64 of an array."""
    return np.unpackbits(np.ascontiguousarray(x, dtype=np.int64).view(np.uint8).reshape(-1, 8), axis=1).sum(axis=1)


def _ladder(state, p, fill):
    """a+_p (``fill``) or a_p on every (mask, sign, alive) of ``state``."""
    mask, sign, alive = state
    bit = np.int64(1) << np.int64(p)
    occupied = (mask & bit) != 0
    odd = (_bits(mask & (bit - np.int64(1))) & 1) != 0
    return mask ^ bit, np.where(odd, -sign, sign), alive & (~occupied if fill else occupied)


def _start(dets):
    dets = np.ascontiguousarray(dets, dtype=np.int64)
    assert dets.ndim == 1 and (dets >= 0).all() and (np.diff(dets) > 0).all(), "an ascending list of masks"
    return dets, (dets, np.ones(len(dets), dtype=np.int64), np.ones(len(dets), dtype=bool))


def _land(dets, state):
    """(col, row, sign) of the states that are alive and in the list: string |dets[col]> = sign |dets[row]>."""
    mask, sign, alive = state
    pos = np.minimum(np.searchsorted(dets, mask), len(dets) - 1)
    hit = alive & (dets[pos] == mask)
    col = np.nonzero(hit)[0]
    return col, pos[col], sign[col]


def string_hamiltonian(ht, ut, dets, moduli=False):
    """H on the ascending int64 masks ``dets`` (any list: a full sector or a subset), in ``numpy.longdouble``:
    every non-zero ht[p,q] adds ht[p,q] a+_p a_q, every non-zero ut[p,q,r,s] adds 1/4 ut[p,q,r,s] a+_p a+_q a_s a_r; a
    target outside the list contributes nothing.  One string maps a determinant to at most one target, so the (row,
    column) pairs of one term are distinct.  With ``moduli`` the sum of the moduli of the terms of every element."""
    dets, start = _start(dets)
    dim = len(dets)
    ht, ut = _wide(ht), _wide(ut)
    H = np.zeros((dim, dim), dtype=np.longdouble if moduli else ht.dtype)

    def add(state, value):
        col, row, sign = _land(dets, state)
        H[row, col] += abs(value) if moduli else value * sign

    for q in np.nonzero((ht != 0).any(axis=0))[0]:
        lowered = _ladder(start, q, False)
        for p in np.nonzero(ht[:, q])[0]:
            add(_ladder(lowered, p, True), ht[p, q])
    quarter = np.longdouble(0.25)
    for r, s in zip(*np.nonzero((ut != 0).any(axis=(0, 1)))):
        lowered = _ladder(_ladder(start, r, False), s, False)                      # a_s a_r, once per (r, s)
        if not lowered[2].any():
            continue
        for q in np.nonzero((ut[:, :, r, s] != 0).any(axis=0))[0]:
            raised = _ladder(lowered, q, True)
            for p in np.nonzero(ut[:, q, r, s])[0]:
                add(_ladder(raised, p, True), quarter * ut[p, q, r, s])
    return H


def string_density(c, dets, m):
    """rho[q, p] = <c| a+_p a_q |c> of one vector on the list ``dets``, in ``numpy.longdouble``, from the same a_p."""
    dets, start = _start(dets)
    cw = _wide(np.asarray(c))
    rho = np.zeros((m, m), dtype=cw.dtype)
    for q in range(m):
        lowered = _ladder(start, q, False)
        for p in range(m):
            col, row, sign = _land(dets, _ladder(lowered, p, True))
            rho[q, p] = np.sum(cw[row].conj() * sign * cw[col])
    return rho


def loewdin(s):
    sv, sU = np.linalg.eigh(s)
    return (sU / np.sqrt(sv)) @ sU.conj().T


def orbital_hamiltonian(h, u, C, anti_symmetrized):
    """``ht = C^H h C`` and the anti-symmetrised ``ut`` in the orbitals ``C`` from the basis's ``h`` and ``u``."""
    ht = C.conj().T @ h @ C
    um = np.einsum("pa,qb,pqrs,rc,sd->abcd", C.conj(), C.conj(), u, C, C, optimize=True)
    return ht, (um if anti_symmetrized else um - um.transpose(0, 1, 3, 2))
