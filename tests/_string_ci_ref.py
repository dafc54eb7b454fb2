"""NumPy restatement of the spin-free problem of ``string_ci.StringCI`` / ``kernels.string_ci_*``, sharing nothing with
the kernels.  The Hamiltonian of Na alpha and Nb beta particles in m spatial orbitals is built from ``_det_ci_ref``'s
Jordan-Wigner matrices on the 2 m spin orbitals ``2 p + sigma`` (alpha = 0): one-body input ``kron(ht, 1_2)``, two-body
input the spin-doubled, anti-symmetrised ``ut``; it is restricted to the (Na, Nb) sector in the interleaved ordering and
conjugated into ``(Ia, Ib)`` order ("all alpha creators first", Ib fastest).  The phase of that conjugation is the
parity of the permutation that sorts the creators, counted inversion by inversion -- no closed formula.  The dense
``E_pq = sum_spin a+_p,spin a_q,spin`` on the sector serve the Knowles-Handy path and its error bound.

Past the dense Fock space, ``list_E`` gives ``E_pq`` of ONE spin on any list of strings from ``_det_ci_ref``'s ladder
operators (a target outside the list contributes nothing), and ``kh_sigma`` the Knowles-Handy sum on them."""

import numpy as np

import _det_ci_ref as dref
from _det_ci_ref import EPS, gamma, popcount  # noqa: F401

SHAPES = [(3, 1, 1), (4, 2, 2), (4, 2, 1), (4, 3, 1), (4, 1, 0), (4, 4, 2)]     # (m, Na, Nb)


def _wide(a):
    return a.astype(np.clongdouble if np.iscomplexobj(a) else np.longdouble)


def random_hamiltonian(m, seed, complex_=False, scale=0.3):
    """Hermitian ``ht`` (m, m) and a plain two-body tensor with ut[pqrs] = conj(ut[rspq]) = ut[qpsr]."""
    rng = np.random.default_rng(seed)

    def draw(*shape):
        x = rng.standard_normal(shape)
        return x + 1j * rng.standard_normal(shape) if complex_ else x

    a = draw(m, m)
    ht = 0.5 * (a + a.conj().T) + np.diag(np.arange(m, dtype=float))
    w = scale * draw(m, m, m, m)
    v = w + w.conj().transpose(2, 3, 0, 1)
    return ht, v + v.transpose(1, 0, 3, 2)


def strings(m, N):
    """Ascending masks of N particles of one spin in m orbitals ([0] for N = 0)."""
    return np.array([x for x in range(1 << m) if popcount(x) == N], dtype=np.int64)


def spin_orbital_inputs(ht, ut):
    """``kron(ht, 1_2)`` and the spin-doubled, anti-symmetrised ``ut`` on spin orbitals 2 p + sigma."""
    m = ht.shape[0]
    eye = np.eye(2)
    h2 = np.kron(ht, eye)
    u2 = np.einsum("pqrs,ac,bd->paqbrcsd", ut, eye, eye).reshape(2 * m, 2 * m, 2 * m, 2 * m)
    return h2, u2 - u2.transpose(0, 1, 3, 2)


def _interleaved(a, b, m):
    return sum(((a >> p) & 1) << (2 * p) | ((b >> p) & 1) << (2 * p + 1) for p in range(m))


def _parity(a, b, m):
    """Sign of the permutation that sorts the creators (alpha ascending, then beta ascending) by spin orbital."""
    seq = [2 * p for p in range(m) if (a >> p) & 1] + [2 * p + 1 for p in range(m) if (b >> p) & 1]
    inv = sum(1 for i in range(len(seq)) for j in range(i + 1, len(seq)) if seq[i] > seq[j])
    return -1.0 if inv & 1 else 1.0


def sector_map(m, Na, Nb):
    """``(pos, phase)`` over (Ia, Ib) row-major: the position of every determinant in ``dref.sector(2 m, Na + Nb)`` and
    the sign between the two creator orders."""
    sec = {int(x): i for i, x in enumerate(dref.sector(2 * m, Na + Nb))}
    pos, phase = [], []
    for a in strings(m, Na):
        for b in strings(m, Nb):
            pos.append(sec[_interleaved(int(a), int(b), m)])
            phase.append(_parity(int(a), int(b), m))
    return np.array(pos), np.array(phase)


def dense_hamiltonian(ht, ut, Na, Nb, extended=False):
    """H on the (Na, Nb) sector in (Ia, Ib) order."""
    m = ht.shape[0]
    h2, u2 = spin_orbital_inputs(ht, ut)
    H = dref.dense_hamiltonian(h2, u2, Na + Nb, extended=extended)
    pos, phase = sector_map(m, Na, Nb)
    return H[np.ix_(pos, pos)] * phase[:, None] * phase[None, :]


def dense_E(m, Na, Nb):
    """E[p, q] = sum_spin a+_p,spin a_q,spin on the sector in (Ia, Ib) order: (m, m, dim, dim), entries 0, +-1, 2."""
    Eso = dref.one_body_operators(2 * m, Na + Nb)
    pos, phase = sector_map(m, Na, Nb)
    E = Eso[0::2, 0::2] + Eso[1::2, 1::2]
    return E[:, :, pos][:, :, :, pos] * phase[:, None] * phase[None, :]


def kh_operands(ht, ut):
    """``k[p,r] = ht[p,r] - 1/2 sum_q ut[p,q,q,r]`` and ``W[(pr),(qs)] = 1/2 ut[p,q,r,s]`` (m^2, m^2)."""
    m = ht.shape[0]
    return ht - 0.5 * np.einsum("pqqr->pr", ut), 0.5 * ut.transpose(0, 2, 1, 3).reshape(m * m, m * m)


def kh_hamiltonian(k, W, E):
    """sum_pr E_pr (k[p,r] + sum_qs W[(pr),(qs)] E_qs) from dense E (m, m, dim, dim)."""
    m, dim = E.shape[0], E.shape[2]
    Ef = E.reshape(m * m, dim, dim).astype(W.dtype)
    inner = np.tensordot(W, Ef, axes=((1,), (0,))) + k.reshape(m * m)[:, None, None] * np.eye(dim)
    return np.einsum("aij,ajk->ik", Ef, inner)


def path_bound(k, W, E, c):
    """|sigma - exact| <= gamma_n sum_pr |E_pr| (|k_pr| |c| + sum_qs |W_pr,qs| |E_qs| |c|) elementwise, n = 3 m^2 + 4;
    complex products cost a further 2 sqrt 2.  ``c`` is (K, dim)."""
    m, dim = E.shape[0], E.shape[2]
    Ea = np.abs(E).reshape(m * m, dim, dim)
    ca = np.abs(c).astype(np.float64)
    Dc = np.einsum("aij,kj->aki", Ea, ca)
    X = np.tensordot(np.abs(W), Dc, axes=((1,), (0,))) + np.abs(k).reshape(m * m)[:, None, None] * ca[None]
    b = np.einsum("aij,akj->ki", Ea, X)
    cplx = np.iscomplexobj(k) or np.iscomplexobj(W) or np.iscomplexobj(c)
    return gamma(3 * m * m + 4) * b * (2.0 * np.sqrt(2.0) if cplx else 1.0)


def diagonal_terms(ht, ut, Na, Nb):
    """``(D, S)``: the diagonal formula in longdouble and the sum of the moduli of its terms, (na, nb) each."""
    m = ht.shape[0]
    sa, sb = strings(m, Na), strings(m, Nb)
    D = np.zeros((len(sa), len(sb)), dtype=np.longdouble)
    S = np.zeros((len(sa), len(sb)))
    hw, uw = _wide(ht), _wide(ut)
    for i, a in enumerate(sa):
        for j, b in enumerate(sb):
            na = np.array([(int(a) >> p) & 1 for p in range(m)])
            nb = np.array([(int(b) >> p) & 1 for p in range(m)])
            n = na + nb
            for p in range(m):
                t = [n[p] * hw[p, p].real]
                for q in range(m):
                    t.append(0.5 * n[p] * n[q] * uw[p, q, p, q].real)
                    t.append(-0.5 * (na[p] * na[q] + nb[p] * nb[q]) * uw[p, q, q, p].real)
                D[i, j] += sum(t)
                S[i, j] += float(sum(abs(x) for x in t))
    return D, S


def table_from_E(E1):
    """The replacement table (n, m^2) of one spin from its dense E (m, m, n, n) with entries 0, +-1."""
    m, n = E1.shape[0], E1.shape[2]
    T = np.zeros((n, m * m), dtype=np.int32)
    for p in range(m):
        for q in range(m):
            K, J = np.nonzero(E1[p, q])
            assert len(set(K)) == len(K)
            T[K, p * m + q] = (np.sign(E1[p, q][K, J]) * (J + 1)).astype(np.int32)
    return T


def list_E(strs, m):
    """E[p, q] = a+_p a_q of ONE spin on the ascending list ``strs`` (m, m, n, n), from the ladder operators of
    ``_det_ci_ref``; a target outside the list contributes nothing.  An empty string list entry [0] gives zeros."""
    dets, start = dref._start(strs)
    n = len(dets)
    E = np.zeros((m, m, n, n))
    for q in range(m):
        lowered = dref._ladder(start, q, False)
        for p in range(m):
            col, row, sign = dref._land(dets, dref._ladder(lowered, p, True))
            E[p, q, row, col] = sign
    return E


def kh_sigma(k, W, Ea, Eb, c):
    """The Knowles-Handy sum on two string lists in longdouble: ``c`` (K, na, nb) -> sigma (K, na, nb)."""
    m, na, nb = Ea.shape[0], Ea.shape[2], Eb.shape[2]
    cw, kw, Ww = _wide(np.asarray(c)), _wide(k).reshape(m * m), _wide(W)
    dt = np.result_type(cw.dtype, kw.dtype)
    Ea, Eb = Ea.reshape(m * m, na, na).astype(dt), Eb.reshape(m * m, nb, nb).astype(dt)
    D = np.einsum("aij,kjb->akib", Ea, cw) + np.einsum("abj,kij->akib", Eb, cw)
    X = np.tensordot(Ww.astype(dt), D, axes=((1,), (0,))) + kw[:, None, None, None] * cw[None]
    return np.einsum("aij,akjb->kib", Ea, X) + np.einsum("abj,akij->kib", Eb, X)
