"""NumPy restatement of coupled-cluster doubles, for the tests of ``coupled_cluster.CCD`` and of
``qs_pair_contract_antisym`` / ``kernels.pair_contract_antisym``.  Nothing here imports the package under test.

``h`` and ``u`` are transformed FULLY with ``einsum`` (the device code never transforms ``u``), the residual is the
literal sum over slices of the transformed tensor, term by term as the equations are written:

    R^{ab}_{ij} = u^{ab}_{ij} + P(ab) f^b_c t^{ac}_{ij} - P(ij) f^k_j t^{ab}_{ik}
                + 1/2 u^{ab}_{cd} t^{cd}_{ij} + 1/2 u^{kl}_{ij} t^{ab}_{kl} + P(ab) P(ij) u^{kb}_{cj} t^{ac}_{ik}
                + 1/4 u^{kl}_{cd} t^{cd}_{ij} t^{ab}_{kl} + P(ij) u^{kl}_{cd} t^{ac}_{ik} t^{bd}_{jl}
                - 1/2 P(ij) u^{kl}_{cd} t^{dc}_{ik} t^{ab}_{lj} - 1/2 P(ab) u^{kl}_{cd} t^{ac}_{lk} t^{db}_{ij}

with ``P(xy) X = X - X(x <-> y)``, ``t <- t + R / D``, ``D = f_ii + f_jj - f_aa - f_bb``,
``E = 1/4 sum u^{ij}_{ab} t^{ab}_{ij}``.  Every function keeps the dtype it is given, ``numpy.longdouble`` included."""

import numpy as np

EPS = 2.0 ** -53


def _wide(a):
    return a.astype(np.clongdouble if np.iscomplexobj(a) else np.longdouble)


def gamma(k):
    return k * EPS / (1.0 - k * EPS)


def orbital_tensors(h, u, C, n, extended=False):
    """``(f, ut)``: the Fock matrix of the determinant of the ``n`` lowest orbitals and the two-body tensor, both in
    the orbitals ``C`` (``u`` anti-symmetrised already)."""
    if extended:
        h, u, C = _wide(h), _wide(u), _wide(C)
    ht = np.einsum("pa,pq,qb->ab", C.conj(), h, C)
    ut = np.einsum("pa,qb,pqrs,rc,sd->abcd", C.conj(), C.conj(), u, C, C, optimize=True)
    f = ht + np.einsum("piqi->pq", ut[:, :n, :, :n])
    return f, ut


def denominators(f, n):
    e = np.real(np.diagonal(f))
    eo, ev = e[:n], e[n:]
    return -ev[:, None, None, None] - ev[None, :, None, None] + eo[None, None, :, None] + eo[None, None, None, :]


def residual(f, ut, t, n):
    o, v = slice(0, n), slice(n, None)
    ein = np.einsum
    R = ut[v, v, o, o].copy()
    X = ein("bc,acij->abij", f[v, v], t)
    R += X - X.transpose(1, 0, 2, 3)
    Y = ein("kj,abik->abij", f[o, o], t)
    R -= Y - Y.transpose(0, 1, 3, 2)
    R += 0.5 * ein("abcd,cdij->abij", ut[v, v, v, v], t)
    R += 0.5 * ein("klij,abkl->abij", ut[o, o, o, o], t)
    Z = ein("kbcj,acik->abij", ut[o, v, v, o], t)
    R += Z - Z.transpose(1, 0, 2, 3) - Z.transpose(0, 1, 3, 2) + Z.transpose(1, 0, 3, 2)
    oovv = ut[o, o, v, v]
    R += 0.25 * ein("klcd,cdij,abkl->abij", oovv, t, t, optimize=True)
    Q = ein("klcd,acik,bdjl->abij", oovv, t, t, optimize=True)
    R += Q - Q.transpose(0, 1, 3, 2)
    B = ein("klcd,dcik,ablj->abij", oovv, t, t, optimize=True)
    R -= 0.5 * (B - B.transpose(0, 1, 3, 2))
    B2 = ein("klcd,aclk,dbij->abij", oovv, t, t, optimize=True)
    R -= 0.5 * (B2 - B2.transpose(1, 0, 2, 3))
    return R


def energy(ut, t, n):
    return float(np.real(0.25 * np.einsum("ijab,abij->", ut[:n, :n, n:, n:], t)))


def first_order(f, ut, n):
    """``t = u^{ab}_{ij} / D``: the MP2 amplitudes."""
    return ut[n:, n:, :n, :n] / denominators(f, n)


def solve(h, u, C, n, tol=1e-11, max_iter=500):
    """Iterate from the first-order amplitudes until the 2-norm of the residual is below ``tol`` (at most
    ``max_iter`` updates).  Returns ``(energy, t, iterations)``."""
    f, ut = orbital_tensors(h, u, C, n)
    D = denominators(f, n)
    t = ut[n:, n:, :n, :n] / D
    for it in range(max_iter):
        R = residual(f, ut, t, n)
        if np.linalg.norm(R.ravel()) < tol:
            return energy(ut, t, n), t, it
        t = t + R / D
        t = 0.5 * (t - t.transpose(1, 0, 2, 3))          # rounding leaves the anti-symmetric amplitudes; the equations
        t = 0.5 * (t - t.transpose(0, 1, 3, 2))          # do not damp what it adds outside them
    raise AssertionError(f"the reference did not converge in {max_iter} iterations")


def mp2(f, ut, n):
    """``mp2_energy``'s formula for spin orbitals: ``1/4 sum |u_ijab|^2 / D_ijab`` on an anti-symmetrised tensor."""
    g = ut[:n, :n, n:, n:]
    e = np.real(np.diagonal(f))
    eo, ev = e[:n], e[n:]
    D = eo[:, None, None, None] + eo[None, :, None, None] - ev[None, None, :, None] - ev[None, None, None, :]
    return float(0.25 * ((g * g.conj()).real / D).sum())


# -- the kernel's sum: the packed triangle


def triangle(l):
    """(r, s) of the packed positions 0 ... l (l - 1) / 2 - 1: r < s, row-major."""
    return np.triu_indices(l, 1)


def packed_rows(Urows, T, extended=False):
    """``2 sum_{r<s} Urows[x,r,s] T[k,r,s]`` as (K, x): the sum of the pair rows ``Urows[x] = U[p_x, q_x]``, from their
    elements r < s and those of ``T`` alone."""
    r, s = triangle(T.shape[-1])
    A, B = Urows[:, r, s], T[:, r, s]
    if extended:
        A, B = _wide(A), _wide(B)
    return 2 * np.einsum("xt,kt->kx", A, B)


def pair_contract_antisym(U, T, extended=False):
    """``S[k,p,q] = 2 sum_{r<s} U[p,q,r,s] T[k,r,s]`` for p < q, ``S[k,q,p] = -S[k,p,q]``, a zero diagonal -- from the
    elements p < q, r < s of ``U`` and r < s of ``T`` alone."""
    r, s = triangle(U.shape[0])
    packed = packed_rows(U[r, s], T, extended)                                   # (K, pairs): rows (p < q), columns (r < s)
    S = np.zeros(T.shape, dtype=packed.dtype)
    S[:, r, s] = packed
    S[:, s, r] = -packed
    return S


def rows_bound(Urows, T):
    """Any-order bound on the device sum of n = l (l - 1) / 2 products and the (exact) doubling, for the pair rows of
    ``packed_rows``: ``gamma_(n+2) * 2 sum_{r<s} |U||T|``, a further ``2 sqrt 2`` for complex products (as
    ``_two_particle_ref``)."""
    l = T.shape[-1]
    n = l * (l - 1) // 2
    A = np.abs(packed_rows(np.abs(Urows), np.abs(T)))
    return gamma(n + 2) * A * (2.0 * np.sqrt(2.0) if (np.iscomplexobj(Urows) or np.iscomplexobj(T)) else 1.0)


def pair_bound(U, T):
    """``rows_bound`` of every pair row p < q, at (p, q) and at (q, p); zero on the diagonal."""
    r, s = triangle(U.shape[0])
    b = rows_bound(U[r, s], T)
    B = np.zeros(T.shape, dtype=b.dtype)
    B[:, r, s] = b
    B[:, s, r] = b
    return B


# -- seeded inputs


def antisymmetric_problem(l, seed, complex_=False, scale=0.03):
    """Hermitian ``h``, Hermitian anti-symmetrised ``u`` on l spin orbitals (as ``_det_ci_ref.random_hamiltonian``)
    and a non-canonical orthonormal ``C`` (unitary)."""
    rng = np.random.default_rng(seed)

    def draw(*shape):
        x = rng.standard_normal(shape)
        return x + 1j * rng.standard_normal(shape) if complex_ else x

    a = draw(l, l)
    h = 0.5 * (a + a.conj().T) * 0.2 + np.diag(2.0 * np.arange(l))      # levels 2 apart: the plain iteration converges
    w = scale * draw(l, l, l, l)
    v = w + w.conj().transpose(2, 3, 0, 1)
    v = v + v.transpose(1, 0, 3, 2)
    u = v - v.transpose(0, 1, 3, 2)
    g = 0.1 * draw(l, l)
    C = np.linalg.qr(np.eye(l) + g - g.conj().T)[0]                    # near the unit matrix: the reference stays the lowest
    return h, u, C


def antisymmetric_amplitudes(rng, nv, n, complex_=False, scale=0.1):
    x = rng.standard_normal((nv, nv, n, n))
    if complex_:
        x = x + 1j * rng.standard_normal((nv, nv, n, n))
    x = x - x.transpose(1, 0, 2, 3)
    return scale * (x - x.transpose(0, 1, 3, 2))
