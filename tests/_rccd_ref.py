"""NumPy restatement of spin-adapted closed-shell coupled-cluster doubles on spatial orbitals, for the tests of
``coupled_cluster.RCCD`` and of ``qs_pair_contract_exchange`` / ``kernels.pair_contract_exchange``.  Nothing here imports
the package under test.

``h`` and ``u`` are transformed FULLY with ``einsum`` (the device code never transforms ``u``); with ``<pq|rs>`` the
transformed tensor (NOT anti-symmetrised), ``n_s`` doubly occupied orbitals (i, j, k, l), the rest virtual (a, b, c, d),
amplitudes ``t[a,b,i,j] = t[b,a,j,i]`` and ``P X = X^{ab}_{ij} + X^{ba}_{ji}``:

    L_klcd = 2<kl|cd> - <kl|dc>
    W_klij = <kl|ij> + sum_cd <kl|cd> t^{cd}_{ij}
    F_bc = f_bc - sum_kld L_klcd t^{bd}_{kl}                 F_kj = f_kj + sum_lcd L_klcd t^{cd}_{jl}
    Wd_kbcj =  <kb|cj> - 1/2 sum_ld <kl|cd> t^{db}_{jl} + 1/2 sum_ld L_klcd t^{db}_{lj}
    Wx_kbjc = -<kb|jc> + 1/2 sum_ld <kl|dc> t^{db}_{jl}
    R^{ab}_{ij} = <ab|ij> + sum_cd <ab|cd> t^{cd}_{ij} + sum_kl W_klij t^{ab}_{kl}
                + P{ F_bc t^{ac}_{ij} - F_kj t^{ab}_{ik}
                     + sum_kc [(t^{ac}_{ik} - t^{ca}_{ik}) Wd_kbcj + t^{ac}_{ik} (Wd_kbcj + Wx_kbjc) + t^{ac}_{kj} Wx_kbic] }
    D = f_ii + f_jj - f_aa - f_bb,    E = sum (2<ij|ab> - <ij|ba>) t^{ab}_{ij},    f = h~ + 2<pi|qi> - <pi|iq>

Every function keeps the dtype it is given, ``numpy.longdouble`` included."""

import numpy as np

EPS = 2.0 ** -53


def _wide(a):
    return a.astype(np.clongdouble if np.iscomplexobj(a) else np.longdouble)


def gamma(k):
    return k * EPS / (1.0 - k * EPS)


def orbital_tensors(h, u, C, ns, extended=False):
    """``(f, ut)``: the closed-shell Fock matrix of ``ns`` doubly occupied orbitals and ``<pq|rs>``, both in the
    orbitals ``C``."""
    if extended:
        h, u, C = _wide(h), _wide(u), _wide(C)
    ht = np.einsum("pa,pq,qb->ab", C.conj(), h, C)
    ut = np.einsum("pa,qb,pqrs,rc,sd->abcd", C.conj(), C.conj(), u, C, C, optimize=True)
    f = ht + 2 * np.einsum("piqi->pq", ut[:, :ns, :, :ns]) - np.einsum("piiq->pq", ut[:, :ns, :ns, :])
    return f, ut


def denominators(f, ns):
    e = np.real(np.diagonal(f))
    eo, ev = e[:ns], e[ns:]
    return -ev[:, None, None, None] - ev[None, :, None, None] + eo[None, None, :, None] + eo[None, None, None, :]


def residual(f, ut, t, ns):
    o, v = slice(0, ns), slice(ns, None)
    ein = np.einsum
    oovv = ut[o, o, v, v]
    L = 2 * oovv - oovv.transpose(0, 1, 3, 2)
    W = ut[o, o, o, o] + ein("klcd,cdij->klij", oovv, t)
    Fvv = f[v, v] - ein("klcd,bdkl->bc", L, t)
    Foo = f[o, o] + ein("klcd,cdjl->kj", L, t)
    Wd = ut[o, v, v, o] - 0.5 * ein("klcd,dbjl->kbcj", oovv, t) + 0.5 * ein("klcd,dblj->kbcj", L, t)
    Wx = -ut[o, v, o, v] + 0.5 * ein("kldc,dbjl->kbjc", oovv, t)
    R = ut[v, v, o, o] + ein("abcd,cdij->abij", ut[v, v, v, v], t) + ein("klij,abkl->abij", W, t)
    X = ein("bc,acij->abij", Fvv, t) - ein("kj,abik->abij", Foo, t)
    X = X + ein("acik,kbcj->abij", t - t.transpose(1, 0, 2, 3), Wd)
    X = X + ein("acik,kbcj->abij", t, Wd + Wx.transpose(0, 1, 3, 2))
    X = X + ein("ackj,kbic->abij", t, Wx)
    return R + X + X.transpose(1, 0, 3, 2)


def energy(ut, t, ns):
    g = ut[:ns, :ns, ns:, ns:]
    return float(np.real(np.einsum("ijab,abij->", 2 * g - g.transpose(0, 1, 3, 2), t)))


def first_order(f, ut, ns):
    """``t = <ab|ij> / D``: the MP2 amplitudes."""
    return ut[ns:, ns:, :ns, :ns] / denominators(f, ns)


def solve(h, u, C, ns, tol=1e-11, max_iter=500):
    """Iterate from the first-order amplitudes until the 2-norm of the residual is below ``tol`` (at most
    ``max_iter`` updates).  Returns ``(energy, t, iterations)``."""
    f, ut = orbital_tensors(h, u, C, ns)
    D = denominators(f, ns)
    t = ut[ns:, ns:, :ns, :ns] / D
    for it in range(max_iter):
        R = residual(f, ut, t, ns)
        if np.linalg.norm(R.ravel()) < tol:
            return energy(ut, t, ns), t, it
        t = t + R / D
        t = 0.5 * (t + t.transpose(1, 0, 3, 2))          # back onto t^{ab}_{ij} = t^{ba}_{ji}
    raise AssertionError(f"the reference did not converge in {max_iter} iterations")


def mp2(f, ut, ns):
    """Closed-shell MP2: ``sum <ij|ab>^* (2<ij|ab> - <ij|ba>) / D_ijab``."""
    g = ut[:ns, :ns, ns:, ns:]
    e = np.real(np.diagonal(f))
    eo, ev = e[:ns], e[ns:]
    D = eo[:, None, None, None] + eo[None, :, None, None] - ev[None, None, :, None] - ev[None, None, None, :]
    return float(((g.conj() * (2 * g - g.transpose(0, 1, 3, 2))).real / D).sum())


# -- the spin-doubled problem: spin orbital 2 P + sigma


def spin_double(h, u, C):
    """``(h, u, C)`` on 2 l spin orbitals 2 P + sigma, ``u`` anti-symmetrised: the input of ``_ccd_ref``."""
    one = np.eye(2)
    l = h.shape[0]
    hs = np.kron(h, one)
    us = np.einsum("pqrs,ac,bd->paqbrcsd", u, one, one).reshape(2 * l, 2 * l, 2 * l, 2 * l)
    return hs, us - us.transpose(0, 1, 3, 2), np.kron(C, one)


def embed(t):
    """The spin-orbital amplitudes of the closed-shell ``t`` (v, v, o, o), ``t[a,b,i,j] = t[b,a,j,i]``:
    ``T[a s, b s', i s, j s'] = t[a,b,i,j]`` minus the same with the upper pair exchanged."""
    nv, no = t.shape[0], t.shape[2]
    one = np.eye(2)
    d = np.einsum("abij,su,tw->asbtiujw", t, one, one)                       # delta(sa, si) delta(sb, sj)
    x = np.einsum("baij,sw,tu->asbtiujw", t, one, one)                       # t[b,a,i,j] delta(sa, sj) delta(sb, si)
    return (d - x).reshape(2 * nv, 2 * nv, 2 * no, 2 * no)


def block(T):
    """The alpha-beta-alpha-beta block of spin-orbital amplitudes: the closed-shell ``t``."""
    return T[0::2, 1::2, 0::2, 1::2]


# -- the kernel's sum: the packed triangle with its diagonal


def triangle(l):
    """(r, s) of the packed positions 0 ... l (l + 1) / 2 - 1: r <= s, row-major."""
    return np.triu_indices(l)


def packed_rows(Arows, Brows, T, extended=False):
    """``(S[k, p_x, q_x], S[k, q_x, p_x])`` as two (K, x), for the row pairs ``Arows[x] = U[p_x, q_x]`` and
    ``Brows[x] = U[q_x, p_x]``, p <= q, from their elements r <= s alone:
    ``S+- = sum_{r<=s} w (U[p,q,r,s] +- U[q,p,r,s]) (T[r,s] +- T[s,r])``."""
    r, s = triangle(T.shape[-1])
    a, b, t, tt = Arows[:, r, s], Brows[:, r, s], T[:, r, s], T[:, s, r]     # columns (r <= s)
    if extended:
        a, b, t, tt = _wide(a), _wide(b), _wide(t), _wide(tt)
    Sp = np.einsum("xt,kt->kx", a + b, (t + tt) * np.where(r == s, 0.5, 1.0))
    Sm = np.einsum("xt,kt->kx", a - b, t - tt)
    return (Sp + Sm) / 2, (Sp - Sm) / 2


def pair_contract_exchange(U, T, extended=False):
    """``S[k,p,q] = sum_rs U[p,q,r,s] T[k,r,s]`` for a ``U`` with ``U[p,q,r,s] = U[q,p,s,r]``, from the elements
    r <= s of ``U`` alone (``packed_rows`` of every row pair p <= q)."""
    r, s = triangle(U.shape[0])
    upper, lower = packed_rows(U[r, s], U[s, r], T, extended)
    S = np.zeros(T.shape, dtype=upper.dtype)
    S[:, s, r] = lower
    S[:, r, s] = upper
    return S


def rows_bound(Arows, Brows, T):
    """Any-order bound on the device sums of n = l (l + 1) / 2 products each, the two combinations before them, the one
    after and the (exact) halving, for the row pairs of ``packed_rows`` (the same at (p, q) and (q, p)):
    ``gamma_(n+4) sum_{r<=s} w (|U[p,q,r,s]| + |U[q,p,r,s]|) (|T[r,s]| + |T[s,r]|)``, a further ``2 sqrt 2`` for complex
    products."""
    l = T.shape[-1]
    n = l * (l + 1) // 2
    r, s = triangle(l)
    a, b, t = np.abs(Arows)[:, r, s], np.abs(Brows)[:, r, s], np.abs(T)
    A = np.einsum("xt,kt->kx", a + b, (t[:, r, s] + t[:, s, r]) * np.where(r == s, 0.5, 1.0))
    return gamma(n + 4) * A * (2.0 * np.sqrt(2.0) if (np.iscomplexobj(Arows) or np.iscomplexobj(T)) else 1.0)


def pair_bound(U, T):
    """``rows_bound`` of every row pair p <= q, at (p, q) and at (q, p)."""
    r, s = triangle(U.shape[0])
    b = rows_bound(U[r, s], U[s, r], T)
    B = np.zeros(T.shape, dtype=np.float64)
    B[:, r, s] = b
    B[:, s, r] = b
    return B


# -- seeded inputs


def closed_shell_problem(ls, seed, complex_=False, scale=0.03):
    """Hermitian ``h``, a Hermitian ``u`` with particle-exchange symmetry on ``ls`` spatial orbitals and a non-canonical
    orthonormal ``C`` (unitary): ``_ccd_ref.antisymmetric_problem`` without its last anti-symmetrisation."""
    rng = np.random.default_rng(seed)

    def draw(*shape):
        x = rng.standard_normal(shape)
        return x + 1j * rng.standard_normal(shape) if complex_ else x

    a = draw(ls, ls)
    h = 0.5 * (a + a.conj().T) * 0.2 + np.diag(2.0 * np.arange(ls))      # levels 2 apart: the plain iteration converges
    w = scale * draw(ls, ls, ls, ls)
    v = w + w.conj().transpose(2, 3, 0, 1)
    u = v + v.transpose(1, 0, 3, 2)
    g = 0.1 * draw(ls, ls)
    C = np.linalg.qr(np.eye(ls) + g - g.conj().T)[0]                    # near the unit matrix: the reference stays the lowest
    return h, u, C


def closed_shell_amplitudes(rng, nv, ns, complex_=False, scale=0.1):
    x = rng.standard_normal((nv, nv, ns, ns))
    if complex_:
        x = x + 1j * rng.standard_normal((nv, nv, ns, ns))
    return scale * (x + x.transpose(1, 0, 3, 2))
