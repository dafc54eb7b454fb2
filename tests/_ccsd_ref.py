"""NumPy restatement of closed-shell coupled-cluster singles and doubles with perturbative triples, for the tests of
``coupled_cluster.RCCSD`` and of ``qs_triples_energy_singles`` / ``kernels.triples_energy_singles``.  Nothing here imports
the package under test.

Two definitions, free of sign and labelling conventions, on the spin-doubled problem (spin orbital 2 P + sigma, the
``2 ns`` lowest occupied in ``|0>``):

  * ``projections``: ``<mu| e^{-T} H e^{T} |0>`` with ``T = T1 + T2`` by matrices on the Fock space of ``m <= 8`` spin
    orbitals (annihilators as 2^m x 2^m matrices, used between the sectors of n, n - 1 and n - 2 particles; ``T`` is
    nilpotent, so both exponentials are finite sums);
  * ``pt_definition``: ``E_(T) = sum_mu Re(conj(A_mu + B_mu) A_mu) / D_mu`` over the triply excited determinants, with
    ``A_mu = <mu| H T2 |0>`` and ``B_mu = <mu| H T1 |0>``, by operators on bit masks (any size).

and the working forms the device code follows:

  * ``dressed``: with ``tau`` (l, l) zero except ``tau[virt, occ] = t1``, ``Xm = 1 - tau`` and ``Ym = 1 + tau``,
    ``h~ = Xm h Ym`` and ``u~ = Xm Xm u Ym Ym`` (bras ``Xm``, kets ``Ym``; ``t1`` is never conjugated), ``f~ = h~ + 2 J~ -
    K~`` of the occupied orbitals.  Then ``_rccd_ref.residual(f~, u~, t2, ns)`` is the doubles projection, with
    ``tt = 2 t2 - t2.transpose(1, 0, 2, 3)``

        R1[a,i] = f~[a,i] + sum_kc f~[k,c] tt[a,c,i,k] + sum_kcd u~[a,k,c,d] tt[c,d,i,k] - sum_klc u~[k,l,i,c] tt[a,c,k,l]

    the singles projection, and ``E = E~_ref + sum (2 u~ - u~^T)[i,j,a,b] t2[a,b,i,j]`` the energy;
  * ``pt_working``: the connected part ``E_[T]`` as ``_triples_ref.working``, and the singles part

        Y_ijk[a,b,c] = 1/2 t1[a,i] <bc|jk>,         V' = the six-fold permuted sum of Y that makes W from X
        E_ST = sum_{i<=j<=k} m_ijk sum_abc Re(conj(V'_abc) Z_abc) / D

``singles_ref`` is the kernel's own singles sum on blocks, factors and two slot tables; ``singles_bound`` its any-order
rounding bound."""

import math

import numpy as np

import _rccd_ref as rc
import _triples_ref as tr

gamma = rc.gamma
_wide = rc._wide


# -- Fock-space matrices: determinant = bit mask over m spin orbitals


def annihilators(m):
    """``a[p]`` (2^m, 2^m) for p < m: ``a_p |det> = (-1)^(occupied below p) |det without p>``."""
    assert m <= 8, "Fock-space matrices are kept to 8 spin orbitals"
    dim = 1 << m
    ops = np.zeros((m, dim, dim))
    for p in range(m):
        for det in range(dim):
            if det >> p & 1:
                ops[p, det ^ (1 << p), det] = (-1) ** bin(det & ((1 << p) - 1)).count("1")
    return ops


def spin_singles(t1):
    """Spin-orbital singles of the closed-shell ``t1`` (v, o): the same amplitude for both spins."""
    return np.kron(t1, np.eye(2))


def projections(h, u, ns, t1, t2):
    """``(E, R1, R2)`` of ``Hbar |0> = e^{-T} H e^{T} |0>``: ``E = <0| Hbar |0>``, ``R1[a,i]`` its projection on
    ``a+_{a alpha} a_{i alpha} |0>`` and ``R2[a,b,i,j]`` on ``a+_{a alpha} a+_{b beta} a_{j beta} a_{i alpha} |0>``.
    ``h`` (l, l) and ``u`` (l, l, l, l, ``<pq|rs>``) in the orbitals, 2 l <= 8."""
    l = h.shape[0]
    hs, us, _ = rc.spin_double(h, u, np.eye(l))
    n, m = 2 * ns, 2 * l
    full = annihilators(m)
    # H and T keep the particle number: all of it happens between the sectors of n, n - 1 and n - 2 particles
    sector = [[det for det in range(1 << m) if bin(det).count("1") == k] for k in (n - 2, n - 1, n)]
    down1 = full[:, sector[1]][:, :, sector[2]]                                # a_p: n -> n - 1
    down2 = full[:, sector[0]][:, :, sector[1]]                                # a_p: n - 1 -> n - 2
    P = np.einsum("sxy,ryz->rsxz", down2, down1)                              # P[r, s] = a_s a_r: n -> n - 2
    Pdag = P.transpose(0, 1, 3, 2)                                            # P[p, q]^T = a+_p a+_q
    ops = down1
    dim = len(sector[2])
    H = np.einsum("pq,pxy,qyz->xz", hs, ops.transpose(0, 2, 1), ops)
    inner = np.tensordot(us, P, axes=([2, 3], [0, 1]))                       # sum_rs us[p,q,r,s] a_s a_r
    H = H + 0.25 * np.einsum("pqxy,pqyz->xz", Pdag, inner)
    T1s, T2s = spin_singles(t1), rc.embed(t2)
    T = np.einsum("ai,axy,iyz->xz", T1s, ops[n:].transpose(0, 2, 1), ops[:n])
    T = T + 0.25 * np.einsum("abij,abxy,ijyz->xz", T2s, Pdag[n:, n:], P[:n, :n])

    def exponential(sign, x):
        out, term = x.copy(), x
        for k in range(1, m + 1):
            term = sign * (T @ term) / k
            out = out + term
        return out

    ref = np.zeros(dim, dtype=H.dtype)
    ref[sector[2].index((1 << n) - 1)] = 1.0
    vacuum = np.zeros(1 << m)
    vacuum[(1 << n) - 1] = 1.0

    def bra(creates, annihilates):
        x = vacuum
        for p in annihilates:
            x = full[p] @ x
        for p in reversed(creates):
            x = full[p].T @ x
        return x[sector[2]]

    hbar = exponential(-1.0, H @ exponential(1.0, ref))
    nv = l - ns
    R1 = np.zeros((nv, ns), dtype=hbar.dtype)
    R2 = np.zeros((nv, nv, ns, ns), dtype=hbar.dtype)
    for a in range(nv):
        A = n + 2 * a
        for i in range(ns):
            R1[a, i] = bra((A,), (2 * i,)) @ hbar
            for b in range(nv):
                B = n + 2 * b + 1
                for j in range(ns):
                    R2[a, b, i, j] = bra((A, B), (2 * i, 2 * j + 1)) @ hbar
    return complex(ref @ hbar), R1, R2


# -- the dressed working form


def dressed(h, u, ns, t1, extended=False):
    """``(h~, u~, f~)`` of the module docstring, in the orbitals ``h`` and ``u`` are given in."""
    if extended:
        h, u, t1 = _wide(h), _wide(u), _wide(t1)
    l = h.shape[0]
    tau = np.zeros((l, l), dtype=np.result_type(h.dtype, u.dtype, t1.dtype))
    tau[ns:, :ns] = t1
    one = np.eye(l, dtype=tau.dtype)
    Xm, Ym = one - tau, one + tau
    hd = Xm @ h @ Ym
    ud = np.einsum("pa,qb,abcd,cr,ds->pqrs", Xm, Xm, u, Ym, Ym, optimize=True)
    fd = hd + 2 * np.einsum("piqi->pq", ud[:, :ns, :, :ns]) - np.einsum("piiq->pq", ud[:, :ns, :ns, :])
    return hd, ud, fd


def reference_energy(h, u, ns):
    """``2 sum_i h_ii + sum_ij (2<ij|ij> - <ij|ji>)`` of the closed-shell determinant (complex: the dressed one is)."""
    o = slice(0, ns)
    return 2 * np.trace(h[o, o]) + 2 * np.einsum("ijij->", u[o, o, o, o]) - np.einsum("ijji->", u[o, o, o, o])


def singles_residual(fd, ud, t2, ns):
    o, v = slice(0, ns), slice(ns, None)
    tt = 2 * t2 - t2.transpose(1, 0, 2, 3)
    return (fd[v, o] + np.einsum("kc,acik->ai", fd[o, v], tt) + np.einsum("akcd,cdik->ai", ud[v, o, v, v], tt)
            - np.einsum("klic,ackl->ai", ud[o, o, o, v], tt))


def residuals(h, u, ns, t1, t2, extended=False):
    """``(R1, R2)`` of the working form."""
    _, ud, fd = dressed(h, u, ns, t1, extended)
    if extended:
        t2 = _wide(t2)
    return singles_residual(fd, ud, t2, ns), rc.residual(fd, ud, t2, ns)


def total_energy(h, u, ns, t1, t2):
    """``E~_ref + sum (2 u~ - u~^T)[i,j,a,b] t2[a,b,i,j]``: the whole ``<0| Hbar |0>`` (complex until converged)."""
    hd, ud, _ = dressed(h, u, ns, t1)
    g = ud[:ns, :ns, ns:, ns:]
    return reference_energy(hd, ud, ns) + np.einsum("ijab,abij->", 2 * g - g.transpose(0, 1, 3, 2), t2)


def conventional_energy(h, u, ns, t1, t2):
    """``E_ref + 2 sum f_ia t1 + sum L_ijab (t2 + t1 t1)`` on the undressed tensors."""
    o, v = slice(0, ns), slice(ns, None)
    f = h + 2 * np.einsum("piqi->pq", u[:, o, :, o]) - np.einsum("piiq->pq", u[:, o, o, :])
    g = u[o, o, v, v]
    L = 2 * g - g.transpose(0, 1, 3, 2)
    return (reference_energy(h, u, ns) + 2 * np.einsum("ia,ai->", f[o, v], t1)
            + np.einsum("ijab,abij->", L, t2 + np.einsum("ai,bj->abij", t1, t1)))


def correlation_energy(h, u, ns, t1, t2):
    return float(np.real(total_energy(h, u, ns, t1, t2) - reference_energy(h, u, ns)))


def orbital_basis(h, u, C):
    """``h`` and ``u`` in the orbitals ``C``."""
    return (np.einsum("pa,pq,qb->ab", C.conj(), h, C),
            np.einsum("pa,qb,pqrs,rc,sd->abcd", C.conj(), C.conj(), u, C, C, optimize=True))


def solve(h, u, ns, tol=1e-11, max_iter=1000):
    """Iterate ``t1 += R1 / (e_i - e_a)``, ``t2 += R2 / D`` from ``f_ai / (e_i - e_a)`` and the first-order doubles until
    the 2-norm of ``(R1, R2)`` is below ``tol``; ``h`` and ``u`` in the orbitals.  Returns ``(E_corr, t1, t2, iterations)``."""
    f, _ = rc.orbital_tensors(h, u, np.eye(h.shape[0]), ns)
    D2 = rc.denominators(f, ns)
    e = np.real(np.diagonal(f))
    D1 = e[None, :ns] - e[ns:, None]
    t1, t2 = f[ns:, :ns] / D1, u[ns:, ns:, :ns, :ns] / D2
    for it in range(max_iter):
        R1, R2 = residuals(h, u, ns, t1, t2)
        if math.hypot(np.linalg.norm(R1.ravel()), np.linalg.norm(R2.ravel())) < tol:
            return correlation_energy(h, u, ns, t1, t2), t1, t2, it
        t1 = t1 + R1 / D1
        t2 = t2 + R2 / D2
        t2 = 0.5 * (t2 + t2.transpose(1, 0, 3, 2))
    raise AssertionError(f"the reference did not converge in {max_iter} iterations")


def two_electron_ground_state(h, u):
    """The lowest eigenvalue of ``h(1) + h(2) + u(1, 2)`` on all l^2 products of two spatial orbitals (opposite spins:
    the symmetric combinations are the singlets, the anti-symmetric ones the M = 0 triplets)."""
    l = h.shape[0]
    one = np.eye(l)
    H = (np.einsum("pr,qs->pqrs", h, one) + np.einsum("pr,qs->pqrs", one, h) + u).reshape(l * l, l * l)
    assert np.abs(H - H.conj().T).max() <= 1e-12 * np.abs(H).max()
    return float(np.linalg.eigvalsh(0.5 * (H + H.conj().T))[0])


# -- (T) with singles: the determinant definition


def pt_definition(h, u, eps, ns, t1, t2):
    """``(E_[T], E_ST)`` by the determinant sum: ``sum |A|^2 / D`` and ``sum Re(conj(B) A) / D``.  ``h`` and ``u`` in
    the canonical orbitals, ``eps`` their energies."""
    l = h.shape[0]
    hs, us, _ = rc.spin_double(h, u, np.eye(l))
    n, m = 2 * ns, 2 * l
    es = np.repeat(np.asarray(eps, dtype=np.float64), 2)
    ref = (1 << n) - 1
    T1s, T2s = spin_singles(t1), rc.embed(t2)
    doubles, singles = {}, {}
    for I in range(n):
        for A in range(n, m):
            s, det = tr._excite(ref, (A,), (I,))
            if s and T1s[A - n, I] != 0:
                singles[det] = singles.get(det, 0) + s * T1s[A - n, I]
            for J in range(I + 1, n):
                for B in range(A + 1, m):
                    s, det = tr._excite(ref, (A, B), (I, J))
                    if s and T2s[A - n, B - n, I, J] != 0:
                        doubles[det] = doubles.get(det, 0) + s * T2s[A - n, B - n, I, J]

    def hamiltonian_on(state):
        out = {}
        for det, coeff in state.items():
            occ = [p for p in range(m) if det >> p & 1]
            for x, r in enumerate(occ):
                for p in range(m):
                    s, new = tr._excite(det, (p,), (r,))
                    if s:
                        out[new] = out.get(new, 0) + s * hs[p, r] * coeff
                for s_ in occ[x + 1:]:
                    for p in range(m):
                        for q in range(p + 1, m):
                            s, new = tr._excite(det, (p, q), (r, s_))
                            if s:
                                out[new] = out.get(new, 0) + s * us[p, q, r, s_] * coeff
        return out

    Amu, Bmu = hamiltonian_on(doubles), hamiltonian_on(singles)
    connected = with_singles = 0.0
    for det, amp in Amu.items():
        holes = [p for p in range(n) if not det >> p & 1]
        if len(holes) != 3:
            continue
        parts = [p for p in range(n, m) if det >> p & 1]
        D = es[holes].sum() - es[parts].sum()
        connected += abs(amp) ** 2 / D
        with_singles += float(np.real(np.conj(Bmu.get(det, 0)) * amp)) / D
    return float(connected), float(with_singles)


# -- (T) with singles: the working form


def singles_blocks(u, ns, t1, extended=False):
    """``Y[i,j,k,a,b,c] = 1/2 t1[a,i] <bc|jk>`` (o, o, o, v, v, v)."""
    if extended:
        u, t1 = _wide(u), _wide(t1)
    return 0.5 * np.einsum("ai,bcjk->ijkabc", t1, u[ns:, ns:, :ns, :ns])


def pt_working(u, eps, ns, t1, t2, extended=False):
    """``(E_[T], E_ST)`` of the working form; ``u`` in the canonical orbitals."""
    W, Z = tr._combine(tr.blocks(u, ns, t2, extended))
    V, _ = tr._combine(singles_blocks(u, ns, t1, extended))
    e_ = np.asarray(eps, dtype=np.longdouble if extended else np.float64)
    eo, ev = e_[:ns], e_[ns:]
    D = (eo[:, None, None, None, None, None] + eo[None, :, None, None, None, None] + eo[None, None, :, None, None, None]
         - ev[None, None, None, :, None, None] - ev[None, None, None, None, :, None] - ev[None, None, None, None, None, :])
    e = ((W.conj() * Z).real / D).sum(axis=(3, 4, 5))
    es = ((V.conj() * Z).real / D).sum(axis=(3, 4, 5))
    return tr.restricted_sum(e), tr.restricted_sum(es)


def singles_factors(u, ns, t1):
    """``(A, G)`` of ``RCCSD.triples``: ``A = 1/2 t1^T`` (o, v) and ``G[q o + r] = <bc|qr>`` (o^2, v, v)."""
    nv = u.shape[0] - ns
    A = np.ascontiguousarray(0.5 * t1.T)
    G = np.ascontiguousarray(u[ns:, ns:, :ns, :ns].transpose(2, 3, 0, 1)).reshape(ns * ns, nv, nv)
    return A, G


def singles_slot_row(ns, i, j, k):
    """``(sa, sg)`` of the six blocks of the triple (i, j, k): block ``X_pqr`` has ``(p, q o + r)``."""
    return [(p, q * ns + r) for p, q, r in ((i, j, k), (i, k, j), (j, i, k), (j, k, i), (k, i, j), (k, j, i))]


# -- the kernel's own singles sum: A (na, v), G (ng, v, v), sslots (n, 6, 2) beside the blocks and slots of _triples_ref


def _triple_V(A, G, srow, absolute=False, extended=False):
    V = 0
    for beta, order in enumerate(tr.ORDERS):
        a, g = A[srow[beta][0]], G[srow[beta][1]]
        if absolute:
            a, g = np.abs(a), np.abs(g)
        elif extended:
            a, g = _wide(a), _wide(g)
        V = V + np.einsum(f"{order[0]},{order[1:]}->abc", a, g)
    return V


def singles_terms(X, row, A, G, srow, eo3, ev, extended=False):
    """``Re(conj(V') Z) / D`` (v, v, v) of ONE triple."""
    W = tr._triple_W(X, row, extended=extended)
    V = _triple_V(A, G, srow, extended=extended)
    return (V.conj() * tr._symmetric(W, "")).real / tr._denominator(eo3, ev, extended)


def singles_ref(X, slots, A, G, sslots, eo3, ev, extended=False):
    """``es`` (n,) of the kernel's definition."""
    return np.array([singles_terms(X, row, A, G, sslots[x], eo3[x], ev, extended).sum()
                     for x, row in enumerate(np.asarray(slots))])


def singles_bound_terms(X, row, A, G, srow, eo3, ev, terms):
    """Any-order bound on one element of ``singles_terms`` whose sum has ``terms`` terms:
    ``gamma(terms + 25) V^ Z^ / |D|`` with ``V^ = sum |A| |G|`` in the place of ``W^`` as the conjugated factor and ``Z^``
    as in ``_triples_ref.kernel_bound_terms``.  The count: every step that ``kernel_bound_terms`` charges its 24 for is
    taken here too, one for one (five additions make ``V'`` as five make ``W``; the combination to ``Z``, the product
    with it, the division, the weight and the sums are the same), and each term of ``V'`` is first a product ``A G``:
    one more rounding on that factor, so 25.  The relative error of ``D`` is ``gamma(6) (|eo3| + |ev_a| + |ev_b| +
    |ev_c|) / |D|`` as there; a further ``2 sqrt 2`` for complex products, which covers the product ``A G`` as well."""
    V = _triple_V(A, G, srow, absolute=True)
    W = tr._triple_W(X, row, absolute=True)

    def at(order):
        return np.einsum(f"{order}->abc", W)

    Z = (4 * W + at("bca") + at("cab") + 2 * at("acb") + 2 * at("cba") + 2 * at("bac")) / 3
    D = np.abs(tr._denominator(eo3, ev))
    a = np.abs(np.asarray(ev, dtype=np.float64))
    mag = abs(float(eo3)) + a[:, None, None] + a[None, :, None] + a[None, None, :]
    base = V * Z / D
    bound = gamma(terms + 25) * base + gamma(6) * mag / D * base
    return bound * (2.0 * np.sqrt(2.0) if np.iscomplexobj(X) else 1.0)


def singles_bound(X, slots, A, G, sslots, eo3, ev):
    """``singles_bound_terms`` summed over the v^3 elements of every triple: (n,)."""
    v = len(ev)
    return np.array([singles_bound_terms(X, row, A, G, sslots[x], eo3[x], ev, v ** 3).sum()
                     for x, row in enumerate(np.asarray(slots))])


def _cyclic(entries):
    """The even orders (0, 3, 4) hold one thing and the odd ones (1, 2, 5) one thing."""
    return entries[0] == entries[3] == entries[4] and entries[1] == entries[2] == entries[5]


def singles_tile_set_sensitivity(X, slots, A, G, sslots, eo3, ev, T):
    """The least ``|singles contribution of a tile set| / singles_bound`` over the triples of the tables and their tile
    sets, from the long-double reference alone (the analogue of ``_triples_ref.tile_set_sensitivity``): a workgroup whose
    singles partial is left out, doubled or put elsewhere moves ``es`` by that many bounds at least.  A tile set holds
    whole orbits of (a, b, c), D is the same on an orbit, and the sum of Z over an orbit is 0 (its coefficients add up
    to 0), so an orbit adds nothing where Z = 0 on it or where V' is the same at its six orders.  What is 0 by such an
    identity is left out, and nothing else:
      * a set that holds a = b = c alone -- the diagonal set of a ragged tile of one element: Z = 0;
      * every set of a triple with ONE block in all six ``slots``: W is totally symmetric, Z = 0;
      * ``slots`` cyclic (orders 0, 3, 4 one block, orders 1, 2, 5 one block): W is totally symmetric wherever two
        indices are equal, Z = 0 there: the diagonal set of a ragged tile of TWO elements holds such orbits alone;
      * every set of a triple whose six ``(sa, sg)`` are all equal: V' is totally symmetric;
      * ``sslots`` cyclic in the same sense (the pairs ``(sa, sg)`` compared): V' is totally symmetric wherever two
        indices are equal, again the diagonal set of a ragged tile of two.
    (Not left out, because no table of the tests has it and the condition then fails on the safe side: a cyclic ``sslots``
    row beside a ``slots`` row under which W is the same at two orders a transposition apart, as the table of i = j is;
    the even and the odd sums of W are then equal and every orbit adds 0.)"""
    v = len(ev)
    ragged = v % T
    bound = singles_bound(X, slots, A, G, sslots, eo3, ev)
    least = np.inf
    for x, row in enumerate(np.asarray(slots)):
        pairs = [tuple(int(y) for y in entry) for entry in np.asarray(sslots[x])]
        if len(set(row.tolist())) == 1 or len(set(pairs)) == 1:
            continue
        terms = singles_terms(X, row, A, G, sslots[x], eo3[x], ev, extended=True)
        sums = np.abs(tr.tile_set_sums(terms, T)).astype(np.float64)
        if ragged == 1 or (ragged == 2 and (_cyclic(row.tolist()) or _cyclic(pairs))):
            sums = sums[:-1]                # (nt - 1, nt - 1, nt - 1), the last set
        if sums.size:
            least = min(least, sums.min() / bound[x])
    return least


def singles_problem(v, n, na, ng, seed, complex_=False, share="none"):
    """Seeded ``A`` (na, v), ``G`` (ng, v, v) and ``sslots`` (n, 6, 2).  ``share``: "none" = six distinct (sa, sg)
    entries per triple, both columns distinct; "repeat" = entries that repeat inside a triple."""
    rng = np.random.default_rng(seed)

    def draw(*shape):
        x = rng.standard_normal(shape)
        return x + 1j * rng.standard_normal(shape) if complex_ else x

    A, G = draw(na, v), draw(ng, v, v)
    sslots = np.empty((n, 6, 2), dtype=np.int32)
    for x in range(n):
        if share == "repeat":
            a, g = rng.choice(na, 2, replace=False), rng.choice(ng, 3, replace=False)
            sslots[x, :, 0] = [a[0], a[0], a[1], a[1], a[0], a[1]]
            sslots[x, :, 1] = [g[0], g[1], g[0], g[2], g[2], g[1]]
        else:
            sslots[x, :, 0] = rng.choice(na, 6, replace=False)
            sslots[x, :, 1] = rng.choice(ng, 6, replace=False)
    return A, G, sslots
