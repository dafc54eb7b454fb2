"""NumPy restatement of the closed-shell perturbative triples correction on doubles amplitudes, for the tests of
``coupled_cluster.RCCD.triples`` and of ``qs_triples_energy`` / ``kernels.triples_energy``.  Nothing here imports the
package under test.

The quantity, free of sign and labelling conventions: in canonical orbitals (Fock matrix ``diag(eps)``), with ``T2`` the
doubles operator of the amplitudes,

    E_T = sum_mu |<mu| H T2 |0>|^2 / D_mu,      D_mu = sum eps(holes of mu) - sum eps(particles of mu)

over the triply excited determinants ``mu`` of the spin-doubled system (``definition``: creation and annihilation
operators on bit masks).  The closed-shell working form (``working``) with ``t[a,b,i,j] = t[b,a,j,i]`` and ``<pq|rs>``
not anti-symmetrised:

    X_ijk[a,b,c] = sum_d t[a,d,i,j] <bc|dk>  -  sum_l t[a,b,i,l] <lc|jk>
    W_ijk[a,b,c] = X_ijk[a,b,c] + X_ikj[a,c,b] + X_jik[b,a,c] + X_jki[b,c,a] + X_kij[c,a,b] + X_kji[c,b,a]
    Z[a,b,c]     = (4 W_abc + W_bca + W_cab - 2 W_acb - 2 W_cba - 2 W_bac) / 3
    e_ijk        = sum_abc Re(conj(W_abc) Z_abc) / (eps_i + eps_j + eps_k - eps_a - eps_b - eps_c)
    E_T          = sum_{i<=j<=k} m_ijk e_ijk,     m = 6 (all different), 3 (two equal), 0 (i = j = k)

``kernel_ref`` is the kernel's own sum on blocks and a slot table, ``kernel_bound`` its any-order rounding bound."""

import numpy as np

import _rccd_ref as rc

gamma = rc.gamma
_wide = rc._wide

# block beta of a triple enters W[a,b,c] at this order of (a, b, c): X_0[abc] + X_1[acb] + X_2[bac] + X_3[bca] + X_4[cab] + X_5[cba]
ORDERS = ("abc", "acb", "bac", "bca", "cab", "cba")


# -- the definition: determinants as bit masks over 2 l spin orbitals (spin orbital 2 P + sigma)


def _annihilate(det, p):
    if not det >> p & 1:
        return 0, 0
    return (-1) ** bin(det & ((1 << p) - 1)).count("1"), det ^ (1 << p)


def _create(det, p):
    if det >> p & 1:
        return 0, 0
    return (-1) ** bin(det & ((1 << p) - 1)).count("1"), det | (1 << p)


def _excite(det, creates, annihilates):
    """``a+_{c0} a+_{c1} ... a_{x1} a_{x0} |det>`` for ``annihilates = (x0, x1, ...)``: (sign, determinant), sign 0 = nothing."""
    sign = 1
    for p in annihilates:
        s, det = _annihilate(det, p)
        if not s:
            return 0, 0
        sign *= s
    for p in reversed(creates):
        s, det = _create(det, p)
        if not s:
            return 0, 0
        sign *= s
    return sign, det


def definition(h, u, eps, ns, t):
    """``E_T`` by the determinant sum.  ``h`` (l, l) and ``u`` (l, l, l, l, ``<pq|rs>``) in the canonical orbitals, ``eps``
    their energies, ``ns`` doubly occupied, ``t`` (v, v, o, o).  ``H`` is the whole Hamiltonian, its one-body part
    included: the bare two-body operator alone has a mean-field part that reaches the triples."""
    l = h.shape[0]
    hs, us, _ = rc.spin_double(h, u, np.eye(l))
    T = rc.embed(t)
    n, m = 2 * ns, 2 * l
    es = np.repeat(np.asarray(eps, dtype=np.float64), 2)
    ref = (1 << n) - 1
    # T2 |0> = sum_{A<B, I<J} T[A,B,I,J] a+_A a+_B a_J a_I |0>
    state = {}
    for I in range(n):
        for J in range(I + 1, n):
            for A in range(n, m):
                for B in range(A + 1, m):
                    s, det = _excite(ref, (A, B), (I, J))
                    if s and T[A - n, B - n, I, J] != 0:
                        state[det] = state.get(det, 0) + s * T[A - n, B - n, I, J]
    # H on it: sum_pr h[p,r] a+_p a_r  +  sum_{p<q, r<s} us[p,q,r,s] a+_p a+_q a_s a_r   (us anti-symmetrised)
    out = {}
    for det, coeff in state.items():
        occ = [p for p in range(m) if det >> p & 1]
        for x, r in enumerate(occ):
            for p in range(m):
                s, new = _excite(det, (p,), (r,))
                if s:
                    out[new] = out.get(new, 0) + s * hs[p, r] * coeff
            for s_ in occ[x + 1:]:
                for p in range(m):
                    for q in range(p + 1, m):
                        s, new = _excite(det, (p, q), (r, s_))
                        if s:
                            out[new] = out.get(new, 0) + s * us[p, q, r, s_] * coeff
    total = 0.0
    for det, amp in out.items():
        holes = [p for p in range(n) if not det >> p & 1]
        if len(holes) != 3:
            continue
        parts = [p for p in range(n, m) if det >> p & 1]
        total += abs(amp) ** 2 / (es[holes].sum() - es[parts].sum())
    return float(total)


# -- the working form


def blocks(u, ns, t, extended=False):
    """``X[i,j,k,a,b,c]`` (o, o, o, v, v, v) of the working form."""
    if extended:
        u, t = _wide(u), _wide(t)
    o, v = slice(0, ns), slice(ns, None)
    return np.einsum("adij,bcdk->ijkabc", t, u[v, v, v, o]) - np.einsum("abil,lcjk->ijkabc", t, u[o, v, o, o])


def _combine(X):
    """``(W, Z)`` (o, o, o, v, v, v) of the blocks ``X``."""
    W = (X + np.einsum("ikjacb->ijkabc", X) + np.einsum("jikbac->ijkabc", X) + np.einsum("jkibca->ijkabc", X)
         + np.einsum("kijcab->ijkabc", X) + np.einsum("kjicba->ijkabc", X))
    return W, _symmetric(W, "ijk")


def _symmetric(W, lead):
    def at(order):
        return np.einsum(f"{lead}{order}->{lead}abc", W)

    return (4 * W + at("bca") + at("cab") - 2 * at("acb") - 2 * at("cba") - 2 * at("bac")) / 3


def working(u, eps, ns, t, extended=False):
    """``(e, E_T)``: the per-triple ``e[i,j,k]`` (o, o, o) of the working form and the sum over i <= j <= k with the
    weights m.  ``u`` in the canonical orbitals."""
    X = blocks(u, ns, t, extended)
    W, Z = _combine(X)
    e_ = np.asarray(eps, dtype=np.longdouble if extended else np.float64)
    eo, ev = e_[:ns], e_[ns:]
    D = (eo[:, None, None, None, None, None] + eo[None, :, None, None, None, None] + eo[None, None, :, None, None, None]
         - ev[None, None, None, :, None, None] - ev[None, None, None, None, :, None] - ev[None, None, None, None, None, :])
    e = ((W.conj() * Z).real / D).sum(axis=(3, 4, 5))
    return e, restricted_sum(e)


def weight(i, j, k):
    return 0 if i == j == k else 3 if (i == j or j == k or i == k) else 6


def triples(ns):
    """The triples i <= j <= k of the restricted sum, (i, i, i) left out (weight 0)."""
    return [(i, j, k) for i in range(ns) for j in range(i, ns) for k in range(j, ns) if not i == j == k]


def restricted_sum(e):
    ns = e.shape[0]
    return sum(weight(i, j, k) * e[i, j, k] for i in range(ns) for j in range(i, ns) for k in range(j, ns))


# -- the kernel's own sum: blocks (nblocks, v, v, v), slots (n, 6), eo3 (n,), ev (v,)


def _triple_W(X, row, absolute=False, extended=False, drop=None):
    W = 0
    for beta, order in enumerate(ORDERS):
        if beta == drop:
            continue
        blk = X[row[beta]]
        if absolute:
            blk = np.abs(blk)
        elif extended:
            blk = _wide(blk)
        W = W + np.einsum(f"{order}->abc", blk)
    return W


def _denominator(eo3, ev, extended=False):
    ev = np.asarray(ev, dtype=np.longdouble if extended else np.float64)
    eo3 = np.longdouble(eo3) if extended else np.float64(eo3)
    return eo3 - ev[:, None, None] - ev[None, :, None] - ev[None, None, :]


def kernel_terms(X, row, eo3, ev, extended=False, drop=None):
    """``Re(conj(W) Z) / D`` (v, v, v) of ONE triple with the slot row ``row`` (``drop``: block beta left out of W)."""
    W = _triple_W(X, row, extended=extended, drop=drop)
    return (W.conj() * _symmetric(W, "")).real / _denominator(eo3, ev, extended)


def kernel_ref(X, slots, eo3, ev, extended=False, drop=None):
    """``e`` (n,) of the kernel's definition."""
    return np.array([kernel_terms(X, row, eo3[x], ev, extended, drop).sum() for x, row in enumerate(np.asarray(slots))])


def kernel_bound_terms(X, row, eo3, ev, terms):
    """Any-order bound on one element of ``kernel_terms`` whose sum has ``terms`` terms: ``gamma(terms + 24) W^ Z^ / |D|``
    with ``W^ = sum |X_pi|`` and ``Z^`` the combination of ``Z`` with absolute coefficients (the five additions, the
    combination, the product and the division), plus the relative error of ``D``, ``gamma(6) (|eo3| + |ev_a| + |ev_b| +
    |ev_c|) / |D|`` of it; a further ``2 sqrt 2`` for complex products."""
    W = _triple_W(X, row, absolute=True)

    def at(order):
        return np.einsum(f"{order}->abc", W)

    Z = (4 * W + at("bca") + at("cab") + 2 * at("acb") + 2 * at("cba") + 2 * at("bac")) / 3
    D = np.abs(_denominator(eo3, ev))
    a = np.abs(np.asarray(ev, dtype=np.float64))
    mag = abs(float(eo3)) + a[:, None, None] + a[None, :, None] + a[None, None, :]
    base = W * Z / D
    bound = gamma(terms + 24) * base + gamma(6) * mag / D * base
    return bound * (2.0 * np.sqrt(2.0) if np.iscomplexobj(X) else 1.0)


def kernel_bound(X, slots, eo3, ev):
    """``kernel_bound_terms`` summed over the v^3 elements of every triple: (n,)."""
    v = len(ev)
    return np.array([kernel_bound_terms(X, row, eo3[x], ev, v ** 3).sum() for x, row in enumerate(np.asarray(slots))])


# -- the kernel's work units: what one (triple, tile set) adds, every coincidence of six slots


def tile_set_sums(terms, T):
    """What every unordered set of three tiles of edge ``T`` adds to the sum of ``terms`` (v, v, v), in the kernel's order
    of sets (tc slowest, then tb, then ta <= tb <= tc): an element belongs to the set of its sorted tile indices, so a set
    holds whole orbits of (a, b, c).  Length nt (nt + 1) (nt + 2) / 6."""
    v = terms.shape[0]
    nt = -(-v // T)
    tile = np.arange(v) // T
    ta, tb, tc = np.sort(np.stack(np.meshgrid(tile, tile, tile, indexing="ij")), axis=0)
    index = tc * (tc + 1) * (tc + 2) // 6 + tb * (tb + 1) // 2 + ta
    sums = np.zeros(nt * (nt + 1) * (nt + 2) // 6, dtype=terms.dtype)
    np.add.at(sums, index.ravel(), terms.ravel())
    return sums


def tile_set_sensitivity(X, slots, eo3, ev, T):
    """The least ``|contribution of a tile set| / kernel_bound`` over the triples of the table and their tile sets, from
    the long-double reference alone: a workgroup left out or corrupted moves ``e`` by that many bounds at least.  What is
    0 by identity is left out, and nothing else:
      * a set that holds a = b = c alone -- the diagonal set of a ragged tile of one element: the six W are equal, Z = 0;
      * every set of a triple with ONE block in all six slots: W is totally symmetric, Z = 0, e = 0 (``e_iii``);
      * where the even orders (slots 0, 3, 4) hold one block and the odd ones (1, 2, 5) one block, W is the same at the
        three cyclic orders of (a, b, c), so it is totally symmetric wherever two of the indices are equal: the diagonal
        set of a ragged tile of TWO elements holds such orbits alone."""
    v = len(ev)
    ragged = v % T
    bound = kernel_bound(X, slots, eo3, ev)
    least = np.inf
    for x, row in enumerate(np.asarray(slots)):
        if len(set(row.tolist())) == 1:
            continue
        cyclic = row[0] == row[3] == row[4] and row[1] == row[2] == row[5]
        sums = np.abs(tile_set_sums(kernel_terms(X, row, eo3[x], ev, extended=True), T)).astype(np.float64)
        if ragged == 1 or (ragged == 2 and cyclic):
            sums = sums[:-1]                # (nt - 1, nt - 1, nt - 1), the last set
        if sums.size:
            least = min(least, sums.min() / bound[x])
    return least


def _set_partitions(m):
    """The partitions of m things as restricted growth strings: thing x in class s[x], classes numbered as they appear."""
    if m == 0:
        return [[]]
    return [s + [c] for s in _set_partitions(m - 1) for c in range(max(s, default=-1) + 2)]


def coincidence(row):
    """Which slots of a row hold the same block: the row with its blocks renumbered as they appear."""
    seen = {}
    return tuple(seen.setdefault(int(b), len(seen)) for b in row)


def slot_partitions(nblocks, seed=0):
    """(203, 6) int32: one slot row for every way in which the six slots of a triple can coincide (the set partitions of
    six things).  The classes of a row go to distinct blocks of ``nblocks >= 6`` drawn by ``seed``, so which class has the
    lowest block, and which appears first, varies from row to row."""
    rng = np.random.default_rng(seed)
    rows = []
    for s in _set_partitions(6):
        blocks = rng.choice(nblocks, max(s) + 1, replace=False)
        rows.append(blocks[s])
    return np.array(rows, dtype=np.int32)


def block_index(ns, p, q, r):
    """Where ``X_pqr`` sits among the o^3 blocks: the last occupied index slowest."""
    return (r * ns + q) * ns + p


def slot_row(ns, i, j, k):
    """The six blocks of the triple (i, j, k): X_ijk, X_ikj, X_jik, X_jki, X_kij, X_kji."""
    return [block_index(ns, *pqr) for pqr in ((i, j, k), (i, k, j), (j, i, k), (j, k, i), (k, i, j), (k, j, i))]


def packed_blocks(Xfull):
    """``blocks`` (o, o, o, v, v, v) as the (o^3, v, v, v) array that ``block_index`` addresses."""
    ns, nv = Xfull.shape[0], Xfull.shape[3]
    return np.ascontiguousarray(Xfull.transpose(2, 1, 0, 3, 4, 5)).reshape(ns ** 3, nv, nv, nv)


# -- seeded inputs


def canonical_problem(ls, ns, seed, complex_=False, scale=0.03):
    """``(h, u, eps)`` on ``ls`` spatial orbitals that ARE the canonical ones of ``ns`` doubly occupied: a Hermitian ``u``
    with particle-exchange symmetry, levels ``eps`` two apart, and ``h = diag(eps) - (2 J - K)`` of the occupied
    orbitals, so that the Fock matrix is ``diag(eps)`` exactly and ``C = 1``."""
    _, u, _ = rc.closed_shell_problem(ls, seed, complex_=complex_, scale=scale)
    rng = np.random.default_rng(seed + 1000)
    eps = 2.0 * np.arange(ls) + 0.3 * rng.random(ls)
    J = np.einsum("piqi->pq", u[:, :ns, :, :ns])
    K = np.einsum("piiq->pq", u[:, :ns, :ns, :])
    h = np.diag(eps).astype(u.dtype) - (2 * J - K)
    return h, u, eps


def kernel_problem(v, n, nblocks, seed, complex_=False, share="none"):
    """Seeded blocks, slot table, ``eo3`` and ``ev`` for the kernel alone.  ``share``: "none" = six distinct blocks per
    triple, "pair" = the table of a triple with i = j (X_ijk = X_jik, X_ikj = X_jki, X_kij = X_kji), "all" = one block
    six times."""
    rng = np.random.default_rng(seed)
    X = rng.standard_normal((nblocks, v, v, v))
    if complex_:
        X = X + 1j * rng.standard_normal((nblocks, v, v, v))
    slots = np.empty((n, 6), dtype=np.int32)
    for x in range(n):
        if share == "all":
            slots[x] = rng.integers(nblocks)
        elif share == "pair":
            a, b, c = rng.choice(nblocks, 3, replace=False)
            slots[x] = [a, b, a, b, c, c]
        else:
            slots[x] = rng.choice(nblocks, 6, replace=False)
    ev = 1.0 + 0.5 * np.arange(v) + 0.2 * rng.random(v)
    eo3 = -3.0 - rng.random(n)
    return X, slots, eo3, ev
