"""``kernels.string_ci_density2`` / ``string_ci_spin_squared`` and ``StringCI``'s observables on them, on the GPU.

Tolerances (derived, not tuned; tests/_string_ci_density_ref.py states them):
  * Gamma, elementwise: gamma_(dim+T+3) ( sum_K |E_rp bra| |E_qs ket| + delta_qr sum_K |bra| |E_ps ket| ), 2 sqrt 2 for
    complex128 -- the dot-product bound, valid for any order of accumulation, with T the partial sums of the schedule
    (``qs_string_ci_density2_plan``); rho, the last row of the same product: gamma_(dim+T+3) sum_K |bra| |E_pq ket|;
  * rho against ``string_ci_density1``: test_gpu_string_ci.py's density bound gamma_(dim+2) (unit vectors);
  * Hermiticity, exchange symmetry and the trace of Gamma: m^2 times the largest element bound (the trace is a sum of
    m^2 elements, the other two compare two);
  * S^2 c, elementwise: gamma_(m^2+2) ( |s0| |c[I]| + sum_pq |c[J_pq(I)]| ), 2 sqrt 2 for complex128.
Where the launch geometry can go wrong the reference is the project's own ``det_ci_density2`` on ``determinant_order``,
spin-summed over four of its elements, each within that test's own bound gamma_(dim+2) |bra| |ket| (``pair_bound``).
Every comparison prints its worst ratio to the bound before it asserts."""

import ctypes
import functools

import numpy as np
import pytest
import torch

import _det_ci_density_ref as ddref
import _det_ci_ref as dref
import _string_ci_density_ref as sref
import _string_ci_ref as ref

pytestmark = pytest.mark.gpu
FORMS = {"f64": False, "c128": True}
S2 = 2.0 * np.sqrt(2.0)


def H(x):
    return torch.as_tensor(x).cpu().numpy()


def dev(x):
    return torch.from_numpy(np.array(x)).cuda()


def vectors(K, na, nb, cplx, seed):
    rng = np.random.default_rng(seed)
    c = rng.standard_normal((K, na, nb))
    return c + 1j * rng.standard_normal((K, na, nb)) if cplx else c


def unit_pair(na, nb, cplx, seed):
    c = vectors(2, na, nb, cplx, seed)
    return c[0] / np.linalg.norm(c[0]), c[1] / np.linalg.norm(c[1])


def tables(sa, sb, m, Na, Nb):
    from quantum_systems_amd import kernels

    ta = kernels.string_ci_table(dev(sa), m, Na)
    return ta, (ta if sa is sb else kernels.string_ci_table(dev(sb), m, Nb))


def ratio_of(err, bound, what):
    bound = np.asarray(bound, dtype=np.float64)
    r = float((np.asarray(err, dtype=np.float64) / np.where(bound > 0, bound, 1.0)).max())
    print(f"{what}: worst error / bound = {r:.3f}")
    return r


def plan(m, na, nb, cplx, budget=None):
    """(rows, passes, T, kc, bytes) of the schedule ``string_ci_density2`` runs under the calling thread's tuning."""
    from quantum_systems_amd import _lib, kernels

    out = (ctypes.c_int64 * 5)()
    budget = kernels.STRING_CI_BYTES if budget is None else budget
    assert _lib.load().qs_string_ci_density2_plan(1 if cplx else 0, m, na, nb, budget, ctypes.cast(out, ctypes.c_void_p)) == 0
    return tuple(out)


@functools.lru_cache(maxsize=None)
def one_spin(m, N):
    """(strings, E of the list, its table) of one spin; computed once, never modified."""
    s = ref.strings(m, N)
    E = ref.list_E(s, m)
    T = ref.table_from_E(E)
    for a in (s, E, T):
        a.setflags(write=False)
    return s, E, T


@functools.lru_cache(maxsize=None)
def dense(m, Na, Nb):
    E, S = ref.dense_E(m, Na, Nb), sref.dense_spin_squared(m, Na, Nb)
    E.setflags(write=False)
    S.setflags(write=False)
    return E, S


@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("m,Na,Nb", ref.SHAPES)
def test_gamma_and_rho_against_the_dense_oracle(m, Na, Nb, form):
    from quantum_systems_amd import kernels

    cc = FORMS[form]
    E, _ = dense(m, Na, Nb)
    sa, sb = ref.strings(m, Na), ref.strings(m, Nb)
    na, nb, N = len(sa), len(sb), Na + Nb
    ta, tb = tables(sa, sb, m, Na, Nb)
    T = plan(m, na, nb, cc)[2]
    bra, ket = unit_pair(na, nb, cc, 5 + m)
    for b, k, what in ((bra, bra, "state"), (bra, ket, "pair")):
        tag = f"({m},{Na},{Nb}) {form} {what}"
        db = dev(b)
        G, rho = kernels.string_ci_density2(ta, tb, m, db, db if k is b else dev(k))
        assert G.shape == (m, m, m, m) and rho.shape == (m, m) and G.dtype == rho.dtype == (torch.complex128 if cc else torch.float64)
        G, rho = H(G), H(rho)
        Gx, rhox = sref.dense_gamma(E, b, k)
        bound = sref.gamma_bound(E, b, k, T)
        assert ratio_of(np.abs(G - Gx), bound, tag + " Gamma") <= 1.0
        assert ratio_of(np.abs(rho - rhox), sref.rho_sum_bound(E, b, k, T), tag + " rho") <= 1.0
        rho1 = H(kernels.string_ci_density1(ta, tb, m, dev(b), dev(k)))
        assert ratio_of(np.abs(rho - rho1), np.float64(ref.gamma(na * nb + 2) * (S2 if cc else 1.0)), tag + " rho against density1") <= 1.0
        wide = m * m * float(bound.max())
        assert ratio_of(np.abs(G - G.transpose(1, 0, 3, 2)), np.float64(wide), tag + " exchange symmetry") <= 1.0
        trace = np.einsum("pqpq->", G)
        want = N * (N - 1) * np.vdot(b, k)
        assert ratio_of(abs(trace - want), np.float64(wide), tag + " trace") <= 1.0
        if k is b:
            assert ratio_of(np.abs(G - G.transpose(2, 3, 0, 1).conj()), np.float64(wide), tag + " Hermiticity") <= 1.0


def det_gamma(sa, sb, m, bra, ket):
    """The project's det_ci_density2 on the interleaved determinants, spin-summed: (Gamma (m, m, m, m), N)."""
    from quantum_systems_amd import kernels
    from quantum_systems_amd.string_ci import determinant_order

    masks, perm, phase = determinant_order(sa, sb)
    N = dref.popcount(int(masks[0]))
    ph, pm = dev(phase).to(bra.dtype), dev(perm)
    vb = (bra.reshape(-1) * ph)[pm].contiguous()
    vk = vb if ket is bra else (ket.reshape(-1) * ph)[pm].contiguous()
    G = kernels.det_ci_density2(dev(masks), vb, vk, 2 * m, N)
    return sum(G[a::2, b::2, a::2, b::2] for a in (0, 1) for b in (0, 1)), N


# (11, 4, 4): 330 x 330, the 256-thread workgroup, two tiles along Ib, the second one with 74 live lanes of 256;
# m = 7, 9, 11: m^2 off the 16-column chunk, odd (fp64 lines of the ket panel on 8-byte boundaries)
GEOMETRY = [(7, 3, 3), (9, 5, 0), (9, 0, 5), (6, 6, 3), (11, 4, 4)]


@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("m,Na,Nb", GEOMETRY)
def test_launch_and_schedule_geometries_against_det_ci_density2(m, Na, Nb, form):
    from quantum_systems_amd import kernels

    cc = FORMS[form]
    (sa, Ea, _), (sb, Eb, _) = one_spin(m, Na), one_spin(m, Nb)
    na, nb = len(sa), len(sb)
    ta, tb = tables(sa, sb, m, Na, Nb)
    T = plan(m, na, nb, cc)[2]
    bra, ket = unit_pair(na, nb, cc, m + Na)
    db, dk = dev(bra), dev(ket)
    G, rho = kernels.string_ci_density2(ta, tb, m, db, dk)
    want, N = det_gamma(sa, sb, m, db, dk)
    # four elements of det_ci_density2, each within its test's own bound, and their sum
    bound = sref.gamma_bound((Ea, Eb), bra, ket, T) + 4 * ddref.pair_bound(bra.reshape(-1), ket.reshape(-1)) * (1 + 4 * ref.EPS)
    tag = f"({m},{Na},{Nb}) {form} {na} x {nb}, T = {T}"
    assert ratio_of(H((G - want).abs()), bound, tag) <= 1.0
    assert float(G.abs().max()) > 1e3 * float(bound.max())                        # the comparison sees the result
    G2, rho2 = kernels.string_ci_density2(ta, tb, m, db, dk)
    assert torch.equal(G, G2) and torch.equal(rho, rho2)                          # a repeated call: identical bits


@pytest.mark.parametrize("form", list(FORMS))
def test_passes_under_three_byte_budgets(form):
    """(9, 4, 4), 126 x 126: one pass, several equal passes, and a ragged last pass whose slices end in zeros."""
    from quantum_systems_amd import kernels

    cc = FORMS[form]
    m, Na, Nb = 9, 4, 4
    (sa, Ea, _), (sb, Eb, _) = one_spin(m, Na), one_spin(m, Nb)
    na, nb, N = len(sa), len(sb), Na + Nb
    ta, tb = tables(sa, sa, m, Na, Nb)
    es = 16 if cc else 8
    budgets = {}
    for r in range(na, 0, -1):
        budget = (2 * m * m + 1) * (r * nb + 64) * es
        rows, passes, T, kc, _ = plan(m, na, nb, cc, budget)
        if passes == 1:
            kind = "one"
        elif na % rows == 0:
            kind = "equal" if passes >= 3 else None
        else:
            kind = "ragged"                                                      # the last pass ends inside the slices
            assert (na - (passes - 1) * rows) * nb < T * kc
        if kind:
            budgets.setdefault(kind, (budget, rows, passes, T, kc))
    assert set(budgets) >= {"one", "equal", "ragged"}, budgets
    bra, ket = unit_pair(na, nb, cc, 94)
    db, dk = dev(bra), dev(ket)
    Tmax = max(b[3] for b in budgets.values())
    bound, rbound = sref.gamma_bound((Ea, Eb), bra, ket, Tmax), sref.rho_sum_bound((Ea, Eb), bra, ket, Tmax)
    got = {}
    for kind, (budget, rows, passes, T, kc) in budgets.items():
        kernels.dispatch_log = log = []
        try:
            with kernels.tuning(string_ci_bytes=budget):
                assert plan(m, na, nb, cc)[:4] == (rows, passes, T, kc)
                G, rho = kernels.string_ci_density2(ta, tb, m, db, dk)
        finally:
            kernels.dispatch_log = None
        print(f"{form} {kind}: {passes} passes of {rows} rows, T = {T}, kc = {kc}, last pass {(na - (passes - 1) * rows) * nb} of {T * kc}")
        entry = [e for e in log if "string_ci" in e]
        assert len(entry) == 1 and len(log) == 1, log                             # one entry names the whole call
        w = 2 if cc else 1
        for name in (f"string_ci_expand_panel_kernel<{w}, false, 1>", f"string_ci_expand_panel_kernel<{w}, true, 1>", "gemm",
                     f"string_ci_gamma_close_kernel<{w}>"):
            assert name in entry[0], (name, entry[0])
        assert "det_ci" not in entry[0] and "string_ci_expand_kernel" not in entry[0]
        G, rho = H(G), H(rho)
        got[kind] = G
        # oracle-free: sum_q Gamma[p,q,r,q] = (N - 1) rho[r,p]
        err = np.abs(np.einsum("pqrq->pr", G) - (N - 1) * rho.T)
        assert ratio_of(err, np.einsum("pqrq->pr", bound) + (N - 1) * rbound.T, f"{form} {kind}: partial trace") <= 1.0
    for kind in ("equal", "ragged"):
        assert ratio_of(np.abs(got[kind] - got["one"]), 2 * bound, f"{form} {kind} against one pass") <= 1.0
    assert float(np.abs(got["one"]).max()) > 1e3 * float(bound.max())


@pytest.mark.parametrize("form", list(FORMS))
def test_a_truncated_alpha_list_against_the_cut_intermediate(form):
    """The random half of the alpha list of (6, 3, 3): E_qs ket is cut to the list before E_pr acts, as in sigma, so
    sum k_pr <E_pr> + sum W X rebuilt from the returned Gamma and rho is <c| string_ci_sigma(c)>."""
    from quantum_systems_amd import kernels

    cc = FORMS[form]
    m, Na, Nb = 6, 3, 3
    ht, ut = ref.random_hamiltonian(m, 633, cc)
    k, W = ref.kh_operands(ht, ut)
    rng = np.random.default_rng(633)
    full = ref.strings(m, Na)
    sa, sb = np.sort(rng.choice(full, len(full) // 2, replace=False)), ref.strings(m, Nb)
    na, nb = len(sa), len(sb)
    ta, tb = tables(sa, sb, m, Na, Nb)
    Ea, Eb = ref.list_E(sa, m), ref.list_E(sb, m)
    assert np.array_equal(H(ta), ref.table_from_E(Ea)) and (H(ta) == 0).sum() > (ref.table_from_E(ref.list_E(full, m)) == 0).sum() // 2 + 1
    T = plan(m, na, nb, cc)[2]
    bra, ket = unit_pair(na, nb, cc, 6)
    for b, kt, what in ((bra, bra, "state"), (bra, ket, "pair")):
        G, rho = kernels.string_ci_density2(ta, tb, m, dev(b), dev(kt))
        G, rho = H(G), H(rho)
        Gx, rhox = sref.dense_gamma((Ea, Eb), b, kt)
        bound, rbound = sref.gamma_bound((Ea, Eb), b, kt, T), sref.rho_sum_bound((Ea, Eb), b, kt, T)
        assert ratio_of(np.abs(G - Gx), bound, f"half of the alpha list, {form} {what}: Gamma") <= 1.0
        assert ratio_of(np.abs(rho - rhox), rbound, f"half of the alpha list, {form} {what}: rho") <= 1.0
        # X[(pr),(qs)] = Gamma[p,q,r,s] + delta_qr <E_ps>, <E_ps> = rho[s,p]
        X, Xb = G.astype(np.clongdouble), bound.copy()
        for q in range(m):
            X[:, q, q, :] += rho.T
            Xb[:, q, q, :] += rbound.T
        Wt = W.reshape(m, m, m, m).transpose(0, 2, 1, 3)                           # W[(pr),(qs)] at [p,q,r,s]
        rebuilt = np.sum(ref._wide(k) * rho.T) + np.sum(ref._wide(Wt) * X)
        rebuilt_bound = float(np.sum(np.abs(k) * rbound.T) + np.sum(np.abs(Wt) * Xb))
        sigma = H(kernels.string_ci_sigma(dev(k), dev(W), ta, tb, dev(kt[None])))[0]
        sbound = ref.kh_sigma(np.abs(k), np.abs(W), np.abs(Ea), np.abs(Eb), np.abs(kt[None])).astype(np.float64)[0]
        sbound = ref.gamma(3 * m * m + 4) * sbound * (S2 if cc else 1.0)
        want = np.sum(ref._wide(b).conj() * ref._wide(sigma))
        assert ratio_of(abs(rebuilt - want), np.float64(rebuilt_bound + float(np.sum(np.abs(b) * sbound))),
                        f"half of the alpha list, {form} {what}: energy rebuilt from Gamma and rho") <= 1.0


@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("m,Na,Nb", ref.SHAPES)
def test_spin_squared_against_the_dense_oracle(m, Na, Nb, form):
    from quantum_systems_amd import kernels

    cc = FORMS[form]
    _, S = dense(m, Na, Nb)
    (sa, Ea, _), (sb, Eb, _) = one_spin(m, Na), one_spin(m, Nb)
    na, nb = len(sa), len(sb)
    ta, tb = tables(sa, sb, m, Na, Nb)
    for K in (1, 3, 9):
        c = vectors(K, na, nb, cc, 11 * K + m)
        got = H(kernels.string_ci_spin_squared(ta, tb, m, Na, Nb, dev(c)))
        assert got.shape == c.shape and got.dtype == (np.complex128 if cc else np.float64)
        exact = (ref._wide(c).reshape(K, -1) @ ref._wide(S).T).reshape(c.shape)
        bound = sref.spin_bound(Ea, Eb, Na, Nb, c)
        assert ratio_of(np.abs(got - exact), bound, f"S^2 ({m},{Na},{Nb}) {form} K={K}") <= 1.0
    one = H(kernels.string_ci_spin_squared(ta, tb, m, Na, Nb, dev(c[0])))           # a 2-D c is one vector
    assert one.shape == (na, nb) and np.array_equal(one, got[0])                    # a vector's chain does not know K


@pytest.mark.parametrize("form", list(FORMS))
def test_spin_squared_of_known_states(form):
    from quantum_systems_amd import kernels

    cc = FORMS[form]
    # all spins up: every vector is an eigenvector with S = 5/2, S (S + 1) = 8.75
    m, Na, Nb = 9, 5, 0
    (sa, Ea, _), (sb, Eb, _) = one_spin(m, Na), one_spin(m, Nb)
    ta, tb = tables(sa, sb, m, Na, Nb)
    c = vectors(3, len(sa), 1, cc, 950)
    got = H(kernels.string_ci_spin_squared(ta, tb, m, Na, Nb, dev(c)))
    assert ratio_of(np.abs(got - 8.75 * c), sref.spin_bound(Ea, Eb, Na, Nb, c), f"(9,5,0) {form}: S (S + 1) = 8.75") <= 1.0
    # the closed-shell determinant (Ia, Ib) = (0, 0) of (8, 4, 4): exactly 0
    m, Na, Nb = 8, 4, 4
    sa = ref.strings(m, Na)
    ta, _ = tables(sa, sa, m, Na, Nb)
    c = np.zeros((len(sa), len(sa)), dtype=np.complex128 if cc else np.float64)
    c[0, 0] = 1.0
    assert int(sa[0]) == 0b1111
    got = H(kernels.string_ci_spin_squared(ta, ta, m, Na, Nb, dev(c)))
    assert np.array_equal(got, np.zeros_like(c))


@pytest.mark.parametrize("form", list(FORMS))
def test_spin_squared_commutes_with_sigma_on_complete_lists(form):
    """(11, 4, 4), 330 x 330, two beta tiles: S^2 (H c) against H (S^2 c).  With A_H = 2 m^2 (max|k| + 2 m^2 max|W|) and
    A_S = |s0| + m^2 the largest row sums of |H| and |S^2| in this formulation, e_H(x) = gamma_(3 m^2 + 4) A_H max|x| and
    e_S(x) = gamma_(m^2 + 2) A_S max|x| the kernels' crude bounds, the two sides differ by at most
    A_S e_H(c) + e_S(H c) + A_H e_S(c) + e_H(S^2 c), times 2 sqrt 2 for complex128."""
    from quantum_systems_amd import kernels

    cc = FORMS[form]
    m, Na, Nb = 11, 4, 4
    ht, ut = ref.random_hamiltonian(m, 1144, cc)
    k, W = ref.kh_operands(ht, ut)
    sa = ref.strings(m, Na)
    ta, _ = tables(sa, sa, m, Na, Nb)
    c = dev(vectors(2, len(sa), len(sa), cc, 1144))
    dk, dW = dev(k), dev(W)
    Hc = kernels.string_ci_sigma(dk, dW, ta, ta, c)
    Sc = kernels.string_ci_spin_squared(ta, ta, m, Na, Nb, c)
    left = kernels.string_ci_spin_squared(ta, ta, m, Na, Nb, Hc)
    right = kernels.string_ci_sigma(dk, dW, ta, ta, Sc)
    AH = 2 * m * m * (float(np.abs(k).max()) + 2 * m * m * float(np.abs(W).max()))
    AS = abs(sref.spin_s0(Na, Nb)) + m * m
    eH = lambda x: ref.gamma(3 * m * m + 4) * AH * float(x.abs().max())
    eS = lambda x: ref.gamma(m * m + 2) * AS * float(x.abs().max())
    bound = (AS * eH(c) + eS(Hc) + AH * eS(c) + eH(Sc)) * (S2 if cc else 1.0)
    assert ratio_of(H((left - right).abs()), np.float64(bound), f"[S^2, H] on (11,4,4) {form}") <= 1.0
    assert float(left.abs().max()) > 1e3 * bound                                   # the comparison sees the result


# ---- solver level ------------------------------------------------------------------------------------------------------


def random_spatial_system(l, n, seed, cplx):
    """The system of test_gpu_string_ci.py's solver test: a seeded RandomBasisSet made physical, 2 n electrons."""
    import quantum_systems_amd as qsa

    np.random.seed(seed)
    bs = qsa.RandomBasisSet(l, 2)
    part = (lambda x: x) if cplx else (lambda x: np.ascontiguousarray(x.real))
    bs.h = part(bs.h)
    s = part(bs.s)
    bs.s = np.eye(l) + 0.1 * (s - np.diag(np.diag(s)))
    u = 0.3 * part(bs.u)
    u = u + u.conj().transpose(2, 3, 0, 1)
    bs.u = u + u.transpose(1, 0, 3, 2)
    system = qsa.SpatialOrbitalSystem(2 * n, bs)
    host = (np.array(bs.h), np.array(bs.s), np.array(bs.u), float(bs.nuclear_repulsion_energy))
    system.change_module(qsa.hip)
    return system, host


@pytest.mark.parametrize("form", list(FORMS))
def test_solver_spin_and_energy_from_densities(form):
    from quantum_systems_amd import StringCI, hip

    cplx = FORMS[form]
    l, n = 4, 2
    system, (h, s, u, e_nuc) = random_spatial_system(l, n, 4242, cplx)
    X = dref.loewdin(s)
    ci = StringCI(system, hip.asarray(X))
    with pytest.raises(RuntimeError, match="solve"):
        ci.two_body_density(0)
    with pytest.raises(RuntimeError, match="solve"):
        ci.energy_from_densities(0)
    with pytest.raises(RuntimeError, match="solve"):
        ci.spin_squared(0)
    with pytest.raises(ValueError):
        ci.apply_spin_squared(torch.zeros(ci.na + 1, ci.nb, dtype=torch.float64, device="cuda"))
    with pytest.raises(ValueError):
        ci.apply_spin_squared(torch.zeros(ci.na * ci.nb, dtype=torch.float64, device="cuda"))
    E, c = ci.solve(4, tol=1e-9)
    assert ci.converged
    E, c = H(E), H(c)
    m, na, nb, N = ci.m, ci.na, ci.nb, 2 * n
    (sa, Ea, _) = one_spin(m, n)
    ht = X.conj().T @ h @ X
    ut = np.einsum("pa,qb,pqrs,rc,sd->abcd", X.conj(), X.conj(), u, X, X, optimize=True)
    k, W = ref.kh_operands(ht, ut)
    T = plan(m, na, nb, cplx)[2]
    for r in range(4):
        # The residual of a Davidson root is below tol = 1e-9; the error of an expectation value of an operator that
        # commutes with H is of second order in it, ~1e-18 / gap, and a factor of 10^3 is left for near-degenerate
        # roots: 1e-6.  The Davidson tolerance is the source of this number, not the kernels.
        s2 = ci.spin_squared(r)
        S = round((np.sqrt(1.0 + 4.0 * max(s2, 0.0)) - 1.0) / 2.0)
        print(f"{form} root {r}: E = {E[r]:.10f}, <S^2> = {s2:.3e}, nearest S = {S}, multiplicity {ci.spin_multiplicity(r):.6f}")
        assert isinstance(s2, float) and S in (0, 1, 2) and abs(s2 - S * (S + 1)) <= 1e-6
        assert abs(ci.spin_multiplicity(r) - np.sqrt(1.0 + 4.0 * s2)) <= 1e-12
        # energy functional against the Rayleigh quotient of the same vector
        e = ci.energy_from_densities(r)
        sigma = H(ci.sigma(ci._c[r]))
        cr = c[r]
        rq = float(np.sum(ref._wide(cr).conj() * ref._wide(sigma)).real) + e_nuc
        gb, rb = sref.gamma_bound((Ea, Ea), cr, cr, T), sref.rho_sum_bound((Ea, Ea), cr, cr, T)
        sb = ref.kh_sigma(np.abs(k), np.abs(W), np.abs(Ea), np.abs(Ea), np.abs(cr[None])).astype(np.float64)[0]
        sb = ref.gamma(3 * m * m + 4) * sb * (S2 if cplx else 1.0)
        # on top: the rounding of the two contractions with ht and ut themselves (m^4 + m^2 terms) and of k = ht - 1/2 sum ut,
        # which sigma uses and the functional does not
        moduli = float(np.sum(np.abs(ht) * np.abs(H(ci.one_body_density(r)).T)) + 0.5 * np.sum(np.abs(ut) * np.abs(H(ci.two_body_density(r)))))
        bound = float(np.sum(np.abs(ht) * rb.T) + 0.5 * np.sum(np.abs(ut) * gb) + np.sum(np.abs(cr) * sb)) + \
            ref.gamma(m * m * m * m + m * m + 4 * l + 2) * moduli * (S2 if cplx else 1.0) + 4 * ref.EPS * abs(e_nuc)
        assert ratio_of(abs(e - rq), np.float64(bound), f"{form} root {r}: energy_from_densities against the Rayleigh quotient") <= 1.0
        assert abs(e - E[r]) <= 1e-8 * max(1.0, abs(E[r]))
    G01 = H(ci.two_body_density(0, 1))
    gb = sref.gamma_bound((Ea, Ea), c[0], c[1], T)
    # <c_0|c_1> = 0 to the solver's orthogonality, ~1e-14: the trace is N (N - 1) <c_0|c_1>
    ortho = N * (N - 1) * abs(np.vdot(c[0], c[1]))
    assert ratio_of(abs(np.einsum("pqpq->", G01)), np.float64(np.einsum("pqpq->", gb) + ortho), f"{form}: trace of the transition Gamma") <= 1.0
    assert np.array_equal(H(ci.two_body_density(1, 1)), H(ci.two_body_density(1)))
    assert H(ci.apply_spin_squared(ci._c)).shape == (4, na, nb)
