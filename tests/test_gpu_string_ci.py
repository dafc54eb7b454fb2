"""``kernels.string_ci_*`` and ``string_ci.StringCI`` on the GPU.

Small shapes go against the dense oracle of tests/_string_ci_ref.py (Jordan-Wigner matrices on the spin orbitals, the
phase between the creator orders counted inversion by inversion).  Tolerances (derived, not tuned):
  * table: exact;
  * diagonal: a sum of m + 2 m^2 terms, gamma_(m + 2 m^2) times the sum of their moduli;
  * sigma: the PATH bound gamma_n sum_pr |E_pr| (|k_pr| |c| + sum_qs |W_pr,qs| |E_qs| |c|), n = 3 m^2 + 4 (m^2 products
    and their sum, the k term, up to 2 m^2 folded terms with their fmas), 2 sqrt 2 for complex products; the exact value
    is the oracle's H c in ``numpy.longdouble``.  |H| |c| would be too small: the delta_qr term cancels inside H but
    not in the arithmetic;
  * density: gamma_(dim+2) ||bra|| ||ket|| (2 sqrt 2 complex); trace = Na + Nb within m of those, Hermiticity within 2.
Where the launch geometry can go wrong the reference is the project's own ``det_ci_sigma`` on ``to_determinants``
(pinned by its own tests to two oracles), with the crude but valid bound
gamma_n 2 m^2 (max|k| + m^2 max|ut|) max|c| plus det_ci's gamma_(t+2) t (N max|h| + N^2 max|ut_as|) max|c|, t its term
count.  A TRUNCATED list is not the projection of H in this formulation (the intermediate E_qs c is cut too), so the
random half of an alpha list goes against the host Knowles-Handy sum on the ladder oracle's E of the list, path bound.
Every comparison prints its worst ratio to the bound before it asserts."""

import functools

import numpy as np
import pytest
import torch

import _det_ci_ref as dref
import _string_ci_ref as ref

pytestmark = pytest.mark.gpu
FORMS = {"f64": (False, False), "real_h_complex_c": (False, True), "c128": (True, True)}
S2 = 2.0 * np.sqrt(2.0)


def H(x):
    return torch.as_tensor(x).cpu().numpy()


def dev(x):
    return torch.from_numpy(np.array(x)).cuda()


def vectors(K, na, nb, cplx, seed):
    rng = np.random.default_rng(seed)
    c = rng.standard_normal((K, na, nb))
    return c + 1j * rng.standard_normal((K, na, nb)) if cplx else c


@functools.lru_cache(maxsize=None)
def problem(m, Na, Nb, hc):
    """Seeded (ht, ut, k, W, E, H longdouble) on the dense sector; computed once, never modified."""
    ht, ut = ref.random_hamiltonian(m, 100 + 10 * m + 3 * Na + Nb, hc)
    k, W = ref.kh_operands(ht, ut)
    out = ht, ut, k, W, ref.dense_E(m, Na, Nb), ref.dense_hamiltonian(ht, ut, Na, Nb, extended=True)
    for a in out:
        a.setflags(write=False)
    return out


def tables(sa, sb, m, Na, Nb):
    from quantum_systems_amd import kernels

    ta = kernels.string_ci_table(dev(sa), m, Na)
    return ta, (ta if sa is sb else kernels.string_ci_table(dev(sb), m, Nb))


def ratio_of(err, bound, what):
    r = float((np.asarray(err, dtype=np.float64) / np.where(bound > 0, bound, 1.0)).max())
    print(f"{what}: worst error / bound = {r:.3f}")
    return r


@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("m,Na,Nb", ref.SHAPES)
def test_table_diagonal_sigma_and_density_against_the_dense_oracle(m, Na, Nb, form):
    from quantum_systems_amd import kernels

    hc, cc = FORMS[form]
    ht, ut, k, W, E, Hx = problem(m, Na, Nb, hc)
    sa, sb = ref.strings(m, Na), ref.strings(m, Nb)
    na, nb = len(sa), len(sb)
    ta, tb = tables(sa, sb, m, Na, Nb)
    for t, s, N in ((ta, sa, Na), (tb, sb, Nb)):
        assert t.dtype == torch.int32 and np.array_equal(H(t), ref.table_from_E(ref.list_E(s, m))), "table"
    # the one-spin E of the ladder oracle is the dense sector's (tests/test_string_ci_ref_host.py): the table is E's

    D = H(kernels.string_ci_diagonal(dev(ht), dev(ut), dev(sa), Na, dev(sb), Nb))
    Dx, S = ref.diagonal_terms(ht, ut, Na, Nb)
    bound = ref.gamma(m + 2 * m * m) * S
    assert ratio_of(np.abs(D - Dx), bound, f"diagonal ({m},{Na},{Nb}) {form}") <= 1.0
    assert np.abs(Dx.reshape(-1) - np.diag(Hx).real).max() <= 1e-12 * max(1.0, float(np.abs(Hx).max()))

    for K in (1, 3, 9):
        c = vectors(K, na, nb, cc, 7 * K + m)
        got = H(kernels.string_ci_sigma(dev(k), dev(W), ta, tb, dev(c)))
        assert got.shape == c.shape and got.dtype == (np.complex128 if cc else np.float64)
        flat = c.reshape(K, na * nb)
        exact = flat.astype(np.clongdouble if cc else np.longdouble) @ Hx.T
        bound = ref.path_bound(k, W, E, flat)
        assert ratio_of(np.abs(got.reshape(K, -1) - exact), bound, f"sigma ({m},{Na},{Nb}) {form} K={K}") <= 1.0
    # a 2-D c is one vector: the first of the last batch, alone (another product, so within twice the bound)
    one = H(kernels.string_ci_sigma(dev(k), dev(W), ta, tb, dev(c[0])))
    assert one.shape == (na, nb)
    assert ratio_of(np.abs(one - got[0]), 2 * bound[0].reshape(na, nb), f"sigma ({m},{Na},{Nb}) {form} 2-D c") <= 1.0

    c = vectors(2, na, nb, cc, 5)
    bra, ket = c[0] / np.linalg.norm(c[0]), c[1] / np.linalg.norm(c[1])
    Ew = E.astype(np.clongdouble if cc else np.longdouble)
    for b, kt in ((bra, bra), (bra, ket)):
        rho = H(kernels.string_ci_density1(ta, tb, m, dev(b), dev(kt)))
        want = np.einsum("i,pqij,j->qp", b.reshape(-1).conj(), Ew, kt.reshape(-1))
        bound = ref.gamma(na * nb + 2) * (S2 if cc else 1.0)                     # ||bra|| = ||ket|| = 1
        assert ratio_of(np.abs(rho - want), bound, f"density ({m},{Na},{Nb}) {form}") <= 1.0
    rho = H(kernels.string_ci_density1(ta, tb, m, dev(bra), dev(bra)))
    assert abs(np.trace(rho) - (Na + Nb)) <= m * bound and np.abs(rho - rho.conj().T).max() <= 2 * bound


def spin_doubled(ht, ut):
    """(h2, u2 anti-symmetrised) on the device, spin orbital 2 p + sigma."""
    from quantum_systems_amd import kernels

    return kernels.add_spin_one_body(ht), kernels.spin_expand_two_body(ut, antisymmetrize=True)


def det_sigma(ht, ut, sa, sb, c):
    """The project's det_ci_sigma on the interleaved determinants, brought back to (Ia, Ib) order."""
    from quantum_systems_amd import kernels
    from quantum_systems_amd.string_ci import determinant_order

    masks, perm, phase = determinant_order(sa, sb)
    N = dref.popcount(int(masks[0]))
    h2, u2 = spin_doubled(ht, ut)
    dets = dev(masks)
    ph, pm = dev(phase).to(c.dtype), dev(perm)
    v = (c.reshape(c.shape[0], -1) * ph)[:, pm].contiguous()
    diag = kernels.det_ci_diagonal(h2, u2, dets, N)
    s = kernels.det_ci_sigma(h2, u2, dets, N, diag, v)
    back = torch.empty_like(s)
    back[:, pm] = s
    return (back * ph).reshape(c.shape), N


def crude_bound(m, N, k, W, ht, ut, cmax, cplx):
    n = 3 * m * m + 4
    kh = ref.gamma(n) * 2 * m * m * (float(np.abs(k).max()) + m * m * 2.0 * float(np.abs(W).max())) * cmax
    t = dref.terms(2 * m, N)
    uas = 2.0 * float(np.abs(ut).max())
    det = ref.gamma(t + 2) * t * (N * float(np.abs(ht).max()) + N * N * uas) * cmax
    return (kh + det) * (S2 if cplx else 1.0)


# (11, 4, 4): 330 x 330, the 256-thread workgroup, two tiles along Ib, the second one with 74 live lanes of 256
GEOMETRY = [(7, 3, 3), (8, 4, 3), (9, 4, 4), (9, 5, 0), (9, 0, 5), (6, 6, 3), (11, 4, 4)]


@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("m,Na,Nb", GEOMETRY)
def test_launch_geometries_against_det_ci_sigma(m, Na, Nb, form):
    from quantum_systems_amd import kernels

    hc, cc = FORMS[form]
    ht, ut = ref.random_hamiltonian(m, 900 + 10 * m + Na, hc)
    k, W = ref.kh_operands(ht, ut)
    sa, sb = ref.strings(m, Na), ref.strings(m, Nb)
    ta, tb = tables(sa, sb, m, Na, Nb)
    c = dev(vectors(3, len(sa), len(sb), cc, m + Na))
    got = kernels.string_ci_sigma(dev(k), dev(W), ta, tb, c)
    want, N = det_sigma(dev(ht), dev(ut), sa, sb, c)
    bound = crude_bound(m, N, k, W, ht, ut, float(c.abs().max()), cc)
    assert ratio_of(H((got - want).abs()), np.float64(bound), f"({m},{Na},{Nb}) {form} {len(sa)} x {len(sb)}") <= 1.0
    assert float(want.abs().max()) > 1e3 * bound                                  # the comparison sees the result
    again = kernels.string_ci_sigma(dev(k), dev(W), ta, tb, c)
    assert torch.equal(got, again)                                                # a repeated call: identical bits


def test_orbitals_up_to_62_embedded_in_m_63():
    """(8, 4, 4) at spatial orbitals {0, 15, 31, 32, 33, 47, 61, 62} of m = 63 (m^4 = 15 752 961 elements of W fit):
    lists of 70 strings each, every other entry of k and W random and non-zero, generated on the device; the result is
    the plain (8, 4, 4) one, whose only difference is the length of the product's sum (m^2 = 3969 terms, zeros but for
    64): both bounds are added."""
    from quantum_systems_amd import kernels

    orb = np.array([0, 15, 31, 32, 33, 47, 61, 62])
    m, M = 8, 63
    ht, ut = ref.random_hamiltonian(m, 63, False)
    k, W = ref.kh_operands(ht, ut)
    small = ref.strings(m, 4)
    big = np.array([sum(1 << int(orb[p]) for p in range(m) if (int(x) >> p) & 1) for x in small], dtype=np.int64)
    assert (np.diff(big) > 0).all() and int(big.max()) >> 62 == 1
    gen = torch.Generator(device="cuda").manual_seed(63)
    kb = torch.randn(M, M, generator=gen, device="cuda", dtype=torch.float64) + 2.0
    Wb = 0.3 * torch.randn(M * M, M * M, generator=gen, device="cuda", dtype=torch.float64) + 1.0
    o = dev(orb)
    kb[o[:, None], o[None, :]] = dev(k)
    pr = (o[:, None] * M + o[None, :]).reshape(-1)
    Wb[pr[:, None], pr[None, :]] = dev(W)
    ts = kernels.string_ci_table(dev(small), m, 4)
    tb = kernels.string_ci_table(dev(big), M, 4)
    # the big table is the small one at the embedded columns and 0 elsewhere
    assert torch.equal(tb[:, pr], ts) and int((tb != 0).sum()) == int((ts != 0).sum())
    c = dev(vectors(2, 70, 70, False, 63))
    plain = kernels.string_ci_sigma(dev(k), dev(W), ts, ts, c)
    got = kernels.string_ci_sigma(kb, Wb, tb, tb, c)
    cmax = float(c.abs().max())
    bound = sum(ref.gamma(3 * mm * mm + 4) * 2 * m * m * (float(np.abs(k).max()) + m * m * 2 * float(np.abs(W).max())) * cmax
                for mm in (m, M))
    assert ratio_of(H((got - plain).abs()), np.float64(bound), "m = 63 embedding of (8,4,4)") <= 1.0


@pytest.mark.parametrize("form", ["f64", "c128"])
def test_a_truncated_alpha_list_drops_missing_targets(form):
    from quantum_systems_amd import kernels

    hc, cc = FORMS[form]
    m, Na, Nb = 8, 4, 3
    ht, ut = ref.random_hamiltonian(m, 843, hc)
    k, W = ref.kh_operands(ht, ut)
    rng = np.random.default_rng(843)
    full = ref.strings(m, Na)
    sa, sb = np.sort(rng.choice(full, len(full) // 2, replace=False)), ref.strings(m, Nb)
    ta, tb = tables(sa, sb, m, Na, Nb)
    Ea, Eb = ref.list_E(sa, m), ref.list_E(sb, m)
    assert np.array_equal(H(ta), ref.table_from_E(Ea)) and np.array_equal(H(tb), ref.table_from_E(Eb))
    assert (H(ta) == 0).sum() > (ref.table_from_E(ref.list_E(full, m)) == 0).sum() // 2 + 1       # targets are missing
    c = vectors(3, len(sa), len(sb), cc, 9)
    got = H(kernels.string_ci_sigma(dev(k), dev(W), ta, tb, dev(c)))
    exact = ref.kh_sigma(k, W, Ea, Eb, c)
    bound = ref.kh_sigma(np.abs(k), np.abs(W), np.abs(Ea), np.abs(Eb), np.abs(c)).astype(np.float64)
    bound = ref.gamma(3 * m * m + 4) * bound * (S2 if cc else 1.0)
    assert ratio_of(np.abs(got - exact), bound, f"half of the alpha list, {form}") <= 1.0


def test_groups_under_a_small_byte_budget():
    from quantum_systems_amd import _lib, kernels

    m, Na, Nb, K = 8, 4, 3, 9
    ht, ut = ref.random_hamiltonian(m, 77, False)
    k, W = ref.kh_operands(ht, ut)
    sa, sb = ref.strings(m, Na), ref.strings(m, Nb)
    ta, tb = tables(sa, sb, m, Na, Nb)
    c = dev(vectors(K, len(sa), len(sb), False, 3))
    one = _lib.load().qs_string_ci_workspace(0, 0, m, len(sa), len(sb), 1)
    bound = 2 * crude_bound(m, Na + Nb, k, W, ht, ut, float(c.abs().max()), False)
    results = {}
    for group in (1, 4, 9):
        kernels.dispatch_log = log = []
        try:
            with kernels.tuning(string_ci_bytes=group * one):
                results[group] = kernels.string_ci_sigma(dev(k), dev(W), ta, tb, c)
        finally:
            kernels.dispatch_log = None
        entry = [e for e in log if "string_ci" in e]
        assert len(entry) == 1, log                                              # one entry names the whole call
        calls = entry[0].split(" | ")
        assert len(calls) == -(-K // group)
        for call in calls:
            # one pass of the rectangular layout: one expand, the product, one fold
            assert call.count("string_ci_expand_kernel<1, qs::ScRect>") == call.count("string_ci_expand_kernel") == 1
            assert call.count("string_ci_fold_kernel<0, qs::ScRect>") == call.count("string_ci_fold_kernel") == 1
            assert "ScTri" not in call and "symmetrize" not in call and "det_ci" not in call
            assert call.index("expand") < call.index("gemm") < call.index("fold")
    for group in (1, 4):
        assert ratio_of(H((results[group] - results[9]).abs()), np.float64(bound), f"groups of {group} against 9") <= 1.0


# ---- solver and API ----------------------------------------------------------------------------------------------------


def random_spatial_system(l, n, seed, cplx):
    """A seeded RandomBasisSet made physical (s positive definite near 1, u with the symmetries of <pq|rs>) with 2 n
    electrons: ``system.n`` = n doubly occupied orbitals."""
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
    assert system.n == n
    host = (np.array(bs.h), np.array(bs.s), np.array(bs.u), float(bs.nuclear_repulsion_energy))
    system.change_module(qsa.hip)
    return system, host


@pytest.mark.parametrize("form", ["f64", "c128"])
def test_solver_densities_and_observables(form):
    import quantum_systems_amd as qsa
    from quantum_systems_amd import DeterminantCI, HartreeFock, StringCI, hip, kernels, sz_sector

    cplx = FORMS[form][0]
    l, n = 4, 2
    system, (h, s, u, e_nuc) = random_spatial_system(l, n, 4242, cplx)
    X = dref.loewdin(s)
    u_before = H(system.u).copy()
    kernels.dispatch_log = log = []
    try:
        ci = StringCI(system, hip.asarray(X))
        built = len(log)
        E, c = ci.solve(3, tol=1e-9)
    finally:
        kernels.dispatch_log = None
    assert (ci.m, ci.na, ci.nb, ci.dim) == (l, 6, 6, 36) and ci._ta is ci._tb
    ht = X.conj().T @ h @ X
    ut = np.einsum("pa,qb,pqrs,rc,sd->abcd", X.conj(), X.conj(), u, X, X, optimize=True)
    lam = np.linalg.eigvalsh(ref.dense_hamiltonian(ht, ut, n, n))
    bound = 1e-8 * max(1.0, np.abs(lam).max())
    E, c = H(E), H(c)
    print(f"{form}: max |dE| = {np.abs(E - e_nuc - lam[:3]).max():.2e} (bound {bound:.1e}), {ci.iterations} iterations")
    assert ci.converged and c.shape == (3, 6, 6) and np.abs(E - e_nuc - lam[:3]).max() <= bound
    # one Davidson step = one sigma call: expand, product, fold per group; no table, no det_ci kernel, W built once
    steps = log[built:]
    assert len(steps) == ci.iterations == len(ci.sigma_history)
    for entry in steps:
        assert "string_ci_expand" in entry and "string_ci_fold" in entry
        assert "table" not in entry and "det_ci" not in entry and "diagonal" not in entry
    assert sum("string_ci_table" in e for e in log[:built]) == 1 and sum("string_ci_diagonal" in e for e in log[:built]) == 1
    assert np.array_equal(H(system.u), u_before)                                  # system.u is never modified

    # DeterminantCI on the spin-doubled system, S_z = 0 sector
    general = system.construct_general_orbital_system()
    C2 = np.kron(X, np.eye(2))
    det = DeterminantCI(general, hip.asarray(C2), dets=sz_sector(2 * l, 2 * n, 0))
    Ed, _ = det.solve(3, tol=1e-9)
    print(f"{form}: against DeterminantCI max |dE| = {np.abs(E - H(Ed)).max():.2e} (bound {bound:.1e})")
    assert np.abs(E - H(Ed)).max() <= bound
    masks, v = ci.to_determinants(ci._c)
    assert np.array_equal(masks, det.dets)
    rho_so = H(kernels.det_ci_density1(dev(masks), v[0].contiguous(), 2 * l, 2 * n))
    rho = H(ci.one_body_density(0))
    tol = 3 * ref.gamma(ci.dim + 2) * (S2 if cplx else 1.0)                       # this density's bound and det_ci's on two blocks
    assert ratio_of(np.abs(rho - (rho_so[0::2, 0::2] + rho_so[1::2, 1::2])), np.float64(tol), f"{form} density, spin sum") <= 1.0
    assert np.array_equal(H(ci.transition_density(0, 0)), rho)
    occ, C_nat = ci.natural_orbitals(0)
    print(f"{form}: |sum of the occupations - {2 * n}| = {abs(float(H(occ).sum()) - 2 * n):.2e} (bound 1e-12)")
    assert abs(float(H(occ).sum()) - 2 * n) <= 1e-12 and H(C_nat).shape == (l, l)
    d = H(ci.transition_dipole(0, 1))
    want = np.einsum("dpq,qp->d", np.einsum("pa,dpq,qb->dab", X.conj(), H(system.dipole_moment), X), H(ci.transition_density(0, 1)))
    print(f"{form}: transition dipole against the contraction on the host: {np.abs(d - want).max():.2e} (bound 1e-12)")
    assert d.shape == (2,) and np.abs(d - want).max() <= 1e-12

    # RHF orbitals
    hf = HartreeFock(system)
    hf.scf()
    ci2 = hf.string_ci()
    E2, _ = ci2.solve(3, tol=1e-9)
    print(f"{form}: RHF orbitals max |dE| = {np.abs(H(E2) - e_nuc - lam[:3]).max():.2e} (bound {bound:.1e})")
    assert np.abs(H(E2) - e_nuc - lam[:3]).max() <= bound


def test_refusals():
    import quantum_systems_amd as qsa
    from quantum_systems_amd import StringCI, hip
    from quantum_systems_amd.sharded_module import ShardedTensor4

    system, (h, s, u, _) = random_spatial_system(4, 2, 99, False)
    X = hip.asarray(dref.loewdin(s))
    with pytest.raises(TypeError, match="DeterminantCI"):
        StringCI(system.construct_general_orbital_system(), X)
    with pytest.raises(TypeError):
        StringCI(object())
    with pytest.raises(ValueError, match="orthonormal"):
        StringCI(system)
    with pytest.raises(ValueError):
        StringCI(system, X, n_up=5)
    with pytest.raises(ValueError, match="ascending"):
        StringCI(system, X, strings_up=np.array([5, 3]))
    ci = StringCI(system, X, n_up=1, n_down=0)
    assert (ci.na, ci.nb) == (4, 1) and ci._ta is not ci._tb
    with pytest.raises(RuntimeError, match="solve"):
        ci.one_body_density(0)
    plain = torch.as_tensor(system.u).as_subclass(torch.Tensor).contiguous()
    system._basis_set.u = ShardedTensor4(plain, 4, 0, 0, 1)
    with pytest.raises(NotImplementedError, match="sharded"):
        StringCI(system, X)
