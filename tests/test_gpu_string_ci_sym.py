"""``qs_string_ci_sigma_sym`` -- sigma on the lower triangle of the intermediate for vectors with c = tau c^T -- its routing
in ``kernels.string_ci_sigma_sym`` and ``StringCI(..., spin_parity=tau)`` on the GPU.

The entry is called directly (K vectors in one call, the byte budget as its argument) against
  * the host Knowles-Handy sum ``ref.kh_sigma`` on ``ref.list_E``, within ``ref.path_bound`` taken with n = 3 m^2 + 5: the
    term set and the term moduli are those of the full sum (a dropped term is tau times a kept term of the transposed
    element, the weight 1/2 is exact), and the closing addition S + tau S^T is one more operation;
  * ``kernels.string_ci_sigma`` on the same vector in every launch geometry, within TWICE ``device_bound`` (two computed
    values, one bound each), the helper of tests/test_gpu_string_ci_rows.py, which that file pins to ``ref.path_bound``.
Every case asserts the boundaries of its plan against the greedy rule first, pre-fills sigma with NaN, checks the exact
parity of the result -- sigma[k,a,b] and tau sigma[k,b,a] equal as values everywhere and bit for bit where they are not
zero, the diagonal +0.0 for tau = -1 --, and prints its worst ratio to the bound before it asserts."""

import ctypes
import functools

import numpy as np
import pytest
import torch

import _det_ci_ref as dref
import _string_ci_ref as ref

pytestmark = pytest.mark.gpu
FORMS = {"f64": (False, False), "real_h_complex_c": (False, True), "c128": (True, True)}
S2 = 2.0 * np.sqrt(2.0)
EVERYTHING = 1 << 50


def H(x):
    return torch.as_tensor(x).cpu().numpy()


def dev(x):
    return torch.from_numpy(np.array(x)).cuda()


def off(r):
    return r * (r + 1) // 2


def vectors(K, n, cplx, seed, tau):
    """K seeded vectors (n, n) with c = tau c^T, bit for bit."""
    rng = np.random.default_rng(seed)
    c = rng.standard_normal((K, n, n))
    if cplx:
        c = c + 1j * rng.standard_normal((K, n, n))
    c = 0.5 * (c + tau * c.transpose(0, 2, 1))
    assert np.array_equal(c, tau * c.transpose(0, 2, 1))
    return np.ascontiguousarray(c)


def ratio_of(err, bound, what):
    r = float((np.asarray(err, dtype=np.float64) / np.where(bound > 0, bound, 1.0)).max())
    print(f"{what}: worst error / bound = {r:.3f}")
    return r


def codes(k, c):
    return (1 if k.is_complex() else 0), (1 if c.is_complex() else 0)


def need(cplx_c, m, length, K):
    return 2 * ((m * m * K * length * (16 if cplx_c else 8) + 15) // 16 * 16)


def greedy(cplx_c, m, n, K, budget):
    b = [0]
    while b[-1] < n:
        r = b[-1] + 1
        while r + 1 <= n and need(cplx_c, m, off(r + 1) - off(b[-1]), K) <= budget:
            r += 1
        b.append(r)
    return b


def sigma_sym(k, W, t, c, tau, budget):
    """qs_string_ci_sigma_sym on the K vectors of c (K, n, n) under ``budget`` bytes, sigma pre-filled with NaN; the plan's
    boundaries are asserted to be the greedy ones first.  Returns (sigma, passes)."""
    from quantum_systems_amd import _lib

    lib = _lib.load()
    K, n, _ = c.shape
    m = k.shape[0]
    want = greedy(c.is_complex(), m, n, K, budget)
    plan = (ctypes.c_int64 * 4)()
    cuts = (ctypes.c_int64 * len(want))()
    assert lib.qs_string_ci_sigma_sym_plan(*codes(k, c), m, n, K, budget, ctypes.addressof(plan), ctypes.addressof(cuts), len(want)) == 0
    longest = max(off(b) - off(a) for a, b in zip(want, want[1:]))
    assert list(cuts) == want and tuple(plan)[:2] == (len(want) - 1, longest) and plan[3] == need(c.is_complex(), m, longest, K)
    work = torch.empty(plan[3], dtype=torch.uint8, device="cuda")
    out = torch.full_like(c, float("nan"))
    rc = lib.qs_string_ci_sigma_sym(*codes(k, c), k.data_ptr(), W.data_ptr(), t.data_ptr(), m, n, tau, c.data_ptr(), K,
                                    out.data_ptr(), work.data_ptr(), plan[3], budget, torch.cuda.current_stream().cuda_stream)
    assert rc == 0, rc
    torch.cuda.synchronize()
    return out, plan[0]


def assert_parity(out, tau):
    """sigma[k,a,b] == tau sigma[k,b,a]: equal values everywhere (no NaN), identical bits wherever the value is not a zero,
    and +0.0 on the diagonal for tau = -1."""
    a = np.ascontiguousarray(H(out))
    K, n, _ = a.shape
    parts = a.view(np.float64).reshape(K, n, n, -1)
    mirror = np.ascontiguousarray(tau * parts.transpose(0, 2, 1, 3))
    assert np.array_equal(parts, mirror)
    there = parts != 0
    assert np.array_equal(parts.view(np.int64)[there], mirror.view(np.int64)[there])
    if tau < 0:
        diagonal = np.ascontiguousarray(np.diagonal(parts, axis1=1, axis2=2))
        assert not diagonal.view(np.int64).any()


def device_bound(k, W, ta, tb, c):
    """The path bound of sigma for c (K, na, nb), elementwise, from the tables: the Knowles-Handy sum on moduli."""
    m2 = ta.shape[1]
    m = int(round(m2 ** 0.5))
    ca = c.abs().to(torch.float64)
    K, na, nb = ca.shape
    ja, jb = (ta.abs().long() - 1).clamp(min=0), (tb.abs().long() - 1).clamp(min=0)
    ma, mb = (ta != 0).to(torch.float64), (tb != 0).to(torch.float64)
    Da = ca[:, ja, :] * ma[None, :, :, None]                                     # (K, na, m2, nb)
    Db = ca[:, :, jb] * mb[None, None, :, :]                                     # (K, na, nb, m2)
    D = Da.permute(2, 0, 1, 3) + Db.permute(3, 0, 1, 2)                          # (m2, K, na, nb)
    X = (W.abs().to(torch.float64) @ D.reshape(m2, -1)).reshape(m2, K, na, nb)
    X = X + k.abs().to(torch.float64).reshape(m2, 1, 1, 1) * ca[None]
    pr = torch.arange(m2, device=c.device)
    Xa = X[pr[None, :], :, ja, :] * ma[:, :, None, None]                         # (na, m2, K, nb)
    Xb = X[pr[None, :], :, :, jb] * mb[:, :, None, None]                         # (nb, m2, K, na)
    b = Xa.sum(1).permute(1, 0, 2) + Xb.sum(1).permute(1, 2, 0)
    cplx = k.is_complex() or c.is_complex()
    return H(ref.gamma(3 * m * m + 4) * b * (S2 if cplx else 1.0))


@functools.lru_cache(maxsize=None)
def sector(m, N):
    """(E1, Ef) of N alpha and N beta particles: E of one spin on its string list (m, m, n, n), and
    E = E1 x 1 + 1 x E1 on the determinants (m, m, n^2, n^2), from the ladder oracle; computed once, never modified."""
    E1 = ref.list_E(ref.strings(m, N), m)
    n = E1.shape[2]
    eye = np.eye(n)
    Ef = np.array([np.kron(e, eye) + np.kron(eye, e) for e in E1.reshape(m * m, n, n)]).reshape(m, m, n * n, n * n)
    for a in (E1, Ef):
        a.setflags(write=False)
    return E1, Ef


@functools.lru_cache(maxsize=None)
def host_operands(m, seed, hc):
    ht, ut = ref.random_hamiltonian(m, seed, hc)
    k, W = ref.kh_operands(ht, ut)
    for a in (k, W):
        a.setflags(write=False)
    return k, W


@functools.lru_cache(maxsize=None)
def operands(m, seed, hc):
    k, W = host_operands(m, seed, hc)
    return dev(k), dev(W)


@functools.lru_cache(maxsize=None)
def table(m, N):
    from quantum_systems_amd import kernels

    return kernels.string_ci_table(dev(ref.strings(m, N)), m, N)


@pytest.mark.parametrize("tau", [1, -1])
@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("m,N", [(4, 2), (5, 2), (5, 3), (6, 3)])
def test_one_pass_and_passes_of_two_rows_against_the_host_oracle(m, N, form, tau):
    """n = 6 / 10 / 10 / 20: a single 64-lane tile, mostly dead lanes."""
    hc, cc = FORMS[form]
    k, W = host_operands(m, 100 + 10 * m + 4 * N, hc)
    E1, Ef = sector(m, N)
    t = table(m, N)
    n = t.shape[0]
    assert np.array_equal(H(t), ref.table_from_E(E1))
    for K in (1, 3):
        c = vectors(K, n, cc, 7 * K + m + tau, tau)
        exact = ref.kh_sigma(k, W, E1, E1, c)
        bound = ref.path_bound(k, W, Ef, c.reshape(K, n * n)).reshape(K, n, n) * (ref.gamma(3 * m * m + 5) / ref.gamma(3 * m * m + 4))
        # one pass, and a budget that holds the two longest packed rows
        for budget in (EVERYTHING, need(cc, m, 2 * n - 1, K)):
            out, passes = sigma_sym(dev(k), dev(W), t, dev(c), tau, budget)
            assert (passes == 1) == (budget == EVERYTHING)
            got = H(out)
            assert got.shape == c.shape and got.dtype == (np.complex128 if cc else np.float64)
            what = f"({m},{N},{N}) {form} tau={tau:+d} K={K} passes={passes}"
            assert ratio_of(np.abs(got - exact), bound, what) <= 1.0
            assert_parity(out, tau)
            again, _ = sigma_sym(dev(k), dev(W), t, dev(c), tau, budget)
            assert torch.equal(out.view(torch.float64).view(torch.int64), again.view(torch.float64).view(torch.int64))     # a repeated call: identical bits


# (m, N, packed elements the budget holds as a divisor of off(n), passes expected): (8,4,4) 70 strings on the 128-lane tile;
# (9,4,4) 126 strings at one pass, at about four passes and at one row per pass; (10,5,5) 252 strings on the 256-lane tile;
# (11,4,4) 330 strings, two tiles, the last with 74 strings, tile 1 wholly above the diagonal for Ia < 256, at one pass and
# at about five passes.  A divisor 0 is a budget of one byte: every pass one row.
GEOMETRY = [(8, 4, 1, (1, 1)), (9, 4, 1, (1, 1)), (9, 4, 4, (4, 5)), (9, 4, 0, (126, 126)), (10, 5, 1, (1, 1)), (11, 4, 1, (1, 1)),
            (11, 4, 5, (5, 6))]


@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("m,N,divisor,expect", GEOMETRY)
def test_launch_geometries_against_the_full_sigma(m, N, divisor, expect, form):
    from quantum_systems_amd import kernels

    hc, cc = FORMS[form]
    K = 2
    k, W = operands(m, 900 + 10 * m + N, hc)
    t = table(m, N)
    n = t.shape[0]
    budget = need(cc, m, -(-off(n) // divisor), K) if divisor else 1
    for tau in (1, -1):
        c = dev(vectors(K, n, cc, m + N + tau, tau))
        assert kernels.string_ci_sigma_plan(m, n, n, c.dtype, K, k.dtype)[1] == 1      # the shipped budget holds the full intermediate
        want = kernels.string_ci_sigma(k, W, t, t, c)
        got, passes = sigma_sym(k, W, t, c, tau, budget)
        assert expect[0] <= passes <= expect[1], passes
        bound = 2 * device_bound(k, W, t, t, c)
        assert ratio_of(H((got - want).abs()), bound, f"({m},{N},{N}) {form} tau={tau:+d} n={n}, {passes} passes") <= 1.0
        assert float(want.abs().max()) > 1e3 * float(bound.max())                     # the comparison sees the result
        assert_parity(got, tau)
        again, _ = sigma_sym(k, W, t, c, tau, budget)
        assert torch.equal(got.view(torch.float64).view(torch.int64), again.view(torch.float64).view(torch.int64))


def test_python_routing_one_call_groups_and_one_vector_per_call():
    from quantum_systems_amd import kernels

    m, N, K, tau = 6, 3, 5, 1
    k, W = operands(m, 77, False)
    t = table(m, N)
    n = t.shape[0]
    c = dev(vectors(K, n, False, 3, tau))
    whole = lambda g: need(False, m, off(n), g)                                   # noqa: E731
    results = {}
    # (budget, calls, passes of each call): all five vectors in one pass; groups of 2, 2 and 1; one vector in three passes
    for budget, sizes, passes in ((whole(K), [5], 1), (whole(2), [2, 2, 1], 1), (whole(1) // 3 + 64, [1] * 5, None)):
        kernels.dispatch_log = log = []
        try:
            with kernels.tuning(string_ci_bytes=budget):
                count = {}
                for g in sorted(set(sizes)):
                    plan, cuts = kernels.string_ci_sigma_sym_plan(m, n, torch.float64, g)
                    assert list(cuts) == greedy(False, m, n, g, budget) and (passes is None or plan[0] == passes)
                    if passes is None:
                        assert plan[0] > 2
                    count[g] = plan[0]
                if sizes[0] < K:
                    assert kernels.string_ci_sigma_sym_plan(m, n, torch.float64, sizes[0] + 1)[0][0] > 1
                out = torch.full_like(c, float("nan"))
                assert kernels.string_ci_sigma_sym(k, W, t, c, tau, out=out) is out
                results[tuple(sizes)] = out
        finally:
            kernels.dispatch_log = None
        assert len(log) == 1, log                                                 # one entry names the whole call
        calls = log[0].split(" | ")
        assert len(calls) == len(sizes)
        for call, g in zip(calls, sizes):
            assert "string_ci_expand_kernel<1, qs::ScTri>" in call and "string_ci_fold_kernel<0, qs::ScTri>" in call and "gemm" in call
            assert "string_ci_symmetrize_kernel<1>" in call and "ScRect" not in call
            assert call.index("expand") < call.index("gemm") < call.index("fold") < call.index("symmetrize")
            assert call.count("symmetrize") == 1
            assert call.count("string_ci_expand_kernel<1, qs::ScTri>") == call.count("string_ci_fold_kernel<0, qs::ScTri>") == count[g]
        assert_parity(out, tau)
    bound = 2 * device_bound(k, W, t, t, c)
    base = results[(5,)]
    for sizes, out in results.items():
        if sizes != (5,):
            assert ratio_of(H((out - base).abs()), bound, f"calls of {list(sizes)} vectors against one call") <= 1.0
    assert float(base.abs().max()) > 1e3 * float(bound.max())
    with pytest.raises(ValueError):
        kernels.string_ci_sigma_sym(k, W, t, c, 0)
    with pytest.raises(ValueError):
        kernels.string_ci_sigma_sym(k, W, t, c[:, :, :-1], 1)


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
def test_solver_returns_the_lowest_states_of_each_parity(form):
    """(6, 3, 3), 20 x 20, against the dense spectrum of ``ref.kh_hamiltonian`` split by the parity <v|P|v> of its
    eigenvectors: +1 keeps the three lowest states of even S, -1 the three lowest of odd S."""
    from quantum_systems_amd import StringCI, hip, kernels

    cplx = FORMS[form][0]
    l, n = 6, 3
    system, (h, s, u, e_nuc) = random_spatial_system(l, n, 633, cplx)
    X = dref.loewdin(s)
    ht = X.conj().T @ h @ X
    ut = np.einsum("pa,qb,pqrs,rc,sd->abcd", X.conj(), X.conj(), u, X, X, optimize=True)
    k, W = ref.kh_operands(ht, ut)
    _, Ef = sector(l, n)
    lam, vec = np.linalg.eigh(ref.kh_hamiltonian(k, W, Ef))
    v = vec.T.reshape(-1, 20, 20)
    parity = np.einsum("kab,kba->k", v.conj(), v).real
    assert np.abs(np.abs(parity) - 1.0).max() < 1e-8                              # no degeneracy mixes the two parities
    bound = 1e-8 * max(1.0, np.abs(lam).max())
    spins = {1: [S * (S + 1) for S in (0, 2)], -1: [S * (S + 1) for S in (1, 3)]}    # three particles per spin: S <= 3

    for tau in (1, -1):
        want = lam[parity * tau > 0][:3]
        ci = StringCI(system, hip.asarray(X), spin_parity=tau)
        assert (ci.m, ci.na, ci.nb, ci.spin_parity) == (l, 20, 20, tau)
        kernels.dispatch_log = log = []
        try:
            E, c = ci.solve(3, tol=1e-9)
            steps = len(log)
        finally:
            kernels.dispatch_log = None
        E = H(E)
        print(f"{form} tau={tau:+d}: max |dE| = {np.abs(E - e_nuc - want).max():.2e} (bound {bound:.1e}), {ci.iterations} iterations")
        assert ci.converged and np.abs(E - e_nuc - want).max() <= bound
        assert steps == ci.iterations
        for e in log:
            for call in e.split(" | "):
                assert call.count("string_ci_expand_kernel") == call.count("string_ci_fold_kernel") >= 1 and "ScRect" not in call
                assert call.index("expand") < call.index("gemm") < call.index("fold") < call.index("symmetrize")
        states = ci._c
        assert tuple(states.shape) == (3, 20, 20)
        assert torch.equal(states, tau * states.transpose(1, 2))
        assert float((torch.linalg.vector_norm(states.reshape(3, -1), dim=1) - 1).abs().max()) < 1e-12
        for j in range(3):
            s2 = ci.spin_squared(j)
            print(f"  root {j}: <S^2> = {s2:.10f}")
            assert min(abs(s2 - x) for x in spins[tau]) <= 1e-8
            rho = H(ci.one_body_density(j))
            assert abs(np.trace(rho).real - 2 * n) <= 1e-10
            assert abs(ci.energy_from_densities(j) - E[j]) <= bound
        # sigma() symmetrises what it is given: H on the part of the vector that has the parity
        x = dev(np.random.default_rng(tau + 5).standard_normal((20, 20))).to(states.dtype)
        part = 0.5 * (x + tau * x.transpose(0, 1))
        full = kernels.string_ci_sigma(ci._k, ci._W, ci._ta, ci._tb, part)
        both = 2 * device_bound(ci._k, ci._W, ci._ta, ci._tb, part[None])[0]
        assert ratio_of(H((ci.sigma(x) - full).abs()), both, f"{form} tau={tau:+d}: sigma of an unsymmetric vector") <= 1.0
        with pytest.raises(ValueError):
            ci.solve(20 * (20 + tau) // 2 + 1)

    # spin_parity=None: the route and the result of the full sector, as before
    ci = StringCI(system, hip.asarray(X))
    assert ci.spin_parity is None
    kernels.dispatch_log = log = []
    try:
        E, _ = ci.solve(3, tol=1e-9)
    finally:
        kernels.dispatch_log = None
    assert ci.converged and np.abs(H(E) - e_nuc - lam[:3]).max() <= bound
    for e in log:                                                                 # one pass of the rectangular layout per call
        for call in e.split(" | "):
            assert call.count("string_ci_expand_kernel") == call.count("string_ci_fold_kernel") == 1
            assert call.index("expand") < call.index("gemm") < call.index("fold")
            assert "ScTri" not in call and "symmetrize" not in call
    with pytest.raises(ValueError):
        StringCI(system, hip.asarray(X), n_up=3, n_down=2, spin_parity=1)
    with pytest.raises(ValueError):
        StringCI(system, hip.asarray(X), strings_up=ref.strings(l, n)[:-1], spin_parity=-1)
    with pytest.raises(ValueError):
        StringCI(system, hip.asarray(X), spin_parity=2)
