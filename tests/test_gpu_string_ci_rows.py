"""``qs_string_ci_sigma_rows`` -- sigma in passes over alpha rows of the intermediate -- and its routing in
``kernels.string_ci_sigma`` and ``StringCI`` on the GPU.

The entry is called directly (K vectors in one call, the byte budget as its argument) against
  * the dense oracle of tests/_string_ci_ref.py on the six small shapes, within the PATH bound of
    tests/test_gpu_string_ci.py, gamma_(3 m^2 + 4) sum_pr |E_pr| (|k_pr| |c| + sum_qs |W_pr,qs| |E_qs| |c|) (2 sqrt 2 for
    complex products).  The bound holds unchanged for any number of passes: a pass boundary stores and reloads the
    accumulator exactly, and the number and kind of operations per element is the same;
  * ``qs_string_ci_sigma`` itself: bit for bit where one pass holds all rows (same product extents, same chain), and within
    TWICE the bound (two computed values, one bound each) where the passes cut the product into other extents.
Past the dense Fock space the bound is evaluated on the device from the replacement tables (``device_bound``: the same
sum with moduli, in fp64, whose own rounding is far below the factor gamma); the dense-oracle test pins it to
``ref.path_bound``.  Budgets are given in alpha rows: ``need(form, m, r, nb, K)`` is the workspace of r rows, so the plan
takes r rows before it evens the passes.  Every test asserts the plan it expects before it runs, pre-fills sigma with
NaN, and prints its worst ratio to the bound before it asserts."""

import ctypes
import functools

import numpy as np
import pytest
import torch

import _det_ci_ref as dref
import _string_ci_density_ref as sref
import _string_ci_ref as ref

pytestmark = pytest.mark.gpu
FORMS = {"f64": (False, False), "real_h_complex_c": (False, True), "c128": (True, True)}
S2 = 2.0 * np.sqrt(2.0)
EVERYTHING = 1 << 50


def H(x):
    return torch.as_tensor(x).cpu().numpy()


def dev(x):
    return torch.from_numpy(np.array(x)).cuda()


def vectors(K, na, nb, cplx, seed):
    rng = np.random.default_rng(seed)
    c = rng.standard_normal((K, na, nb))
    return c + 1j * rng.standard_normal((K, na, nb)) if cplx else c


def ratio_of(err, bound, what):
    r = float((np.asarray(err, dtype=np.float64) / np.where(bound > 0, bound, 1.0)).max())
    print(f"{what}: worst error / bound = {r:.3f}")
    return r


def codes(k, c):
    return (1 if k.is_complex() else 0), (1 if c.is_complex() else 0)


def need(cplx_c, m, rows, nb, K):
    return 2 * ((m * m * K * rows * nb * (16 if cplx_c else 8) + 15) // 16 * 16)


def evened(na, r):
    """(rows, passes) of the plan that starts from r rows per pass."""
    passes = -(-na // min(r, na))
    return -(-na // passes), passes


def plan_of(k, c, m, na, nb, K, budget):
    from quantum_systems_amd import _lib

    out = (ctypes.c_int64 * 4)()
    assert _lib.load().qs_string_ci_sigma_plan(*codes(k, c), m, na, nb, K, budget, ctypes.addressof(out)) == 0
    return tuple(out)


def sigma_rows(k, W, ta, tb, c, budget, expect):
    """qs_string_ci_sigma_rows on the K vectors of c (K, na, nb) under ``budget`` bytes, sigma pre-filled with NaN; the
    plan is asserted to be ``expect`` = (rows, passes) first."""
    from quantum_systems_amd import _lib

    lib = _lib.load()
    K, na, nb = c.shape
    m = k.shape[0]
    rows, passes, cols, nbytes = plan_of(k, c, m, na, nb, K, budget)
    assert (rows, passes) == expect and nbytes == need(c.is_complex(), m, rows, nb, K), (rows, passes, nbytes)
    work = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    out = torch.full_like(c, float("nan"))
    rc = lib.qs_string_ci_sigma_rows(*codes(k, c), k.data_ptr(), W.data_ptr(), ta.data_ptr(), tb.data_ptr(), m, na, nb,
                                     c.data_ptr(), K, out.data_ptr(), work.data_ptr(), nbytes, budget,
                                     torch.cuda.current_stream().cuda_stream)
    assert rc == 0, rc
    torch.cuda.synchronize()
    return out


def sigma_once(k, W, ta, tb, c):
    """qs_string_ci_sigma on the K vectors of c in one call."""
    from quantum_systems_amd import _lib

    lib = _lib.load()
    K, na, nb = c.shape
    m = k.shape[0]
    nbytes = lib.qs_string_ci_workspace(*codes(k, c), m, na, nb, K)
    work = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    out = torch.full_like(c, float("nan"))
    rc = lib.qs_string_ci_sigma(*codes(k, c), k.data_ptr(), W.data_ptr(), ta.data_ptr(), tb.data_ptr(), m, na, nb,
                                c.data_ptr(), K, out.data_ptr(), work.data_ptr(), nbytes, torch.cuda.current_stream().cuda_stream)
    assert rc == 0
    torch.cuda.synchronize()
    return out


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
def problem(m, Na, Nb, hc):
    """Seeded (k, W, E, H longdouble) on the dense sector; computed once, never modified."""
    ht, ut = ref.random_hamiltonian(m, 100 + 10 * m + 3 * Na + Nb, hc)
    k, W = ref.kh_operands(ht, ut)
    out = k, W, ref.dense_E(m, Na, Nb), ref.dense_hamiltonian(ht, ut, Na, Nb, extended=True)
    for a in out:
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def operands(m, seed, hc):
    ht, ut = ref.random_hamiltonian(m, seed, hc)
    k, W = ref.kh_operands(ht, ut)
    return dev(k), dev(W)


@functools.lru_cache(maxsize=None)
def table(m, N):
    from quantum_systems_amd import kernels

    return kernels.string_ci_table(dev(ref.strings(m, N)), m, N)


@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("m,Na,Nb", ref.SHAPES)
def test_passes_of_one_and_of_two_rows_against_the_dense_oracle(m, Na, Nb, form):
    hc, cc = FORMS[form]
    k, W, E, Hx = problem(m, Na, Nb, hc)
    ta, tb = table(m, Na), table(m, Nb)
    na, nb = ta.shape[0], tb.shape[0]
    for K in (1, 3):
        c = vectors(K, na, nb, cc, 7 * K + m)
        flat = c.reshape(K, na * nb)
        exact = flat.astype(np.clongdouble if cc else np.longdouble) @ Hx.T
        bound = ref.path_bound(k, W, E, flat)
        on_device = device_bound(dev(k), dev(W), ta, tb, dev(c)).reshape(K, -1)
        assert np.abs(on_device - bound).max() <= 1e-12 * bound.max()             # the bound of the larger shapes, pinned here
        for r in (1, 2):
            got = H(sigma_rows(dev(k), dev(W), ta, tb, dev(c), need(cc, m, r, nb, K), evened(na, r)))
            assert got.shape == c.shape and got.dtype == (np.complex128 if cc else np.float64)
            assert ratio_of(np.abs(got.reshape(K, -1) - exact), bound, f"({m},{Na},{Nb}) {form} K={K} rows={r}") <= 1.0


@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("m,Na,Nb", [(9, 4, 4), (11, 4, 4)])
def test_one_pass_gives_the_bits_of_the_one_piece_sigma(m, Na, Nb, form):
    """The two entries run the same expand and fold kernels: this pins their drivers -- pass boundaries, product extents and
    the carving of the workspace -- against each other."""
    hc, cc = FORMS[form]
    k, W = operands(m, 900 + 10 * m + Na, hc)
    ta = tb = table(m, Na)
    na, nb = ta.shape[0], tb.shape[0]
    c = dev(vectors(2, na, nb, cc, m + Na))
    got = sigma_rows(k, W, ta, tb, c, EVERYTHING, (na, 1))
    want = sigma_once(k, W, ta, tb, c)
    assert not torch.isnan(want).any() and torch.equal(got, want)


# (m, Na, Nb, rows the budget holds): (7,3,3) 64-thread workgroups, m^2 = 49 leaves a ragged last chunk; (9,4,4) 126 strings
# on 128 threads; (6,6,3) and (9,5,0) distinct tables with na != nb (1 x 20 and 126 x 1); (11,4,4) 330 x 330, 256 threads,
# two tiles, the second with 74 live lanes, m^2 = 121: 100 rows are evened to four passes of 83, 83, 83, 81, and one row per
# pass has its targets mostly outside the pass
GEOMETRY = [(7, 3, 3, 11, (9, 4)), (9, 4, 4, 40, (32, 4)), (6, 6, 3, 1, (1, 1)), (9, 5, 0, 50, (42, 3)),
            (11, 4, 4, 100, (83, 4)), (11, 4, 4, 1, (1, 330))]


@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("m,Na,Nb,r,expect", GEOMETRY)
def test_launch_geometries_against_the_one_piece_sigma(m, Na, Nb, r, expect, form):
    from quantum_systems_amd import kernels

    hc, cc = FORMS[form]
    K = 2
    k, W = operands(m, 900 + 10 * m + Na, hc)
    ta, tb = table(m, Na), table(m, Nb)
    na, nb = ta.shape[0], tb.shape[0]
    assert evened(na, r) == expect
    c = dev(vectors(K, na, nb, cc, m + Na))
    assert kernels.string_ci_sigma_plan(m, na, nb, c.dtype, K, k.dtype)[1] == 1      # the shipped budget holds the vectors
    want = kernels.string_ci_sigma(k, W, ta, tb, c)
    budget = need(cc, m, r, nb, K)
    got = sigma_rows(k, W, ta, tb, c, budget, expect)
    bound = 2 * device_bound(k, W, ta, tb, c)
    assert ratio_of(H((got - want).abs()), bound, f"({m},{Na},{Nb}) {form} {na} x {nb}, {expect[1]} passes of {expect[0]}") <= 1.0
    assert float(want.abs().max()) > 1e3 * float(bound.max())                     # the comparison sees the result
    assert torch.equal(got, sigma_rows(k, W, ta, tb, c, budget, expect))           # a repeated call: identical bits


@pytest.mark.parametrize("form", list(FORMS))
def test_a_truncated_alpha_list_in_passes_of_two_rows(form):
    """A seeded random half of the alpha list of (8, 4, 3) against the host Knowles-Handy sum on that list: a table entry
    that points nowhere contributes nothing in either kernel."""
    from quantum_systems_amd import kernels

    hc, cc = FORMS[form]
    m, Na, Nb, K = 8, 4, 3, 3
    ht, ut = ref.random_hamiltonian(m, 843, hc)
    k, W = ref.kh_operands(ht, ut)
    rng = np.random.default_rng(843)
    full = ref.strings(m, Na)
    sa, sb = np.sort(rng.choice(full, len(full) // 2, replace=False)), ref.strings(m, Nb)
    na, nb = len(sa), len(sb)
    ta, tb = kernels.string_ci_table(dev(sa), m, Na), table(m, Nb)
    Ea, Eb = ref.list_E(sa, m), ref.list_E(sb, m)
    assert np.array_equal(H(ta), ref.table_from_E(Ea)) and np.array_equal(H(tb), ref.table_from_E(Eb))
    assert (H(ta) == 0).sum() > (ref.table_from_E(ref.list_E(full, m)) == 0).sum() // 2 + 1       # targets are missing
    c = vectors(K, na, nb, cc, 9)
    got = H(sigma_rows(dev(k), dev(W), ta, tb, dev(c), need(cc, m, 2, nb, K), (2, 18)))
    exact = ref.kh_sigma(k, W, Ea, Eb, c)
    bound = ref.kh_sigma(np.abs(k), np.abs(W), np.abs(Ea), np.abs(Eb), np.abs(c)).astype(np.float64)
    bound = ref.gamma(3 * m * m + 4) * bound * (S2 if (hc or cc) else 1.0)
    assert ratio_of(np.abs(got - exact), bound, f"half of the alpha list, {form}, 18 passes of 2") <= 1.0


def test_python_routing_by_the_budget_of_one_vector():
    from quantum_systems_amd import _lib, kernels

    m, Na, K = 9, 4, 3
    k, W = operands(m, 77, False)
    ta = tb = table(m, Na)
    na = nb = ta.shape[0]
    c = dev(vectors(K, na, nb, False, 3))
    one = _lib.load().qs_string_ci_workspace(0, 0, m, na, nb, 1)
    results = {}
    for budget, passes in ((one, 1), (one // 3, 3)):
        kernels.dispatch_log = log = []
        try:
            with kernels.tuning(string_ci_bytes=budget):
                assert kernels.string_ci_sigma_plan(m, na, nb, torch.float64)[1] == passes
                results[passes] = kernels.string_ci_sigma(k, W, ta, tb, c)
        finally:
            kernels.dispatch_log = None
        entry = [e for e in log if "string_ci" in e]
        assert len(entry) == 1 and len(log) == 1, log                             # one entry names the whole call
        calls = entry[0].split(" | ")
        assert len(calls) == K                                                    # one vector per call on either route
        for call in calls:
            assert "gemm" in call and "det_ci" not in call
            # as many expands and folds of the rectangular layout as passes, each pass expand, product, fold
            assert call.count("string_ci_expand_kernel<1, qs::ScRect>") == call.count("string_ci_expand_kernel") == passes
            assert call.count("string_ci_fold_kernel<0, qs::ScRect>") == call.count("string_ci_fold_kernel") == passes
            assert "ScTri" not in call and "symmetrize" not in call
            assert call.index("expand") < call.index("gemm") < call.index("fold")
    bound = 2 * device_bound(k, W, ta, tb, c)
    assert ratio_of(H((results[3] - results[1]).abs()), bound, "three passes against the one-piece route") <= 1.0
    assert float(results[1].abs().max()) > 1e3 * float(bound.max())


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
def test_solver_and_one_body_density_under_a_fifth_of_one_vector(form):
    """(6, 3, 3), 20 x 20: every Davidson step and the density run in passes.  The dense spectrum is that of the host's
    sum_pr E_pr (k_pr + sum_qs W_pr,qs E_qs) with E = E1 x 1 + 1 x E1 from the ladder oracle's one-spin E1 (12 spin orbitals
    are past the dense Fock space of the Jordan-Wigner oracle)."""
    from quantum_systems_amd import StringCI, _lib, hip, kernels

    cplx = FORMS[form][0]
    l, n = 6, 3
    system, (h, s, u, e_nuc) = random_spatial_system(l, n, 633, cplx)
    X = dref.loewdin(s)
    ht = X.conj().T @ h @ X
    ut = np.einsum("pa,qb,pqrs,rc,sd->abcd", X.conj(), X.conj(), u, X, X, optimize=True)
    k, W = ref.kh_operands(ht, ut)
    strs = ref.strings(l, n)
    E1 = ref.list_E(strs, l)
    eye = np.eye(len(strs))
    Ef = np.array([np.kron(e, eye) + np.kron(eye, e) for e in E1.reshape(l * l, len(strs), len(strs))]).astype(W.dtype)
    inner = np.tensordot(W, Ef, axes=((1,), (0,))) + k.reshape(l * l)[:, None, None] * np.eye(Ef.shape[1])
    lam = np.linalg.eigvalsh(np.matmul(Ef, inner).sum(0))
    bound = 1e-8 * max(1.0, np.abs(lam).max())

    code = 1 if cplx else 0
    dt = torch.complex128 if cplx else torch.float64
    one = _lib.load().qs_string_ci_workspace(code, code, l, 20, 20, 1)
    ci = StringCI(system, hip.asarray(X))
    assert (ci.m, ci.na, ci.nb) == (l, 20, 20)
    kernels.dispatch_log = log = []
    try:
        with kernels.tuning(string_ci_bytes=one // 5):
            assert kernels.string_ci_sigma_plan(l, 20, 20, dt)[:2] == (4, 5)
            E, c = ci.solve(3, tol=1e-9)
            steps = len(log)
            rho = H(ci.one_body_density(0))
            plan = (ctypes.c_int64 * 5)()
            assert _lib.load().qs_string_ci_density2_plan(code, l, 20, 20, 0, ctypes.addressof(plan)) == 0
            occ, _ = ci.natural_orbitals(0)
    finally:
        kernels.dispatch_log = None
    E = H(E)
    print(f"{form}: max |dE| = {np.abs(E - e_nuc - lam[:3]).max():.2e} (bound {bound:.1e}), {ci.iterations} iterations")
    assert ci.converged and np.abs(E - e_nuc - lam[:3]).max() <= bound
    assert steps == ci.iterations
    for e in log[:steps]:                                                         # every call of every step: the plan's 5 passes
        for call in e.split(" | "):
            assert call.count("string_ci_expand_kernel") == call.count("string_ci_fold_kernel") == 5 and "ScTri" not in call
            assert call.index("expand") < call.index("gemm") < call.index("fold")
    density = log[steps]
    assert f"string_ci_expand_panel_kernel<{code + 1}, false, 1>" in density and "string_ci_expand_kernel<" not in density and plan[1] > 1

    want = H(ci.one_body_density(0))                                              # the shipped budget: qs_string_ci_density1
    state = H(ci._c[0])
    rbound = sref.rho_sum_bound((E1, E1), state, state, int(plan[2]))
    assert ratio_of(np.abs(rho - want), rbound, f"{form}: one-body density in {plan[1]} passes against one piece") <= 1.0
    assert abs(float(H(occ).sum()) - 2 * n) <= l * float(rbound.max()) + 1e-12
