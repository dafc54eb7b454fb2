"""CPU-only checks of ``qs_string_ci_sigma_sym_plan`` and ``qs_string_ci_sigma_sym`` (sigma on the lower triangle of the
intermediate for vectors with c = tau c^T): the symbols, every refused argument and the order of the refusals (no GPU is
touched: the checks run before any HIP call), the greedy schedule over a grid of extents, forms and budgets, and the
identity the kernels rest on, pinned on the host with NumPy."""

import ctypes

import numpy as np
import pytest

import _string_ci_ref as ref

F64, C128 = 0, 1
BAD_EXTENT, NULL, MISALIGNED, WORKSPACE, BAD_DTYPE, ALIAS = -1, -2, -3, -4, -6, -7
FORMS = {0: (F64, F64), 1: (C128, C128), 2: (F64, C128)}
BIG = (1 << 31) - 1
SHIPPED = 2 << 30


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as entry

    entry.build()
    from quantum_systems_amd import _lib

    return _lib.load()


def test_symbols_are_exported_and_bound(lib):
    from quantum_systems_amd import _lib

    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name in ("qs_string_ci_sigma_sym_plan", "qs_string_ci_sigma_sym"):
        assert hasattr(raw, name) and name in _lib.SIGNATURES
    assert lib.qs_abi_version() == 4


def ceil16(x):
    return (x + 15) // 16 * 16


def off(r):
    return r * (r + 1) // 2


def need(form, m, length, K):
    """Workspace of a pass of ``length`` packed elements per (qs) and vector."""
    return 2 * ceil16(m * m * K * length * (8 if form == 0 else 16))


def greedy(form, m, n, K, eff):
    """The boundaries by the rule of the header, one row at a time."""
    b = [0]
    while b[-1] < n:
        r = b[-1] + 1
        while r + 1 <= n and need(form, m, off(r + 1) - off(b[-1]), K) <= eff:
            r += 1
        b.append(r)
    return b


def plan_of(lib, form, m, n, K, budget, room=None):
    """(rc, plan, boundaries): the passes from a first query without boundaries, then the boundaries."""
    out = (ctypes.c_int64 * 4)()
    rc = lib.qs_string_ci_sigma_sym_plan(*FORMS[form], m, n, K, budget, ctypes.cast(out, ctypes.c_void_p), None, 0)
    if rc:
        return rc, tuple(out), None
    first = tuple(out)
    room = first[0] + 1 if room is None else room
    cuts = (ctypes.c_int64 * max(room, 1))(*([-7] * max(room, 1)))
    rc = lib.qs_string_ci_sigma_sym_plan(*FORMS[form], m, n, K, budget, ctypes.cast(out, ctypes.c_void_p),
                                         ctypes.cast(cuts, ctypes.c_void_p), room)
    assert rc or tuple(out) == first                                              # the same plan twice
    return rc, first, tuple(cuts)


@pytest.mark.parametrize("form", list(FORMS))
def test_plan_over_a_grid_of_extents_and_budgets(lib, form):
    f = 2 if form == 2 else 1
    for m, n in [(1, 1), (3, 3), (4, 6), (5, 10), (7, 35), (9, 126), (11, 330), (16, 1820), (63, 70)]:
        for K in (1, 3):
            row = need(form, m, n, K)                                             # the D and G of the longest packed row
            whole = need(form, m, off(n), K)
            budgets = [0, 1, row - 1, row, 2 * row + 5, 3 * row + row // 2, 7 * row, whole // 4, whole // 2 + 48, whole - 1,
                       whole, 1 << 50]
            for budget in budgets:
                rc, (passes, longest, cols, nbytes), cuts = plan_of(lib, form, m, n, K, budget)
                assert rc == 0
                eff = budget if budget > 0 else SHIPPED
                want = greedy(form, m, n, K, eff)
                assert list(cuts) == want and passes == len(want) - 1
                # the passes cover [0, n) once and none is empty
                assert cuts[0] == 0 and cuts[-1] == n and all(b > a for a, b in zip(cuts, cuts[1:]))
                lengths = [off(b) - off(a) for a, b in zip(cuts, cuts[1:])]
                assert longest == max(lengths) and sum(lengths) == off(n)
                assert nbytes == need(form, m, longest, K) and nbytes % 32 == 0
                assert cols == K * longest * f <= BIG
                for a, b, length in zip(cuts, cuts[1:], lengths):
                    if b - a > 1:
                        assert need(form, m, length, K) <= eff                    # within the budget
                    if b < n:
                        assert need(form, m, off(b + 1) - off(a), K) > eff        # and no further row would be
                if row > eff:
                    # even the longest row is over the budget: the rows from the first such one on go one per pass
                    first = next(r for r in range(n) if need(form, m, r + 1, K) > eff)
                    assert all(b - a == 1 for a, b in zip(cuts, cuts[1:]) if a >= first)
                if need(form, m, 1, K) > eff:
                    assert passes == n
                if whole <= eff:
                    assert passes == 1
    # half of the square: where the full intermediate of (9, 126, 126) needs its budget, the triangle needs 8001 / 15876 of it
    m, n = 9, 126
    square = lib.qs_string_ci_workspace(*FORMS[form], m, n, n, 1)
    assert plan_of(lib, form, m, n, 1, square)[1][3] == need(form, m, off(n), 1) <= square * 8001 // 15876 + 32


def test_the_boundaries_are_optional_and_their_room_is_checked(lib):
    m, n, K = 9, 126, 1
    budget = need(0, m, off(n) // 4, K)
    rc, plan, cuts = plan_of(lib, 0, m, n, K, budget)
    assert rc == 0 and plan[0] > 2 and len(cuts) == plan[0] + 1
    rc, _, untouched = plan_of(lib, 0, m, n, K, budget, room=plan[0])
    assert rc == BAD_EXTENT and set(untouched) == {-7}                                # nothing is written
    rc, again, more = plan_of(lib, 0, m, n, K, budget, room=plan[0] + 3)
    assert rc == 0 and again == plan and more[:plan[0] + 1] == cuts and set(more[plan[0] + 1:]) == {-7}


def test_the_32_bit_columns_of_one_product(lib):
    m, n = 2, 1 << 15
    for form in (0, 1):
        rc, (passes, longest, cols, nbytes), _ = plan_of(lib, form, m, n, 1, 1 << 50)
        assert rc == 0 and passes == 1 and longest == off(n) and cols == off(n) <= BIG and nbytes == need(form, m, off(n), 1)
        assert plan_of(lib, form, m, n, 2, 0)[0] == BAD_EXTENT                        # the extents rule of the full sigma
    assert plan_of(lib, 2, m, n, 1, 0)[0] == BAD_EXTENT


def test_the_tuning_key_overrides_the_argument(lib):
    m, n = 9, 126
    unit = need(0, m, off(n) // 8, 1)
    try:
        base = plan_of(lib, 0, m, n, 1, 4 * unit)
        assert base[0] == 0 and list(base[2]) == greedy(0, m, n, 1, 4 * unit) and base[1][0] > 1
        assert lib.qs_tuning_set(b"string_ci_bytes", unit) == 0
        assert plan_of(lib, 0, m, n, 1, 4 * unit) == plan_of(lib, 0, m, n, 1, 0) != base
        assert list(plan_of(lib, 0, m, n, 1, 0)[2]) == greedy(0, m, n, 1, unit)
        assert lib.qs_tuning_set(b"string_ci_bytes", 0) == 0                            # 0 = the argument again
        assert plan_of(lib, 0, m, n, 1, 4 * unit) == base
    finally:
        lib.qs_tuning_reset()
    assert plan_of(lib, 0, m, n, 1, 0)[1][0] == 1                                       # 2 GiB shipped


def test_plan_refusals(lib):
    def q(h, c, m, n, K, budget, out=True):
        buf = (ctypes.c_int64 * 4)()
        return lib.qs_string_ci_sigma_sym_plan(h, c, m, n, K, budget, ctypes.cast(buf, ctypes.c_void_p) if out else None, None, 0)

    assert q(C128, F64, 8, 70, 1, 0) == BAD_DTYPE and q(2, 0, 8, 70, 1, 0) == BAD_DTYPE and q(0, -1, 8, 70, 1, 0) == BAD_DTYPE
    assert q(C128, F64, 64, 70, 1, 0) == BAD_DTYPE                                    # the dtype pair comes first
    for dt in FORMS.values():
        assert q(*dt, 0, 5, 1, 0) == BAD_EXTENT and q(*dt, 64, 5, 1, 0) == BAD_EXTENT
        assert q(*dt, 8, 0, 1, 0) == BAD_EXTENT and q(*dt, 8, BIG, 1, 0) == BAD_EXTENT
        assert q(*dt, 8, 5, 0, 0) == BAD_EXTENT and q(*dt, 8, 5, -2, 0) == BAD_EXTENT
        assert q(*dt, 8, 1 << 20, 1, 0) == BAD_EXTENT and q(*dt, 8, 5, 1, -1) == BAD_EXTENT
        assert q(*dt, 8, 5, 1, 0, out=False) == NULL and q(*dt, 0, 5, 1, 0, out=False) == BAD_EXTENT


# fake, well-separated device addresses: every call below returns before any HIP call is made
KK, W, T, C, S, WORK = (k << 40 for k in range(1, 7))
M, N, K = 8, 70, 3
NEED = 2 * M * M * K * off(N) * 8                                                     # everything in one pass


def test_sigma_sym_refusals_and_their_order(lib):
    def call(h=F64, c_dt=F64, k=KK, w=W, t=T, m=M, n=N, parity=1, c=C, K=K, s=S, work=WORK, nbytes=2 * NEED, budget=0):
        return lib.qs_string_ci_sigma_sym(h, c_dt, k, w, t, m, n, parity, c, K, s, work, nbytes, budget, None)

    assert plan_of(lib, 0, M, N, K, 0)[1] == (1, off(N), K * off(N), NEED)
    assert call(h=C128, c_dt=F64) == BAD_DTYPE and call(h=3) == BAD_DTYPE and call(c_dt=-1) == BAD_DTYPE
    for parity in (0, 2, -2, 1 << 32, -(1 << 32) + 1):
        assert call(parity=parity) == BAD_EXTENT, parity
    assert call(m=0) == BAD_EXTENT and call(m=64) == BAD_EXTENT and call(n=0) == BAD_EXTENT and call(n=BIG) == BAD_EXTENT
    assert call(K=0) == BAD_EXTENT and call(K=-1) == BAD_EXTENT and call(n=1 << 20) == BAD_EXTENT and call(K=1 << 62) == BAD_EXTENT
    assert call(budget=-1) == BAD_EXTENT and call(budget=-(1 << 40)) == BAD_EXTENT
    for name in ("k", "w", "t", "c", "s", "work"):
        assert call(**{name: None}) == NULL, name
    for name, base in (("k", KK), ("w", W), ("t", T), ("c", C), ("s", S)):
        assert call(**{name: base + 2}) == MISALIGNED, name
    assert call(k=KK + 4) == MISALIGNED and call(work=WORK + 8) == MISALIGNED
    assert call(t=T + 4, nbytes=0) == WORKSPACE                                       # a table entry is 4 bytes
    for name, base in (("k", KK), ("w", W), ("c", C), ("s", S)):                        # a complex element is 16 bytes
        assert call(h=C128, c_dt=C128, **{name: base + 8}) == MISALIGNED, name
    assert call(h=F64, c_dt=C128, k=KK + 8, w=W + 8, nbytes=0) == WORKSPACE and call(h=F64, c_dt=C128, c=C + 8) == MISALIGNED
    assert call(nbytes=NEED - 1) == WORKSPACE and call(nbytes=0) == WORKSPACE and call(h=F64, c_dt=C128, nbytes=2 * NEED - 1) == WORKSPACE
    assert call(nbytes=NEED, s=C) == ALIAS and call(nbytes=NEED, s=C, parity=-1) == ALIAS    # exactly the plan is enough
    # a smaller budget needs less: the size that is checked is the plan's, under the tuning key too
    rc, (passes, longest, _, small), _ = plan_of(lib, 0, M, N, K, NEED // 7)
    assert rc == 0 and passes > 1 and small == need(0, M, longest, K) <= NEED // 7 < NEED
    assert call(nbytes=small, budget=NEED // 7, s=C) == ALIAS and call(nbytes=small - 1, budget=NEED // 7) == WORKSPACE
    assert call(nbytes=small) == WORKSPACE
    try:
        assert lib.qs_tuning_set(b"string_ci_bytes", NEED // 7) == 0
        assert call(nbytes=small, s=C) == ALIAS and call(nbytes=small - 1, s=C) == WORKSPACE
    finally:
        lib.qs_tuning_reset()
    # an output that overlaps an input: sigma and c are full (K, n, n) arrays
    s_bytes = K * N * N * 8
    assert call(s=C) == ALIAS and call(s=W) == ALIAS and call(s=KK) == ALIAS and call(s=T) == ALIAS
    assert call(s=C + s_bytes - 8) == ALIAS and call(s=C - s_bytes + 8) == ALIAS
    assert call(s=W + 8 * (M ** 4 - 1)) == ALIAS and call(s=KK + 8 * (M * M - 1)) == ALIAS
    assert call(s=T + 4 * N * M * M - 8) == ALIAS
    assert call(s=WORK + NEED - 8) == ALIAS and call(s=WORK - s_bytes + 8) == ALIAS
    # the workspace overlapping an input: expand writes D_p while it reads c and the table
    for name in ("c", "w", "k", "t"):
        assert call(**{name: WORK + NEED - 16}) == ALIAS, name
    assert call(c=WORK - s_bytes + 16) == ALIAS
    # order: dtype pair, extents (parity and the budget among them), null, alignment, workspace, alias
    assert call(h=C128, c_dt=F64, m=0, parity=0, budget=-1, k=None) == BAD_DTYPE
    assert call(m=0, k=None) == BAD_EXTENT and call(parity=0, k=None) == BAD_EXTENT and call(budget=-1, k=None) == BAD_EXTENT
    assert call(k=None, w=W + 4) == NULL
    assert call(w=W + 4, nbytes=0) == MISALIGNED
    assert call(nbytes=0, s=C) == WORKSPACE


def test_the_plan_wrapper(lib):
    import torch

    from quantum_systems_amd import kernels

    rc, plan, cuts = plan_of(lib, 0, 9, 126, 1, kernels.STRING_CI_BYTES)
    assert kernels.string_ci_sigma_sym_plan(9, 126, torch.float64) == (plan, cuts)
    rc, plan, cuts = plan_of(lib, 2, 9, 126, 3, 0)
    assert kernels.string_ci_sigma_sym_plan(9, 126, torch.complex128, 3, torch.float64) == (plan, cuts)
    with kernels.tuning(string_ci_bytes=need(1, 9, off(126) // 5, 1)):
        got, cuts = kernels.string_ci_sigma_sym_plan(9, 126, torch.complex128)
        assert list(cuts) == greedy(1, 9, 126, 1, need(1, 9, off(126) // 5, 1)) and got[0] == len(cuts) - 1 > 4
    with pytest.raises(Exception):
        kernels.string_ci_sigma_sym_plan(64, 126, torch.float64)


@pytest.mark.parametrize("m,N,cplx", [(5, 2, False), (4, 2, True)])
@pytest.mark.parametrize("tau", [1, -1])
def test_the_lower_triangle_of_x_carries_sigma(m, N, cplx, tau):
    """S + tau S^T, with S folded from the stored elements X[r, c], r >= c, alone (weight 1/2 on the diagonal), is the
    Knowles-Handy sigma of c = tau c^T.  Both sides are sums of the same products: the tolerance is the fp64 path bound
    gamma_(3 m^2 + 5) on the sum of moduli, which a longdouble evaluation meets with room."""
    ht, ut = ref.random_hamiltonian(m, 40 + m, cplx)
    k, W = ref.kh_operands(ht, ut)
    E = ref.list_E(ref.strings(m, N), m)
    n = E.shape[2]
    rng = np.random.default_rng(5 * m + tau)
    c = rng.standard_normal((2, n, n)) + (1j * rng.standard_normal((2, n, n)) if cplx else 0)
    c = 0.5 * (c + tau * c.transpose(0, 2, 1))
    want = ref.kh_sigma(k, W, E, E, c)
    wide = np.clongdouble if cplx else np.longdouble
    Ef = E.reshape(m * m, n, n).astype(wide)
    cw = c.astype(wide)
    D = np.einsum("aij,kjb->akib", Ef, cw) + np.einsum("abj,kij->akib", Ef, cw)
    assert np.array_equal(D, tau * D.transpose(0, 1, 3, 2))                           # every row of D has the parity
    X = np.tensordot(W.astype(wide), D, axes=((1,), (0,))) + k.reshape(m * m).astype(wide)[:, None, None, None] * cw[None]
    weight = np.tril(np.ones((n, n)), -1) + 0.5 * np.eye(n)                           # 0 above the diagonal: never read
    Xl = X * weight
    S = np.einsum("aij,akjb->kib", Ef, Xl) + np.einsum("abj,akij->kib", Ef, Xl)
    got = S + tau * S.transpose(0, 2, 1)
    moduli = ref.kh_sigma(np.abs(k), np.abs(W), np.abs(E), np.abs(E), np.abs(c)).astype(np.float64)
    bound = ref.gamma(3 * m * m + 5) * moduli * (2.0 * np.sqrt(2.0) if cplx else 1.0)
    err = np.abs(got - want).astype(np.float64)
    print(f"({m},{N},{N}) tau={tau:+d}: worst error / bound = {(err / bound).max():.3e}, |sigma| max {np.abs(want).max():.2f}")
    assert (err <= bound).all() and np.abs(want).max() > 1e3 * bound.max()
    assert np.array_equal(got, tau * got.transpose(0, 2, 1))
    if tau < 0:
        assert not np.diagonal(X, axis1=2, axis2=3).any()                             # the diagonal of X is exactly 0
