"""CPU-only checks of ``qs_string_ci_sigma_plan`` and ``qs_string_ci_sigma_rows`` (sigma in passes over alpha rows of the
intermediate): the symbols, every refused argument and the order of the refusals (no GPU is touched: the checks run
before any HIP call), and the schedule over a grid of extents, forms and budgets."""

import ctypes

import pytest

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
    for name in ("qs_string_ci_sigma_plan", "qs_string_ci_sigma_rows"):
        assert hasattr(raw, name) and name in _lib.SIGNATURES
    assert lib.qs_abi_version() == 4


def ceil16(x):
    return (x + 15) // 16 * 16


def plan_of(lib, form, m, na, nb, K, budget):
    out = (ctypes.c_int64 * 4)()
    rc = lib.qs_string_ci_sigma_plan(*FORMS[form], m, na, nb, K, budget, ctypes.cast(out, ctypes.c_void_p))
    return rc, tuple(out)


def need(form, m, rows, nb, K):
    return 2 * ceil16(m * m * K * rows * nb * (8 if form == 0 else 16))


@pytest.mark.parametrize("form", list(FORMS))
def test_plan_over_a_grid_of_extents_and_budgets(lib, form):
    f = 2 if form == 2 else 1
    for m, na, nb in [(1, 1, 1), (3, 3, 3), (4, 6, 4), (7, 35, 35), (9, 126, 126), (9, 126, 1), (9, 1, 126), (11, 330, 330),
                      (8, 35, 70), (16, 1820, 1820), (63, 70, 70)]:
        for K in (1, 3):
            row = need(form, m, 1, nb, K)                                         # the D and G of one alpha row
            budgets = [0, 1, row - 1, row, 2 * row + 5, 3 * row + row // 2, 7 * row, (na // 2 + 1) * row + 48,
                       need(form, m, na, nb, K) - 1, need(form, m, na, nb, K), 1 << 50]
            for budget in budgets:
                rc, (rows, passes, cols, nbytes) = plan_of(lib, form, m, na, nb, K, budget)
                assert rc == 0
                eff = budget if budget > 0 else SHIPPED
                # the passes cover [0, na) once, the last one may be shorter but is not empty
                assert 1 <= rows <= na and passes * rows >= na > (passes - 1) * rows
                assert nbytes == need(form, m, rows, nb, K) and nbytes % 32 == 0
                assert cols == K * rows * nb * f <= BIG
                if rows > 1:
                    assert nbytes <= eff
                if row > eff:
                    assert (rows, passes) == (1, na)
                # no fewer passes would do: one more row per pass, in the passes before the evening, is over the budget
                if passes > 1:
                    most = -(-na // (passes - 1))                                 # the shortest passes that need one pass fewer
                    assert need(form, m, most, nb, K) > eff
                else:
                    assert rows == na and (nbytes <= eff or na == 1)
                assert plan_of(lib, form, m, na, nb, K, budget) == (0, (rows, passes, cols, nbytes))      # the same plan twice
    # one vector fits exactly where qs_string_ci_workspace(..., 1) does: the boundary of the Python routing
    m, na, nb = 9, 126, 126
    one = lib.qs_string_ci_workspace(*FORMS[form], m, na, nb, 1)
    assert one == need(form, m, na, nb, 1)
    assert plan_of(lib, form, m, na, nb, 1, one)[1][:2] == (na, 1) and plan_of(lib, form, m, na, nb, 1, one - 1)[1][1] == 2
    # 330 rows at a budget for 100: four passes, evened to 83, 83, 83, 81
    rc, (rows, passes, _, nbytes) = plan_of(lib, form, 11, 330, 330, 1, need(form, 11, 100, 330, 1))
    assert (rows, passes) == (83, 4) and nbytes == need(form, 11, 83, 330, 1)


def test_the_32_bit_columns_of_one_product(lib):
    """(2, 1 << 15, 1 << 15): 2^30 determinants.  The columns of every pass stay within 2^31 - 1; a real W against a
    complex c would need 2^31 of them for all rows and is refused by the extents rule of qs_string_ci_sigma, which this
    entry keeps."""
    m, n = 2, 1 << 15
    for form in (0, 1):
        for budget in (0, 1, 1 << 50):
            rc, (rows, passes, cols, nbytes) = plan_of(lib, form, m, n, n, 1, budget)
            assert rc == 0 and cols == rows * n <= BIG and passes * rows >= n > (passes - 1) * rows
            assert nbytes == need(form, m, rows, n, 1)
        assert plan_of(lib, form, m, n, n, 2, 0)[0] == BAD_EXTENT
    assert plan_of(lib, 2, m, n, n, 1, 0)[0] == BAD_EXTENT
    rc, (rows, passes, cols, _) = plan_of(lib, 2, m, n, n >> 1, 1, 1 << 50)
    assert rc == 0 and (rows, passes) == (n, 1) and cols == 2 * n * (n >> 1) <= BIG


def test_the_tuning_key_overrides_the_argument(lib):
    m, na, nb = 9, 126, 126
    row = need(0, m, 1, nb, 1)
    try:
        base = plan_of(lib, 0, m, na, nb, 1, 10 * row)
        assert base[1][:2] == (10, 13)
        assert lib.qs_tuning_set(b"string_ci_bytes", 4 * row) == 0
        assert plan_of(lib, 0, m, na, nb, 1, 10 * row) == plan_of(lib, 0, m, na, nb, 1, 0) != base
        assert plan_of(lib, 0, m, na, nb, 1, 0)[1][:2] == (4, 32)
        assert lib.qs_tuning_set(b"string_ci_bytes", 0) == 0                            # 0 = the argument again
        assert plan_of(lib, 0, m, na, nb, 1, 10 * row) == base
    finally:
        lib.qs_tuning_reset()
    assert plan_of(lib, 0, m, na, nb, 1, 0)[1][:2] == (na, 1)                            # 2 GiB shipped


def test_plan_refusals(lib):
    def q(h, c, m, na, nb, K, budget, out=True):
        buf = (ctypes.c_int64 * 4)()
        return lib.qs_string_ci_sigma_plan(h, c, m, na, nb, K, budget, ctypes.cast(buf, ctypes.c_void_p) if out else None)

    assert q(C128, F64, 8, 70, 70, 1, 0) == BAD_DTYPE and q(2, 0, 8, 70, 70, 1, 0) == BAD_DTYPE and q(0, -1, 8, 70, 70, 1, 0) == BAD_DTYPE
    assert q(C128, F64, 64, 70, 70, 1, 0) == BAD_DTYPE                                # the dtype pair comes first
    for dt in FORMS.values():
        assert q(*dt, 0, 5, 5, 1, 0) == BAD_EXTENT and q(*dt, 64, 5, 5, 1, 0) == BAD_EXTENT
        assert q(*dt, 8, 0, 5, 1, 0) == BAD_EXTENT and q(*dt, 8, 5, 0, 1, 0) == BAD_EXTENT
        assert q(*dt, 8, BIG, 1, 1, 0) == BAD_EXTENT and q(*dt, 8, 1, BIG, 1, 0) == BAD_EXTENT
        assert q(*dt, 8, 5, 5, 0, 0) == BAD_EXTENT and q(*dt, 8, 5, 5, -2, 0) == BAD_EXTENT
        assert q(*dt, 8, 1 << 20, 1 << 20, 1, 0) == BAD_EXTENT and q(*dt, 8, 5, 5, 1, -1) == BAD_EXTENT
        assert q(*dt, 8, 5, 5, 1, 0, out=False) == NULL and q(*dt, 0, 5, 5, 1, 0, out=False) == BAD_EXTENT


# fake, well-separated device addresses: every call below returns before any HIP call is made
KK, W, TA, TB, C, S, WORK = (k << 40 for k in range(1, 8))
M, NA, NB, K = 8, 70, 56, 3
NEED = 2 * M * M * K * NA * NB * 8                                                    # everything in one pass


def test_sigma_rows_refusals_and_their_order(lib):
    def call(h=F64, c_dt=F64, k=KK, w=W, ta=TA, tb=TB, m=M, na=NA, nb=NB, c=C, K=K, s=S, work=WORK, n=2 * NEED, budget=0):
        return lib.qs_string_ci_sigma_rows(h, c_dt, k, w, ta, tb, m, na, nb, c, K, s, work, n, budget, None)

    assert plan_of(lib, 0, M, NA, NB, K, 0)[1] == (NA, 1, K * NA * NB, NEED)
    assert call(h=C128, c_dt=F64) == BAD_DTYPE and call(h=3) == BAD_DTYPE and call(c_dt=-1) == BAD_DTYPE
    assert call(m=0) == BAD_EXTENT and call(m=64) == BAD_EXTENT and call(na=0) == BAD_EXTENT and call(nb=0) == BAD_EXTENT
    assert call(na=BIG) == BAD_EXTENT and call(nb=BIG) == BAD_EXTENT and call(K=0) == BAD_EXTENT and call(K=-1) == BAD_EXTENT
    assert call(na=1 << 20, nb=1 << 20) == BAD_EXTENT and call(K=1 << 62) == BAD_EXTENT
    assert call(budget=-1) == BAD_EXTENT and call(budget=-(1 << 40)) == BAD_EXTENT
    for name in ("k", "w", "ta", "tb", "c", "s", "work"):
        assert call(**{name: None}) == NULL, name
    for name, base in (("k", KK), ("w", W), ("ta", TA), ("tb", TB), ("c", C), ("s", S)):
        assert call(**{name: base + 2}) == MISALIGNED, name
    assert call(k=KK + 4) == MISALIGNED and call(work=WORK + 8) == MISALIGNED
    assert call(ta=TA + 4, tb=TB + 4, n=0) == WORKSPACE                                 # a table entry is 4 bytes
    for name, base in (("k", KK), ("w", W), ("c", C), ("s", S)):                        # a complex element is 16 bytes
        assert call(h=C128, c_dt=C128, **{name: base + 8}) == MISALIGNED, name
    assert call(h=F64, c_dt=C128, k=KK + 8, w=W + 8, n=0) == WORKSPACE and call(h=F64, c_dt=C128, c=C + 8) == MISALIGNED
    assert call(n=NEED - 1) == WORKSPACE and call(n=0) == WORKSPACE and call(h=F64, c_dt=C128, n=2 * NEED - 1) == WORKSPACE
    assert call(n=NEED, s=C) == ALIAS                                                   # exactly the plan is enough
    # a smaller budget needs less: the size that is checked is the plan's, under the tuning key too
    rc, (rows, passes, _, small) = plan_of(lib, 0, M, NA, NB, K, NEED // 7)
    assert rc == 0 and passes > 1 and small == need(0, M, rows, NB, K) <= NEED // 7 < NEED
    assert call(n=small, budget=NEED // 7, s=C) == ALIAS and call(n=small - 1, budget=NEED // 7) == WORKSPACE
    assert call(n=small) == WORKSPACE
    try:
        assert lib.qs_tuning_set(b"string_ci_bytes", NEED // 7) == 0
        assert call(n=small, s=C) == ALIAS and call(n=small - 1, s=C) == WORKSPACE
    finally:
        lib.qs_tuning_reset()
    # an output that overlaps an input
    s_bytes = K * NA * NB * 8
    assert call(s=C) == ALIAS and call(s=W) == ALIAS and call(s=KK) == ALIAS and call(s=TA) == ALIAS and call(s=TB) == ALIAS
    assert call(s=C + s_bytes - 8) == ALIAS and call(s=C - s_bytes + 8) == ALIAS
    assert call(s=W + 8 * (M ** 4 - 1)) == ALIAS and call(s=KK + 8 * (M * M - 1)) == ALIAS
    assert call(s=TA + 4 * NA * M * M - 8) == ALIAS and call(s=TB + 4 * NB * M * M - 8) == ALIAS
    assert call(s=WORK + NEED - 8) == ALIAS and call(s=WORK - s_bytes + 8) == ALIAS
    # the workspace overlapping an input: expand writes D_p while it reads c and the tables
    for name in ("c", "w", "k", "ta", "tb"):
        assert call(**{name: WORK + NEED - 16}) == ALIAS, name
    assert call(c=WORK - s_bytes + 16) == ALIAS
    assert call(tb=TA, nb=NA, n=0) == WORKSPACE                                         # one table for both spins passes the checks before it
    # order: dtype pair, extents (the budget among them), null, alignment, workspace, alias
    assert call(h=C128, c_dt=F64, m=0, budget=-1, k=None) == BAD_DTYPE
    assert call(m=0, k=None) == BAD_EXTENT and call(budget=-1, k=None) == BAD_EXTENT
    assert call(k=None, w=W + 4) == NULL
    assert call(w=W + 4, n=0) == MISALIGNED
    assert call(n=0, s=C) == WORKSPACE


def test_the_plan_wrapper(lib):
    import torch

    from quantum_systems_amd import kernels

    assert kernels.string_ci_sigma_plan(9, 126, 126, torch.float64) == plan_of(lib, 0, 9, 126, 126, 1, kernels.STRING_CI_BYTES)[1]
    assert kernels.string_ci_sigma_plan(9, 126, 126, torch.complex128, 3, torch.float64) == plan_of(lib, 2, 9, 126, 126, 3, 0)[1]
    with kernels.tuning(string_ci_bytes=need(1, 9, 5, 126, 1)):
        assert kernels.string_ci_sigma_plan(9, 126, 126, torch.complex128)[:2] == (5, 26)
    with pytest.raises(Exception):
        kernels.string_ci_sigma_plan(64, 126, 126, torch.float64)
