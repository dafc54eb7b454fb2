"""CPU-only checks of ``qs_string_ci_density2_spin`` / ``_spin_workspace`` / ``_spin_plan``: the symbols, every refused
argument and the order of the refusals (no GPU is touched: the checks run before any HIP call), the pass-and-slice
schedule over a grid of extents and budgets, and the GPU-only wrapper."""

import ctypes

import pytest

F64, C128 = 0, 1
BAD_EXTENT, NULL, MISALIGNED, WORKSPACE, BAD_DTYPE, ALIAS = -1, -2, -3, -4, -6, -7
NAMES = ("qs_string_ci_density2_spin_workspace", "qs_string_ci_density2_spin_plan", "qs_string_ci_density2_spin")
BIG = (1 << 31) - 1


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as entry

    entry.build()
    from quantum_systems_amd import _lib

    return _lib.load()


def test_symbols_are_exported_and_bound(lib):
    from quantum_systems_amd import _lib

    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name in NAMES:
        assert hasattr(raw, name) and name in _lib.SIGNATURES
    assert lib.qs_abi_version() == 4


def plan_of(lib, dt, m, na, nb, budget):
    out = (ctypes.c_int64 * 5)()
    rc = lib.qs_string_ci_density2_spin_plan(dt, m, na, nb, budget, ctypes.cast(out, ctypes.c_void_p))
    return rc, tuple(out)


def half(m, dt):
    """Columns of one spin in the ket panel: m^2, for fp64 rounded up to even."""
    return m * m + (m * m & 1 if dt == F64 else 0)


def panels(m, dt, pitch, es):
    """Bytes of the bra panel (2 m^2 + 1 rows) and the ket panel (2 h columns) over ``pitch`` determinants."""
    return (2 * m * m + 1 + 2 * half(m, dt)) * pitch * es


@pytest.mark.parametrize("dt", [F64, C128])
def test_plan_over_a_grid_of_extents_and_budgets(lib, dt):
    es = 8 if dt == F64 else 16
    for m, na, nb in [(1, 1, 1), (3, 3, 3), (4, 6, 4), (7, 35, 35), (9, 126, 126), (9, 126, 1), (9, 1, 126), (11, 330, 330),
                      (8, 35, 70), (16, 1820, 1820), (63, 70, 70)]:
        m2, h = m * m, half(m, dt)
        assert h % 2 == 0 or dt == C128
        row = panels(m, dt, nb, es)                                               # the panels of one alpha row, unpadded
        budgets = [0, 1, row - 1, row, 2 * row + 5, 3 * row + row // 2, 7 * row, (na // 2 + 1) * row + 64 * es * (4 * m2 + 3),
                   (na + 1) * row + (1 << 20), 1 << 40]
        for budget in budgets:
            rc, (rows, passes, T, kc, nbytes) = plan_of(lib, dt, m, na, nb, budget)
            assert rc == 0
            # passes x rows cover [0, na) exactly once, the last pass may be shorter but is not empty
            assert 1 <= rows <= na and (passes - 1) * rows < na <= passes * rows
            # the slices cover the determinants of a full pass, none of them empty; an even slice length
            assert T >= 1 and kc >= 1 and kc % 2 == 0 and T * kc >= rows * nb > (T - 1) * kc
            part = T * ((m2 + 1) * 2 * h + m2 * h) * es
            assert nbytes == part + panels(m, dt, T * kc, es)
            assert nbytes == lib.qs_string_ci_density2_spin_workspace(dt, m, na, nb, budget) and nbytes % 16 == 0
            # the panels stay within the budget, or are the (padded) panels of one row; the partial results on top are
            # small next to them wherever there is more than one slice
            eff = budget if budget > 0 else 2 << 30
            if rows > 1:
                assert panels(m, dt, T * kc, es) <= eff
            else:
                assert panels(m, dt, T * kc, es) <= max(eff, panels(m, dt, nb + 2 * T, es))
            if row <= eff:                                                        # one row fits: so does every pass
                assert panels(m, dt, rows * nb, es) <= eff
            assert T == 1 or 8 * part <= panels(m, dt, rows * nb, es)
            tiles = -(-(m2 + 1) // 128) * -(-2 * h // 128)
            assert T * tiles <= 256 + tiles
            # everything fits and is asked for: one pass
            if budget == 1 << 40:
                assert (rows, passes) == (na, 1)
            if budget in (1, row - 1):
                assert (rows, passes) == (1, na)
    # the schedule depends on the extents, the dtype and the budget alone, and the tuning key overrides the argument
    m, na, nb = 9, 126, 126
    row = panels(m, F64, nb, 8)
    try:
        base = plan_of(lib, F64, m, na, nb, 10 * row)
        assert base == plan_of(lib, F64, m, na, nb, 10 * row)
        assert lib.qs_tuning_set(b"string_ci_bytes", 4 * row) == 0
        assert plan_of(lib, F64, m, na, nb, 10 * row) == plan_of(lib, F64, m, na, nb, 0) != base
        assert lib.qs_tuning_set(b"string_ci_bytes", 0) == 0
        assert plan_of(lib, F64, m, na, nb, 10 * row) == base
    finally:
        lib.qs_tuning_reset()
    assert plan_of(lib, F64, m, na, nb, 4 * row)[1][1] > 1


def test_plan_and_workspace_refusals(lib):
    q = lib.qs_string_ci_density2_spin_workspace
    assert q(2, 8, 70, 70, 0) == BAD_DTYPE and q(-1, 8, 70, 70, 0) == BAD_DTYPE and q(2, 0, 70, 70, 0) == BAD_DTYPE
    for dt in (F64, C128):
        assert q(dt, 0, 5, 5, 0) == BAD_EXTENT and q(dt, 64, 5, 5, 0) == BAD_EXTENT
        assert q(dt, 8, 0, 5, 0) == BAD_EXTENT and q(dt, 8, 5, 0, 0) == BAD_EXTENT
        assert q(dt, 8, BIG, 1, 0) == BAD_EXTENT and q(dt, 8, 1, BIG, 0) == BAD_EXTENT
        assert q(dt, 8, 1 << 20, 1 << 20, 0) == BAD_EXTENT and q(dt, 8, 5, 5, -1) == BAD_EXTENT
    assert plan_of(lib, 2, 8, 70, 70, 0)[0] == BAD_DTYPE and plan_of(lib, F64, 64, 70, 70, 0)[0] == BAD_EXTENT
    assert plan_of(lib, F64, 8, 70, 70, -1)[0] == BAD_EXTENT
    assert lib.qs_string_ci_density2_spin_plan(F64, 8, 70, 70, 0, None) == NULL
    assert lib.qs_string_ci_density2_spin_plan(F64, 0, 70, 70, 0, None) == BAD_EXTENT


# fake, well-separated device addresses: every call below returns before any HIP call is made
TA, TB, BRA, KET, GAA, GAB, GBB, RHOA, RHOB, WORK = (k << 40 for k in range(1, 11))
M, NA, NB = 7, 35, 21
OUTS = (("gamma_aa", GAA), ("gamma_ab", GAB), ("gamma_bb", GBB), ("rho_a", RHOA), ("rho_b", RHOB))


def test_density2_spin_refusals_and_their_order(lib):
    need = lib.qs_string_ci_density2_spin_workspace(F64, M, NA, NB, 0)
    need_c = lib.qs_string_ci_density2_spin_workspace(C128, M, NA, NB, 0)
    assert need > 0 and need_c > need

    def call(c_dt=F64, ta=TA, tb=TB, m=M, na=NA, nb=NB, bra=BRA, ket=KET, gamma_aa=GAA, gamma_ab=GAB, gamma_bb=GBB, rho_a=RHOA,
             rho_b=RHOB, work=WORK, n=need, budget=0):
        return lib.qs_string_ci_density2_spin(c_dt, ta, tb, m, na, nb, bra, ket, gamma_aa, gamma_ab, gamma_bb, rho_a, rho_b, work, n,
                                              budget, None)

    assert call(c_dt=2) == BAD_DTYPE and call(c_dt=-1) == BAD_DTYPE
    assert call(m=0) == BAD_EXTENT and call(m=64) == BAD_EXTENT and call(na=0) == BAD_EXTENT and call(nb=BIG) == BAD_EXTENT
    assert call(na=1 << 20, nb=1 << 20) == BAD_EXTENT and call(budget=-1) == BAD_EXTENT
    names = ("ta", "tb", "bra", "ket") + tuple(name for name, _ in OUTS) + ("work",)
    for name in names:
        assert call(**{name: None}) == NULL, name
    for name, base in (("ta", TA), ("tb", TB), ("bra", BRA), ("ket", KET)) + OUTS:
        assert call(**{name: base + 2}) == MISALIGNED, name
    assert call(work=WORK + 8) == MISALIGNED
    for name, base in (("bra", BRA), ("ket", KET)) + OUTS:                               # a complex element is 16 bytes
        assert call(c_dt=C128, n=need_c, **{name: base + 8}) == MISALIGNED, name
    assert call(ta=TA + 4, tb=TB + 4, n=0) == WORKSPACE                                   # a table entry is 4 bytes
    assert call(n=need - 1) == WORKSPACE and call(n=0) == WORKSPACE and call(c_dt=C128, n=need_c - 1) == WORKSPACE
    assert call(c_dt=C128, n=need_c, gamma_ab=BRA) == ALIAS                               # exactly the query is enough
    # a smaller budget needs less: the size that is checked is the plan's
    small = lib.qs_string_ci_density2_spin_workspace(F64, M, NA, NB, 1)
    assert small < need and call(n=small, budget=1, gamma_aa=BRA) == ALIAS and call(n=small) == WORKSPACE
    # each of the five outputs overlapping an input, the workspace or another output
    v_bytes, g_bytes, r_bytes = NA * NB * 8, M ** 4 * 8, M * M * 8
    size = {"gamma_aa": g_bytes, "gamma_ab": g_bytes, "gamma_bb": g_bytes, "rho_a": r_bytes, "rho_b": r_bytes}
    for name, base in OUTS:
        assert call(**{name: BRA}) == ALIAS and call(**{name: KET + v_bytes - 8}) == ALIAS, name
        assert call(**{name: BRA - size[name] + 8}) == ALIAS, name
        assert call(**{name: TA + 4 * NA * M * M - 4}) == ALIAS and call(**{name: TB}) == ALIAS, name
        assert call(**{name: WORK + need - 8}) == ALIAS and call(**{name: WORK - size[name] + 8}) == ALIAS, name
        for other, at in OUTS:
            if other != name:
                assert call(**{name: at + size[other] - 8}) == ALIAS, (name, other)
                assert call(**{name: at - size[name] + 8}) == ALIAS, (name, other)
    for name in ("bra", "ket", "ta", "tb"):                                               # the workspace overlapping an input
        assert call(**{name: WORK + need - 16}) == ALIAS, name
    assert call(bra=WORK - v_bytes + 16) == ALIAS
    # bra == ket as one pointer is no overlap of an output
    assert call(ket=BRA, n=0) == WORKSPACE
    # order: dtype, extents, null, alignment, workspace, alias
    assert call(c_dt=2, m=0, ta=None) == BAD_DTYPE and call(m=0, ta=None) == BAD_EXTENT
    assert call(ta=None, bra=BRA + 2) == NULL and call(bra=BRA + 2, n=0) == MISALIGNED and call(n=0, gamma_bb=BRA) == WORKSPACE


def test_the_tuning_key_sets_the_workspace_that_is_checked(lib):
    need = lib.qs_string_ci_density2_spin_workspace(F64, M, NA, NB, 0)
    try:
        assert lib.qs_tuning_set(b"string_ci_bytes", 1) == 0
        small = lib.qs_string_ci_density2_spin_workspace(F64, M, NA, NB, 1 << 40)
        assert small < need and plan_of(lib, F64, M, NA, NB, 1 << 40)[1][:2] == (1, NA)
    finally:
        lib.qs_tuning_reset()
    assert lib.qs_string_ci_density2_spin_workspace(F64, M, NA, NB, 1 << 40) == need


def test_wrapper_is_gpu_only():
    import torch

    from quantum_systems_amd import kernels

    m = 4
    table = torch.zeros(6, m * m, dtype=torch.int32)
    c = torch.zeros(6, 6, dtype=torch.float64)
    with pytest.raises(RuntimeError, match="GPU only"):
        kernels.string_ci_density2_spin(table, table, m, c, c)
