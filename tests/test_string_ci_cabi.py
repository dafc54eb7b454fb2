"""CPU-only checks of the string-CI entries (``qs_string_ci_table`` / ``_diagonal`` / ``_workspace`` / ``_group`` /
``_sigma`` / ``_density1``): the symbols, every refused argument and the order of the refusals (no GPU is touched: the
checks run before any HIP call), the workspace formula, the grouping under the byte budget and its tuning key, and the
GPU-only wrappers."""

import pytest

F64, C128 = 0, 1
BAD_EXTENT, NULL, MISALIGNED, WORKSPACE, BAD_DTYPE, ALIAS = -1, -2, -3, -4, -6, -7
NAMES = ("qs_string_ci_table", "qs_string_ci_diagonal", "qs_string_ci_workspace", "qs_string_ci_group",
         "qs_string_ci_sigma", "qs_string_ci_density1")
BIG = (1 << 31) - 1


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as entry

    entry.build()
    from quantum_systems_amd import _lib

    return _lib.load()


def test_symbols_are_exported_and_bound(lib):
    import ctypes

    from quantum_systems_amd import _lib

    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name in NAMES:
        assert hasattr(raw, name) and name in _lib.SIGNATURES
    assert lib.qs_abi_version() == 4


def ceil16(x):
    return (x + 15) // 16 * 16


def test_workspace_formula(lib):
    q = lib.qs_string_ci_workspace
    for m, na, nb, K in [(1, 1, 1, 1), (3, 3, 3, 1), (8, 70, 56, 9), (16, 1820, 1820, 8), (63, 70, 70, 1), (9, 126, 1, 3)]:
        assert q(F64, F64, m, na, nb, K) == 2 * ceil16(m * m * K * na * nb * 8)
        assert q(F64, C128, m, na, nb, K) == 2 * m * m * K * na * nb * 16
        assert q(C128, C128, m, na, nb, K) == 2 * m * m * K * na * nb * 16
    assert q(C128, F64, 8, 70, 70, 1) == BAD_DTYPE and q(2, 0, 8, 70, 70, 1) == BAD_DTYPE and q(0, -1, 8, 70, 70, 1) == BAD_DTYPE
    assert q(C128, F64, 64, 70, 70, 1) == BAD_DTYPE                                   # the dtype pair comes first
    for dt in ((F64, F64), (F64, C128), (C128, C128)):
        assert q(*dt, 0, 5, 5, 1) == BAD_EXTENT and q(*dt, 64, 5, 5, 1) == BAD_EXTENT
        assert q(*dt, 8, 0, 5, 1) == BAD_EXTENT and q(*dt, 8, 5, 0, 1) == BAD_EXTENT
        assert q(*dt, 8, BIG, 1, 1) == BAD_EXTENT and q(*dt, 8, 1, BIG, 1) == BAD_EXTENT
        assert q(*dt, 8, 5, 5, 0) == BAD_EXTENT and q(*dt, 8, 5, 5, -2) == BAD_EXTENT
        assert q(*dt, 8, BIG - 1, BIG - 1, 1 << 40) == BAD_EXTENT                      # a product past int64
    # the columns of one product: K na nb, twice that for a real W against complex c
    assert q(F64, F64, 2, 1 << 15, 1 << 15, 1) > 0 and q(F64, F64, 2, 1 << 15, 1 << 15, 2) == BAD_EXTENT
    assert q(C128, C128, 2, 1 << 15, 1 << 15, 1) > 0 and q(F64, C128, 2, 1 << 15, 1 << 15, 1) == BAD_EXTENT


def test_group_under_the_byte_budget(lib):
    g = lib.qs_string_ci_group
    m, na, nb = 8, 70, 56
    one = lib.qs_string_ci_workspace(F64, F64, m, na, nb, 1)
    try:
        assert g(F64, F64, m, na, nb, 9, 0) == 9                                       # 2 GiB shipped
        assert g(F64, F64, m, na, nb, 9, 4 * one) == 4 and g(F64, F64, m, na, nb, 9, 4 * one - 1) == 3
        assert g(F64, F64, m, na, nb, 9, 1) == 1 and g(F64, F64, m, na, nb, 3, 100 * one) == 3
        assert g(F64, C128, m, na, nb, 9, 4 * one) == 2
        assert lib.qs_tuning_set(b"string_ci_bytes", one) == 0
        assert g(F64, F64, m, na, nb, 9, 4 * one) == 1
        assert lib.qs_tuning_set(b"string_ci_bytes", 0) == 0                            # 0 = the shipped value
        assert g(F64, F64, m, na, nb, 9, 4 * one) == 4
        assert lib.qs_tuning_set(b"string_ci_bytes", -1) == BAD_EXTENT
        assert g(F64, F64, 2, 1 << 15, 1 << 15, 5, 0) == 1                              # the product's 32-bit columns
    finally:
        lib.qs_tuning_reset()
    assert g(C128, F64, m, na, nb, 9, 0) == BAD_DTYPE
    assert g(F64, F64, 64, na, nb, 9, 0) == BAD_EXTENT and g(F64, F64, m, na, nb, 0, 0) == BAD_EXTENT
    assert g(F64, F64, m, na, nb, 9, -5) == BAD_EXTENT


# fake, well-separated device addresses: every call below returns before any HIP call is made
KK, W, TA, TB, C, S, WORK, SA, SB, D, HT, UT, RHO, BRA, KET = (k << 40 for k in range(1, 16))
M, NA, NB, K = 8, 70, 56, 3
NEED = 2 * M * M * K * NA * NB * 8


def test_sigma_refusals_and_their_order(lib):
    def call(h=F64, c_dt=F64, k=KK, w=W, ta=TA, tb=TB, m=M, na=NA, nb=NB, c=C, K=K, s=S, work=WORK, n=2 * NEED):
        return lib.qs_string_ci_sigma(h, c_dt, k, w, ta, tb, m, na, nb, c, K, s, work, n, None)

    assert call(h=C128, c_dt=F64) == BAD_DTYPE and call(h=3) == BAD_DTYPE and call(c_dt=-1) == BAD_DTYPE
    assert call(m=0) == BAD_EXTENT and call(m=64) == BAD_EXTENT and call(na=0) == BAD_EXTENT and call(nb=0) == BAD_EXTENT
    assert call(na=BIG) == BAD_EXTENT and call(nb=BIG) == BAD_EXTENT and call(K=0) == BAD_EXTENT and call(K=-1) == BAD_EXTENT
    assert call(na=1 << 20, nb=1 << 20) == BAD_EXTENT and call(K=1 << 62) == BAD_EXTENT
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
    assert call(n=NEED, s=C) == ALIAS                                                   # exactly the query is enough
    # an output that overlaps an input
    s_bytes = K * NA * NB * 8
    assert call(s=C) == ALIAS and call(s=W) == ALIAS and call(s=KK) == ALIAS and call(s=TA) == ALIAS and call(s=TB) == ALIAS
    assert call(s=C + s_bytes - 8) == ALIAS and call(s=C - s_bytes + 8) == ALIAS
    assert call(s=W + 8 * (M ** 4 - 1)) == ALIAS and call(s=KK + 8 * (M * M - 1)) == ALIAS
    assert call(s=TA + 4 * NA * M * M - 8) == ALIAS and call(s=TB + 4 * NB * M * M - 8) == ALIAS
    assert call(s=WORK + NEED - 8) == ALIAS
    # the workspace overlapping an input: expand writes D while it reads c and the tables
    for name in ("c", "w", "k", "ta", "tb"):
        assert call(**{name: WORK + NEED - 16}) == ALIAS, name
    assert call(c=WORK - s_bytes + 16) == ALIAS
    assert call(tb=TA, nb=NA, n=0) == WORKSPACE                                         # one table for both spins passes the checks before it
    # order: dtype pair, extents, null, alignment, workspace, alias
    assert call(h=C128, c_dt=F64, m=0, k=None) == BAD_DTYPE
    assert call(m=0, k=None) == BAD_EXTENT
    assert call(k=None, w=W + 4) == NULL
    assert call(w=W + 4, n=0) == MISALIGNED
    assert call(n=0, s=C) == WORKSPACE


def test_table_refusals_and_their_order(lib):
    def call(strings=SA, n=NA, m=M, N=4, table=TA):
        return lib.qs_string_ci_table(strings, n, m, N, table, None)

    assert call(m=0) == BAD_EXTENT and call(m=64) == BAD_EXTENT and call(N=-1) == BAD_EXTENT and call(N=M + 1) == BAD_EXTENT
    assert call(n=0) == BAD_EXTENT and call(n=BIG) == BAD_EXTENT
    assert call(strings=None) == NULL and call(table=None) == NULL
    assert call(strings=SA + 4) == MISALIGNED and call(table=TA + 2) == MISALIGNED
    assert call(table=SA) == ALIAS and call(table=SA + 8 * (NA - 1)) == ALIAS and call(table=SA - 4 * NA * M * M + 4) == ALIAS
    assert call(m=0, strings=None) == BAD_EXTENT and call(strings=None, table=TA + 2) == NULL
    assert call(strings=SA + 4, table=SA) == MISALIGNED


def test_diagonal_refusals_and_their_order(lib):
    def call(h=F64, ht=HT, ut=UT, sa=SA, na=NA, Na=4, sb=SB, nb=NB, Nb=3, m=M, D=D):
        return lib.qs_string_ci_diagonal(h, ht, ut, sa, na, Na, sb, nb, Nb, m, D, None)

    assert call(h=2) == BAD_DTYPE and call(h=-1) == BAD_DTYPE
    assert call(m=0) == BAD_EXTENT and call(m=64) == BAD_EXTENT and call(Na=-1) == BAD_EXTENT and call(Nb=M + 1) == BAD_EXTENT
    assert call(na=0) == BAD_EXTENT and call(nb=BIG) == BAD_EXTENT
    for name in ("ht", "ut", "sa", "sb", "D"):
        assert call(**{name: None}) == NULL, name
    for name, base in (("ht", HT), ("ut", UT), ("sa", SA), ("sb", SB), ("D", D)):
        assert call(**{name: base + 4}) == MISALIGNED, name
    assert call(h=C128, ht=HT + 8) == MISALIGNED and call(h=C128, ut=UT + 8) == MISALIGNED
    assert call(D=HT) == ALIAS and call(D=UT + 8 * (M ** 4 - 1)) == ALIAS and call(D=SA) == ALIAS
    assert call(D=SB - 8 * (NA * NB - 1)) == ALIAS
    assert call(h=2, m=0, ht=None) == BAD_DTYPE and call(m=0, ht=None) == BAD_EXTENT
    assert call(ht=None, ut=UT + 4) == NULL and call(ut=UT + 4, D=HT) == MISALIGNED


def test_density_refusals_and_their_order(lib):
    need = M * M * NA * NB * 8

    def call(c_dt=F64, ta=TA, tb=TB, m=M, na=NA, nb=NB, bra=BRA, ket=KET, rho=RHO, work=WORK, n=need):
        return lib.qs_string_ci_density1(c_dt, ta, tb, m, na, nb, bra, ket, rho, work, n, None)

    assert call(c_dt=2) == BAD_DTYPE and call(c_dt=-1) == BAD_DTYPE
    assert call(m=0) == BAD_EXTENT and call(m=64) == BAD_EXTENT and call(na=0) == BAD_EXTENT and call(nb=BIG) == BAD_EXTENT
    for name in ("ta", "tb", "bra", "ket", "rho", "work"):
        assert call(**{name: None}) == NULL, name
    for name, base in (("ta", TA), ("tb", TB), ("bra", BRA), ("ket", KET), ("rho", RHO)):
        assert call(**{name: base + 2}) == MISALIGNED, name
    assert call(c_dt=C128, bra=BRA + 8, n=2 * need) == MISALIGNED and call(work=WORK + 8) == MISALIGNED
    assert call(n=need - 1) == WORKSPACE and call(c_dt=C128, n=2 * need - 1) == WORKSPACE
    # the query with K = 1 is sufficient
    assert lib.qs_string_ci_workspace(F64, F64, M, NA, NB, 1) >= need
    assert call(rho=BRA) == ALIAS and call(rho=KET + 8 * (NA * NB - 1)) == ALIAS and call(rho=TA) == ALIAS
    assert call(rho=TB - 8 * (M * M - 1)) == ALIAS and call(rho=WORK) == ALIAS
    for name in ("bra", "ket", "ta", "tb"):                                            # the workspace overlapping an input
        assert call(**{name: WORK + need - 16}) == ALIAS, name
    assert call(c_dt=2, m=0, ta=None) == BAD_DTYPE and call(m=0, ta=None) == BAD_EXTENT
    assert call(ta=None, bra=BRA + 2) == NULL and call(bra=BRA + 2, n=0) == MISALIGNED and call(n=0, rho=BRA) == WORKSPACE


def test_wrappers_are_gpu_only():
    import torch

    from quantum_systems_amd import kernels

    m = 4
    ht, ut = torch.zeros(m, m, dtype=torch.float64), torch.zeros(m, m, m, m, dtype=torch.float64)
    strings = torch.tensor([3, 5, 6, 9, 10, 12], dtype=torch.int64)
    table = torch.zeros(6, m * m, dtype=torch.int32)
    c = torch.zeros(6, 6, dtype=torch.float64)
    with pytest.raises(RuntimeError, match="GPU only"):
        kernels.string_ci_table(strings, m, 2)
    with pytest.raises(RuntimeError, match="GPU only"):
        kernels.string_ci_diagonal(ht, ut, strings, 2, strings, 2)
    with pytest.raises(RuntimeError, match="GPU only"):
        kernels.string_ci_sigma(ht, torch.zeros(m * m, m * m, dtype=torch.float64), table, table, c)
    with pytest.raises(RuntimeError, match="GPU only"):
        kernels.string_ci_density1(table, table, m, c, c)
    assert kernels.STRING_CI_BYTES > 0
