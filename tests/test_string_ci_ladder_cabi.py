"""CPU-only checks of ``qs_string_ci_ladder_table`` and ``qs_string_ci_ladder``: the symbols, every refused argument and the
order of the refusals (no GPU is touched: the checks run before any HIP call), and the GPU-only wrappers."""

import ctypes

import pytest

F64, C128 = 0, 1
BAD_EXTENT, NULL, MISALIGNED, BAD_DTYPE, ALIAS = -1, -2, -3, -6, -7
NAMES = ("qs_string_ci_ladder_table", "qs_string_ci_ladder")
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


# fake, well-separated device addresses: every call below returns before any HIP call is made
PHI, TABLE, C, OUT, TARGET, SOURCE = (k << 44 for k in range(1, 7))
M, NA, NB, NT, D, K = 8, 70, 56, 28, 3, 2


def test_table_refusals_and_their_order(lib):
    def call(target=TARGET, n_t=NT, source=SOURCE, n_s=NB, m=M, table=TABLE):
        return lib.qs_string_ci_ladder_table(target, n_t, source, n_s, m, table, None)

    # 1: extents
    assert call(m=0) == BAD_EXTENT and call(m=64) == BAD_EXTENT and call(m=-1) == BAD_EXTENT
    assert call(n_t=0) == BAD_EXTENT and call(n_t=BIG) == BAD_EXTENT and call(n_s=0) == BAD_EXTENT and call(n_s=BIG) == BAD_EXTENT
    # 2: null pointers
    for name in ("target", "source", "table"):
        assert call(**{name: None}) == NULL, name
    # 3: alignment: 8 for the lists, 4 for the table
    assert call(target=TARGET + 4) == MISALIGNED and call(source=SOURCE + 4) == MISALIGNED and call(table=TABLE + 2) == MISALIGNED
    # 4: the table shares a byte with a list, down to the last byte of either
    t_bytes = 4 * NT * M
    assert call(table=TARGET) == ALIAS and call(table=TARGET + 8 * NT - 4) == ALIAS and call(table=TARGET - t_bytes + 4) == ALIAS
    assert call(table=SOURCE) == ALIAS and call(table=SOURCE + 8 * NB - 4) == ALIAS and call(table=SOURCE - t_bytes + 4) == ALIAS
    # order: extents, null, alignment, alias
    assert call(m=0, target=None) == BAD_EXTENT and call(n_s=0, table=None) == BAD_EXTENT
    assert call(target=None, source=SOURCE + 4) == NULL and call(source=SOURCE + 4, table=SOURCE) == MISALIGNED


def test_ladder_refusals_and_their_order(lib):
    def call(h_dt=F64, c_dt=F64, phi=PHI, d=D, spin=0, table=TABLE, m=M, n_alpha=4, na_s=NA, nb_s=NB, n_t=NT, c=C, K=K, out=OUT):
        return lib.qs_string_ci_ladder(h_dt, c_dt, phi, d, spin, table, m, n_alpha, na_s, nb_s, n_t, c, K, out, None)

    # 1: the forms of sigma; a complex phi against a real c is refused
    assert call(h_dt=2) == BAD_DTYPE and call(c_dt=-1) == BAD_DTYPE and call(h_dt=C128, c_dt=F64) == BAD_DTYPE
    # 2: the extents of sigma on the source lists ...
    assert call(m=0) == BAD_EXTENT and call(m=64) == BAD_EXTENT and call(na_s=0) == BAD_EXTENT and call(nb_s=BIG) == BAD_EXTENT
    assert call(K=0) == BAD_EXTENT and call(K=-1) == BAD_EXTENT and call(K=1 << 62) == BAD_EXTENT
    assert call(na_s=1 << 20, nb_s=1 << 20, n_t=1) == BAD_EXTENT                        # more than 2^31 - 1 elements of c
    assert call(c_dt=C128, na_s=1 << 15, nb_s=1 << 15, n_t=1, K=1) == BAD_EXTENT        # 2^30 complex elements are 2^31 real columns
    # ... and on the target lists: (n_t, nb_s) for spin 0, (na_s, n_t) for spin 1
    assert call(n_t=0) == BAD_EXTENT and call(n_t=BIG) == BAD_EXTENT and call(spin=1, n_t=0) == BAD_EXTENT
    assert call(spin=0, na_s=1, nb_s=1 << 20, n_t=1 << 20) == BAD_EXTENT and call(spin=1, na_s=1 << 20, nb_s=1, n_t=1 << 20) == BAD_EXTENT
    # 3: d, spin, n_alpha, the bytes of out, the grid
    assert call(d=0) == BAD_EXTENT and call(d=-1) == BAD_EXTENT and call(spin=2) == BAD_EXTENT and call(spin=-1) == BAD_EXTENT
    assert call(n_alpha=-1) == BAD_EXTENT and call(n_alpha=M + 1) == BAD_EXTENT
    assert call(d=1 << 62) == BAD_EXTENT and call(d=1 << 50) == BAD_EXTENT              # d K na_t nb_t elements, their bytes
    # the grid ceil(d / 4) K na_t ntile: 2^28 operators in groups of 4 on 2 x 28 x 1 workgroups are more than 2^31 - 1
    assert call(d=1 << 28) == BAD_EXTENT
    # 4: null pointers
    for name in ("phi", "table", "c", "out"):
        assert call(**{name: None}) == NULL, name
    # 5: alignment
    for name, base in (("phi", PHI), ("table", TABLE), ("c", C), ("out", OUT)):
        assert call(**{name: base + 2}) == MISALIGNED, name
    assert call(c_dt=C128, c=C + 8) == MISALIGNED and call(c_dt=C128, out=OUT + 8) == MISALIGNED
    assert call(h_dt=C128, c_dt=C128, phi=PHI + 8) == MISALIGNED
    assert call(table=TABLE + 4, out=C) == ALIAS                                        # a table entry is 4 bytes
    # 6: out shares a byte with c, phi or the table, down to the last element of either
    for spin, dims in ((0, NT * NB), (1, NA * NT)):
        v_bytes, o_bytes, p_bytes, t_bytes = K * NA * NB * 8, D * K * dims * 8, D * M * 8, NT * M * 4
        assert call(spin=spin, out=C) == ALIAS and call(spin=spin, out=C + v_bytes - 8) == ALIAS and call(spin=spin, out=C - o_bytes + 8) == ALIAS
        assert call(spin=spin, out=PHI) == ALIAS and call(spin=spin, out=PHI + p_bytes - 8) == ALIAS and call(spin=spin, out=PHI - o_bytes + 8) == ALIAS
        assert call(spin=spin, out=TABLE) == ALIAS and call(spin=spin, out=TABLE + t_bytes - 8) == ALIAS
        assert call(spin=spin, out=TABLE - o_bytes + 8) == ALIAS
    # order: dtype, extents, null, alignment, alias
    assert call(h_dt=C128, c_dt=F64, m=0, table=None) == BAD_DTYPE and call(m=0, d=0, table=None) == BAD_EXTENT
    assert call(spin=2, table=None) == BAD_EXTENT and call(n_alpha=-1, c=None) == BAD_EXTENT
    assert call(d=0, table=None) == BAD_EXTENT and call(table=None, c=C + 2) == NULL and call(c=C + 2, out=C) == MISALIGNED


def test_wrappers_are_gpu_only():
    import torch

    from quantum_systems_amd import kernels

    m = 4
    target, source = torch.tensor([1, 2, 4, 8], dtype=torch.int64), torch.tensor([3, 5, 6, 9, 10, 12], dtype=torch.int64)
    with pytest.raises(RuntimeError, match="GPU only"):
        kernels.string_ci_ladder_table(target, source, m)
    table = torch.zeros(4, m, dtype=torch.int32)
    c = torch.zeros(6, 6, dtype=torch.float64)
    phi = torch.zeros(m, dtype=torch.float64)
    for spin in (0, 1):
        with pytest.raises(RuntimeError, match="GPU only"):
            kernels.string_ci_ladder(phi, table, spin, 2, c)
        with pytest.raises(RuntimeError, match="GPU only"):
            kernels.string_ci_ladder(phi[None], table, spin, 2, c[None])
