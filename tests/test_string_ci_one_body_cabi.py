"""CPU-only checks of ``qs_string_ci_one_body``: the symbol, every refused argument and the order of the refusals (no GPU
is touched: the checks run before any HIP call), and the GPU-only wrapper."""

import ctypes

import pytest

F64, C128 = 0, 1
BAD_EXTENT, NULL, MISALIGNED, BAD_DTYPE, ALIAS = -1, -2, -3, -6, -7
NAME = "qs_string_ci_one_body"
BIG = (1 << 31) - 1


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as entry

    entry.build()
    from quantum_systems_amd import _lib

    return _lib.load()


def test_symbol_is_exported_and_bound(lib):
    from quantum_systems_amd import _lib

    raw = ctypes.CDLL(_lib.LIB_PATH)
    assert hasattr(raw, NAME) and NAME in _lib.SIGNATURES
    assert lib.qs_abi_version() == 4


# fake, well-separated device addresses: every call below returns before any HIP call is made
AU, AD, TA, TB, C, OUT = (k << 44 for k in range(1, 7))
M, NA, NB, D, K = 8, 70, 56, 3, 2


def test_refusals_and_their_order(lib):
    def call(h_dt=F64, c_dt=F64, au=AU, ad=AD, d=D, ta=TA, tb=TB, m=M, na=NA, nb=NB, c=C, K=K, out=OUT):
        return lib.qs_string_ci_one_body(h_dt, c_dt, au, ad, d, ta, tb, m, na, nb, c, K, out, None)

    # 1: the forms of sigma; a complex A against a real c is refused
    assert call(h_dt=2) == BAD_DTYPE and call(c_dt=-1) == BAD_DTYPE and call(h_dt=C128, c_dt=F64) == BAD_DTYPE
    # 2: extents
    assert call(m=0) == BAD_EXTENT and call(m=64) == BAD_EXTENT and call(na=0) == BAD_EXTENT and call(nb=BIG) == BAD_EXTENT
    assert call(K=0) == BAD_EXTENT and call(K=-1) == BAD_EXTENT and call(K=1 << 62) == BAD_EXTENT
    assert call(na=1 << 20, nb=1 << 20) == BAD_EXTENT                                   # more than 2^31 - 1 elements of c
    assert call(c_dt=C128, na=1 << 15, nb=1 << 15, K=1) == BAD_EXTENT                   # 2^30 complex elements are 2^31 real columns
    assert call(d=0) == BAD_EXTENT and call(d=-1) == BAD_EXTENT
    assert call(d=1 << 62) == BAD_EXTENT and call(d=1 << 50) == BAD_EXTENT              # d K na nb elements, their bytes
    # the grid ceil(d / 4) K na ntile: 2^28 operators in groups of 4 on 2 x 70 x 1 workgroups are more than 2^31 - 1
    assert call(d=1 << 28) == BAD_EXTENT
    # 3: null pointers; A_down may be null
    for name in ("au", "ta", "tb", "c", "out"):
        assert call(**{name: None}) == NULL, name
    # 4: alignment
    for name, base in (("au", AU), ("ad", AD), ("ta", TA), ("tb", TB), ("c", C), ("out", OUT)):
        assert call(**{name: base + 2}) == MISALIGNED, name
    assert call(c_dt=C128, c=C + 8) == MISALIGNED and call(c_dt=C128, out=OUT + 8) == MISALIGNED
    assert call(h_dt=C128, c_dt=C128, au=AU + 8) == MISALIGNED and call(h_dt=C128, c_dt=C128, ad=AD + 8) == MISALIGNED
    assert call(ta=TA + 4, tb=TB + 4, out=C) == ALIAS                                   # a table entry is 4 bytes
    # 5: out shares a byte with c, A_up, A_down or a table
    v_bytes, o_bytes, a_bytes = K * NA * NB * 8, D * K * NA * NB * 8, D * M * M * 8
    assert call(out=C) == ALIAS and call(out=C + v_bytes - 8) == ALIAS and call(out=C - o_bytes + 8) == ALIAS
    for base in (AU, AD):
        assert call(out=base) == ALIAS and call(out=base + a_bytes - 8) == ALIAS and call(out=base - o_bytes + 8) == ALIAS
    assert call(out=TA) == ALIAS and call(out=TB + 4 * NB * M * M - 8) == ALIAS and call(out=TA - o_bytes + 8) == ALIAS
    # the spans are exact: one byte past an input, or an input that ends where out begins, is fine -- such a call would go
    # on to the launch, so it is only made with the next refusal in line
    assert call(out=C + v_bytes, au=None) == NULL and call(out=AU + a_bytes, ta=None) == NULL
    # a null A_down has no bytes, and A_down == A_up is allowed (an input twice)
    assert call(ad=None, out=C) == ALIAS and call(ad=AU, out=AU) == ALIAS
    # order: dtype, extents, null, alignment, alias
    assert call(h_dt=C128, c_dt=F64, m=0, ta=None) == BAD_DTYPE and call(m=0, d=0, ta=None) == BAD_EXTENT
    assert call(d=0, ta=None) == BAD_EXTENT and call(ta=None, c=C + 2) == NULL and call(c=C + 2, out=C) == MISALIGNED
    assert call(ad=AD + 2, out=AD) == MISALIGNED


def test_wrapper_is_gpu_only():
    import torch

    from quantum_systems_amd import kernels

    m = 4
    table = torch.zeros(6, m * m, dtype=torch.int32)
    c = torch.zeros(6, 6, dtype=torch.float64)
    A = torch.zeros(m, m, dtype=torch.float64)
    with pytest.raises(RuntimeError, match="GPU only"):
        kernels.string_ci_one_body(A, table, table, m, c)
    with pytest.raises(RuntimeError, match="GPU only"):
        kernels.string_ci_one_body(A, table, table, m, c, A_down=A)
