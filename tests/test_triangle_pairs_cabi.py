"""CPU-only checks of the triangular batch's host side (include/qs_amd.h): ``qs_triangle_pair`` -- the ONE remap
pair number -> (i, j >= i) that the product kernels and the check kernel share (csrc/qs_triangle.h) -- against a plain
Python enumeration, and the refusals of ``qs_matmul_pairs`` that happen before any HIP call."""

import ctypes

import pytest

BAD_EXTENT, NULL_POINTER, MISALIGNED, BAD_DTYPE = -1, -2, -3, -6
F64, C128 = 0, 1


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as entry

    entry.build()
    from quantum_systems_amd import _lib

    return _lib.load()


def _pair(lib, n, t):
    i, j = ctypes.c_int64(-1), ctypes.c_int64(-1)
    assert lib.qs_triangle_pair(n, t, ctypes.byref(i), ctypes.byref(j)) == 0, (n, t)
    return i.value, j.value


def test_every_pair_of_every_grid_up_to_130(lib):
    for n in range(1, 131):
        want = [(i, j) for i in range(n) for j in range(i, n)]
        got = [_pair(lib, n, t) for t in range(len(want))]
        assert got == want, n


@pytest.mark.parametrize("n", [1000, 4096])
def test_first_and_last_pair_of_every_row_of_a_large_grid(lib, n):
    start = 0
    for i in range(n):
        assert _pair(lib, n, start) == (i, i), (n, i)
        assert _pair(lib, n, start + n - i - 1) == (i, n - 1), (n, i)
        start += n - i
    assert start == n * (n + 1) // 2


def _strict_pair(lib, l, t):
    """(r, s), r < s, of packed position t by the identity that csrc/qs_pair_walk.h's pair_unpack<false> rests on: the
    triangle WITH its diagonal of n = l - 1, its second index shifted by one.  The shift is redone HERE, on top of
    ``qs_triangle_pair``: this pins the identity and ``triangle_row`` at n = l - 1, not the C++ line itself (that one
    runs under the GPU parity tests only)."""
    r, j = _pair(lib, l - 1, t)
    return r, j + 1


def test_the_strict_triangle_is_the_triangle_of_l_minus_1_shifted(lib):
    for l in range(2, 41):
        want = [(r, s) for r in range(l) for s in range(r + 1, l)]
        got = [_strict_pair(lib, l, t) for t in range(len(want))]
        assert got == want, l
    l, start = 4096, 0
    for r in range(l - 1):                                   # run r: (r, r + 1) ... (r, l - 1)
        assert _strict_pair(lib, l, start) == (r, r + 1), r
        assert _strict_pair(lib, l, start + l - r - 2) == (r, l - 1), r
        start += l - r - 1
    assert start == l * (l - 1) // 2


def test_pair_refuses_bad_arguments(lib):
    i, j = ctypes.c_int64(7), ctypes.c_int64(7)
    ri, rj = ctypes.byref(i), ctypes.byref(j)
    for n, t in [(0, 0), (-3, 0), (5, -1), (5, 15), (1, 1), (4096, 4096 * 4097 // 2)]:
        assert lib.qs_triangle_pair(n, t, ri, rj) == BAD_EXTENT, (n, t)
    assert (i.value, j.value) == (7, 7)                      # a refusal writes nothing
    assert lib.qs_triangle_pair(5, 14, ri, rj) == 0 and (i.value, j.value) == (4, 4)
    assert lib.qs_triangle_pair(5, 0, None, rj) == NULL_POINTER
    assert lib.qs_triangle_pair(5, 0, ri, None) == NULL_POINTER


def test_matmul_pairs_refuses_before_any_hip_call(lib):
    def call(dtype=F64, A=16, B=16, out=16, grid_n=3, sa=0, sb=16, sc=16):
        return lib.qs_matmul_pairs(dtype, A, B, out, 4, 4, 4, 4, 4, 4, grid_n, sa, sb, sc, 0, None)

    assert call(dtype=5) == BAD_DTYPE and call(dtype=-1) == BAD_DTYPE
    assert call(A=None) == NULL_POINTER and call(B=None) == NULL_POINTER and call(out=None) == NULL_POINTER
    assert call(A=12) == MISALIGNED and call(dtype=C128, B=24) == MISALIGNED
    assert call(grid_n=0) == BAD_EXTENT and call(grid_n=-2) == BAD_EXTENT
    assert call(sa=-1) == BAD_EXTENT and call(sb=-1) == BAD_EXTENT and call(sc=-1) == BAD_EXTENT
    # extents are the product's own: refused by the dispatch's validation, still before a launch
    assert lib.qs_matmul_pairs(F64, 16, 16, 16, 0, 4, 4, 4, 4, 4, 3, 0, 16, 16, 0, None) == BAD_EXTENT
    assert lib.qs_matmul_pairs(F64, 16, 16, 16, 4, 4, 4, 3, 4, 4, 3, 0, 16, 16, 0, None) == BAD_EXTENT     # lda < k


def test_the_tuning_key(lib):
    try:
        assert lib.qs_tuning_set(b"exchange_pairs", -1) == BAD_EXTENT
        assert lib.qs_tuning_set(b"exchange_pairs", 2) == BAD_EXTENT
        assert lib.qs_tuning_set(b"exchange_pairs", 0) == 0 and lib.qs_tuning_set(b"exchange_pairs", 1) == 0
    finally:
        lib.qs_tuning_reset()
    assert lib.qs_abi_version() == 4
