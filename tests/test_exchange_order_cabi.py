"""CPU-only checks of the tuning key ``exchange_order`` (include/qs_amd.h) -- its range, that a reset restores the
automatic rule, that it leaves the route's own policy (``qs_transform_two_body_exchange_wanted``) alone, and that the
ABI version did not move -- and of the refusals of ``qs_matmul_pairs_mirrored`` that happen before any HIP call."""

import pytest

BAD_EXTENT = -1
F64, C128 = 0, 1


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as entry

    entry.build()
    from quantum_systems_amd import _lib

    return _lib.load()


def test_the_tuning_key(lib):
    try:
        assert lib.qs_tuning_set(b"exchange_order", -1) == BAD_EXTENT
        assert lib.qs_tuning_set(b"exchange_order", 3) == BAD_EXTENT
        for value in (0, 1, 2):
            assert lib.qs_tuning_set(b"exchange_order", value) == 0
            # which order the route takes is not whether it is taken
            for code, first in ((F64, 192), (C128, 160)):
                assert lib.qs_transform_two_body_exchange_wanted(code, first, first) == 1
                assert lib.qs_transform_two_body_exchange_wanted(code, first - 1, first - 1) == 0
    finally:
        assert lib.qs_tuning_reset() == 0
    assert lib.qs_abi_version() == 4


def test_mirrored_pairs_entry_refuses_before_any_launch(lib):
    """``qs_matmul_pairs_mirrored``: what its kernel cannot do is an error code, decided on the host."""
    NULL_POINTER, BAD_DTYPE = -2, -6

    def call(dtype=F64, A=16, B=16, out=16, m=128, n=128, k=16, lda=16, ldb=128, ldc=128, grid=3, sa=0, sb=16 * 128,
             sc=128 * 128, acc=0):
        return lib.qs_matmul_pairs_mirrored(dtype, A, B, out, m, n, k, lda, ldb, ldc, grid, sa, sb, sc, acc, None)

    assert call(dtype=7) == BAD_DTYPE and call(out=None) == NULL_POINTER
    assert call(grid=0) == BAD_EXTENT and call(sb=-1) == BAD_EXTENT
    assert call(n=256, ldb=256, ldc=256) == BAD_EXTENT           # m != n
    assert call(acc=1) == BAD_EXTENT
    assert call(m=64, n=64, ldb=64, ldc=64) == BAD_EXTENT        # no whole 128 x 128 tiles
    assert call(k=8, lda=8) == BAD_EXTENT                        # no whole k-stage
    assert call(dtype=C128) == BAD_EXTENT                        # complex128: not built
    try:
        assert lib.qs_tuning_set(b"gemm_fast", 0) == 0           # the general kernel has no such epilogue
        assert call() == BAD_EXTENT
    finally:
        lib.qs_tuning_reset()
    assert lib.qs_last_dispatch() == b""
