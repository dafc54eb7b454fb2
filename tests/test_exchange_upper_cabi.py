"""CPU-only checks of the tuning key ``exchange_upper`` (include/qs_amd.h) -- its range, what a reset restores, where the
column-triangle form applies (``qs_transform_two_body_exchange_leading_upper``) -- and of every refusal of the two new
entries ``qs_matmul_upper`` / ``qs_exchange_mirror_lower`` that happens before any HIP call."""

import pytest

BAD_EXTENT, NULL_POINTER, MISALIGNED, BAD_DTYPE = -1, -2, -3, -6
F64, C128 = 0, 1


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as entry

    entry.build()
    from quantum_systems_amd import _lib

    return _lib.load()


def test_the_tuning_key_and_its_reset(lib):
    upper, on_pairs = lib.qs_transform_two_body_exchange_leading_upper, lib.qs_transform_two_body_exchange_leading_pairs
    sizes = (24, 64, 128, 160, 191, 192, 256, 320, 512, 1024)
    try:
        assert lib.qs_tuning_set(b"exchange_upper", -1) == BAD_EXTENT
        assert lib.qs_tuning_set(b"exchange_upper", 3) == BAD_EXTENT
        for value in (0, 1, 2):
            assert lib.qs_tuning_set(b"exchange_upper", value) == 0
            # how the route contracts its leading indices is not whether it is taken
            assert lib.qs_transform_two_body_exchange_wanted(F64, 192, 192) == 1
            assert lib.qs_transform_two_body_exchange_wanted(F64, 191, 191) == 0
        # automatic (the default): never below the route's own threshold, whatever the order
        assert lib.qs_tuning_set(b"exchange_upper", 1) == 0
        for order in (1, 2):
            assert lib.qs_tuning_set(b"exchange_order", order) == 0
            for l in (16, 64, 128, 176):
                assert upper(F64, l, l) == 0
        assert lib.qs_tuning_set(b"exchange_order", 2) == 0
        assert upper(F64, 128, 192) == 0 and upper(F64, 192, 128) == 0          # min(L, M) decides
        # ... from there on wherever M >= L and the product takes both shapes, and the pairs step aside
        for l in (192, 256, 320, 512):
            assert upper(F64, l, l) == 1 and on_pairs(F64, l, l) == 0
        assert upper(F64, 192, 256) == 1 and upper(F64, 208, 256) == 1 and upper(F64, 191, 256) == 0
        assert upper(F64, 256, 192) == 0 and upper(F64, 224, 224) == 0 and upper(F64, 240, 240) == 0
        assert on_pairs(F64, 240, 240) == 1                                     # M no multiple of 64: today's route
        # ... never for complex128, nor for M no multiple of 64 or L no multiple of 16, at any key value
        for value in (1, 2):
            assert lib.qs_tuning_set(b"exchange_upper", value) == 0
            for l in sizes:
                assert upper(C128, l, l) == 0
            assert upper(F64, 256, 200) == 0 and upper(F64, 256, 288) == 0 and upper(F64, 200, 256) == 0
            assert upper(F64, 0, 64) == 0 and upper(7, 64, 64) == 0
        # 2: wherever the product takes both shapes, M < L included, inside the leading-first order only
        assert lib.qs_tuning_set(b"exchange_upper", 2) == 0
        assert upper(F64, 64, 64) == 1 and upper(F64, 48, 64) == 1 and upper(F64, 128, 64) == 1 and upper(F64, 256, 256) == 1
        assert on_pairs(F64, 64, 64) == 0 and on_pairs(F64, 256, 256) == 0     # the other form answers 0 where this takes over
        assert lib.qs_tuning_set(b"exchange_leading", 2) == 0
        assert upper(F64, 64, 64) == 1 and on_pairs(F64, 64, 64) == 0
        assert on_pairs(F64, 40, 64) == 1 and upper(F64, 40, 64) == 0          # refused here: the pairs as before
        assert lib.qs_tuning_set(b"exchange_order", 0) == 0
        assert upper(F64, 64, 64) == 0 and upper(F64, 256, 256) == 0
        assert lib.qs_tuning_set(b"exchange_order", 2) == 0
        assert lib.qs_tuning_set(b"exchange_upper", 0) == 0
        assert all(upper(F64, l, l) == 0 for l in sizes)
        assert on_pairs(F64, 64, 64) == 1
        # automatic steps aside while exchange_leading is 0 or 2: exactly those launches
        assert lib.qs_tuning_set(b"exchange_upper", 1) == 0
        for leading in (0, 2):
            assert lib.qs_tuning_set(b"exchange_leading", leading) == 0
            assert all(upper(F64, l, l) == 0 for l in sizes)
        # a reset restores 1, not 0 and not 2
        assert lib.qs_tuning_set(b"exchange_order", 2) == 0 and lib.qs_tuning_set(b"exchange_upper", 2) == 0
        assert upper(F64, 64, 64) == 1
        assert lib.qs_tuning_reset() == 0
        after_reset = [upper(F64, l, l) for l in sizes]
        assert after_reset[0] == 0 and after_reset[1] == 0                      # (2 would say 1 at 64 orbitals under order 2)
        assert after_reset == [0, 0, 0, 0, 0, 1, 1, 1, 1, 1]
        assert lib.qs_tuning_set(b"exchange_upper", 1) == 0
        assert [upper(F64, l, l) for l in sizes] == after_reset
        # the segment length of the product's tiles
        for value in (-1, 8, 24, 64):
            assert lib.qs_tuning_set(b"gemm_upper_s", value) == BAD_EXTENT
        for value in (0, 16, 32):
            assert lib.qs_tuning_set(b"gemm_upper_s", value) == 0
        assert lib.qs_tuning_set(b"exchange_order", 2) == 0 and lib.qs_tuning_set(b"exchange_upper", 2) == 0
        assert upper(F64, 48, 64) == 0 and upper(F64, 64, 64) == 1              # S = 32: L a multiple of 32
    finally:
        assert lib.qs_tuning_reset() == 0
    assert lib.qs_abi_version() == 4


def test_matmul_upper_refuses_before_any_launch(lib):
    fn = lib.qs_matmul_upper
    A, B, C = 1 << 20, 2 << 20, 3 << 20

    def call(dtype=F64, a=A, b=B, c=C, m=64, side=32, stack=1, k=16, lda=None, ldb=None, ldc=None, batch=1,
             sa=0, sb=0, sc=0, accumulate=0):
        n = stack * side * side if side > 0 and stack > 0 else 1
        return fn(dtype, a, b, c, m, side, stack, k, k if lda is None else lda, n if ldb is None else ldb,
                  n if ldc is None else ldc, batch, sa, sb, sc, accumulate, None)

    assert call(dtype=7) == BAD_DTYPE
    assert call(a=None) == NULL_POINTER and call(b=None) == NULL_POINTER and call(c=None) == NULL_POINTER
    assert call(a=A + 4) == MISALIGNED and call(b=B + 4) == MISALIGNED and call(c=C + 4) == MISALIGNED
    assert call(sa=-1) == BAD_EXTENT and call(sb=-1) == BAD_EXTENT and call(sc=-1) == BAD_EXTENT
    for side in (0, -16, 24, 40, 65536):
        assert call(side=side) == BAD_EXTENT
    assert call(stack=0) == BAD_EXTENT and call(stack=-1) == BAD_EXTENT
    assert call(side=4096, stack=128) == BAD_EXTENT                     # n past 31 bits
    assert call(dtype=C128) == BAD_EXTENT                               # complex128: not built
    assert call(accumulate=1) == BAD_EXTENT
    assert call(m=96) == BAD_EXTENT and call(m=0) == BAD_EXTENT and call(m=32) == BAD_EXTENT
    assert call(k=24) == BAD_EXTENT and call(k=0) == BAD_EXTENT
    assert call(batch=0) == BAD_EXTENT
    assert call(lda=8) == BAD_EXTENT and call(ldb=1000) == BAD_EXTENT and call(ldc=1000) == BAD_EXTENT
    try:
        assert lib.qs_tuning_set(b"gemm_upper_s", 32) == 0
        assert call(side=48) == BAD_EXTENT                              # a multiple of 16, not of 32
        assert lib.qs_tuning_reset() == 0
        assert lib.qs_tuning_set(b"gemm_fast", 0) == 0                  # the general kernel walks no column triangle
        assert call() == BAD_EXTENT
    finally:
        assert lib.qs_tuning_reset() == 0
    assert lib.qs_last_dispatch() == b""


def test_mirror_lower_refuses_before_any_launch(lib):
    fn = lib.qs_exchange_mirror_lower
    assert fn(7, 1 << 20, 4, 6, None) == BAD_DTYPE
    assert fn(C128, 1 << 20, 4, 6, None) == BAD_DTYPE                    # float64 only
    for n, m in [(0, 6), (4, 0), (-1, 6), (4, -1), (4097, 6), (4, 4097)]:
        assert fn(F64, 1 << 20, n, m, None) == BAD_EXTENT
    assert fn(F64, 1 << 20, 4096, 4096, None) == BAD_EXTENT              # a grid of 2^31 workgroups or more
    assert fn(F64, None, 4, 6, None) == NULL_POINTER
    assert fn(F64, (1 << 20) + 4, 4, 6, None) == MISALIGNED
    assert lib.qs_last_dispatch() == b""
