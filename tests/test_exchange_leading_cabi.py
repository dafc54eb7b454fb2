"""CPU-only checks of the tuning key ``exchange_leading`` (include/qs_amd.h) -- its range, what a reset restores, where
key value 2 applies (``qs_transform_two_body_exchange_leading_pairs``: M >= L inside the leading-first order only) -- and
of every refusal of the two pair movers ``qs_exchange_pair_transpose`` / ``qs_exchange_pair_transpose_back`` that happens
before any HIP call."""

import pytest

BAD_EXTENT, NULL_POINTER, MISALIGNED, BAD_DTYPE, ALIAS = -1, -2, -3, -6, -7
F64, C128 = 0, 1


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as entry

    entry.build()
    from quantum_systems_amd import _lib

    return _lib.load()


def test_the_tuning_key_and_its_reset(lib):
    on_pairs = lib.qs_transform_two_body_exchange_leading_pairs
    try:
        assert lib.qs_tuning_set(b"exchange_leading", -1) == BAD_EXTENT
        assert lib.qs_tuning_set(b"exchange_leading", 3) == BAD_EXTENT
        for value in (0, 1, 2):
            assert lib.qs_tuning_set(b"exchange_leading", value) == 0
            # how the route contracts its leading indices is not whether it is taken
            for code, first in ((F64, 192), (C128, 160)):
                assert lib.qs_transform_two_body_exchange_wanted(code, first, first) == 1
                assert lib.qs_transform_two_body_exchange_wanted(code, first - 1, first - 1) == 0
        assert lib.qs_tuning_set(b"exchange_order", 2) == 0
        for code in (F64, C128):
            assert lib.qs_tuning_set(b"exchange_leading", 2) == 0
            assert on_pairs(code, 24, 24) == 1 and on_pairs(code, 12, 20) == 1
            assert on_pairs(code, 20, 12) == 0                       # M < L: the blocks
            assert on_pairs(code, 0, 24) == 0 and on_pairs(7, 24, 24) == 0
            assert lib.qs_tuning_set(b"exchange_leading", 0) == 0
            assert on_pairs(code, 24, 24) == 0 and on_pairs(code, 1024, 1024) == 0
            # automatic: never below the route's own thresholds, never for M < L
            assert lib.qs_tuning_set(b"exchange_leading", 1) == 0
            for l in (5, 24, 128, 159):
                assert on_pairs(code, l, l) == 0
            assert on_pairs(code, 1024, 512) == 0
        # only inside the leading-first order
        assert lib.qs_tuning_set(b"exchange_leading", 2) == 0 and lib.qs_tuning_set(b"exchange_order", 0) == 0
        assert on_pairs(F64, 24, 24) == 0 and on_pairs(F64, 256, 256) == 0
        # a reset restores 1, not 0 and not 2: what the automatic rule answers is what a fresh key value 1 answers
        assert lib.qs_tuning_set(b"exchange_order", 2) == 0 and lib.qs_tuning_set(b"exchange_leading", 2) == 0
        assert on_pairs(F64, 24, 24) == 1
        assert lib.qs_tuning_reset() == 0
        after_reset = [on_pairs(code, l, l) for code in (F64, C128) for l in (24, 160, 192, 224, 256, 512, 1024)]
        assert after_reset[0] == 0 and after_reset[7] == 0           # (2 would say 1 at 24 orbitals under any order)
        assert lib.qs_tuning_set(b"exchange_leading", 1) == 0
        assert [on_pairs(code, l, l) for code in (F64, C128) for l in (24, 160, 192, 224, 256, 512, 1024)] == after_reset
    finally:
        assert lib.qs_tuning_reset() == 0
    assert lib.qs_abi_version() == 4


def test_pair_transpose_refuses_before_any_launch(lib):
    fn = lib.qs_exchange_pair_transpose
    n = 4**4 * 8
    assert fn(7, 1 << 20, 2 << 20, 4, None) == BAD_DTYPE
    for L in (0, -3, 4097, 5000):
        assert fn(F64, 1 << 20, 2 << 20, L, None) == BAD_EXTENT
    assert fn(F64, 1 << 20, 1 << 40, 2048, None) == BAD_EXTENT          # a grid of 2^31 workgroups or more
    assert fn(F64, None, 2 << 20, 4, None) == NULL_POINTER
    assert fn(F64, 1 << 20, None, 4, None) == NULL_POINTER
    assert fn(F64, (1 << 20) + 4, 2 << 20, 4, None) == MISALIGNED
    assert fn(F64, 1 << 20, (2 << 20) + 4, 4, None) == MISALIGNED
    assert fn(C128, (1 << 20) + 8, 2 << 20, 4, None) == MISALIGNED
    assert fn(C128, 1 << 20, (2 << 20) + 8, 4, None) == MISALIGNED
    assert fn(F64, 1 << 20, 1 << 20, 4, None) == ALIAS
    assert fn(F64, 1 << 20, (1 << 20) + n - 8, 4, None) == ALIAS        # the last element of src is the first of dst
    assert fn(F64, (1 << 20) + n - 8, 1 << 20, 4, None) == ALIAS
    assert lib.qs_last_dispatch() == b""


def test_pair_transpose_back_refuses_before_any_launch(lib):
    fn = lib.qs_exchange_pair_transpose_back
    n = 4 * 4 * 6 * 6 * 8
    assert fn(7, 1 << 20, 2 << 20, 4, 6, None) == BAD_DTYPE
    for L, M in [(0, 6), (4, 0), (-1, 6), (4, -1), (4097, 6), (4, 4097)]:
        assert fn(F64, 1 << 20, 2 << 20, L, M, None) == BAD_EXTENT
    assert fn(F64, 1 << 20, 1 << 40, 2048, 2048, None) == BAD_EXTENT    # a grid of 2^31 workgroups or more
    assert fn(F64, None, 2 << 20, 4, 6, None) == NULL_POINTER
    assert fn(F64, 1 << 20, None, 4, 6, None) == NULL_POINTER
    assert fn(F64, (1 << 20) + 4, 2 << 20, 4, 6, None) == MISALIGNED
    assert fn(F64, 1 << 20, (2 << 20) + 4, 4, 6, None) == MISALIGNED
    assert fn(C128, (1 << 20) + 8, 2 << 20, 4, 6, None) == MISALIGNED
    assert fn(C128, 1 << 20, (2 << 20) + 8, 4, 6, None) == MISALIGNED
    assert fn(F64, 1 << 20, 1 << 20, 4, 6, None) == ALIAS
    assert fn(F64, 1 << 20, (1 << 20) + n - 8, 4, 6, None) == ALIAS
    assert fn(F64, (1 << 20) + n - 8, 1 << 20, 4, 6, None) == ALIAS
    assert lib.qs_last_dispatch() == b""
