"""CPU-only checks of the tuning key ``exchange_lower`` (include/qs_amd.h) -- its range, what a reset restores, where the
route drops the fill (``qs_transform_two_body_exchange_lower_d``) -- and of every refusal of ``qs_matmul_pairs_lower`` that
happens before any HIP call."""

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
    lower, upper = lib.qs_transform_two_body_exchange_lower_d, lib.qs_transform_two_body_exchange_leading_upper
    sizes = (64, 128, 192, 255, 256, 320, 384, 512, 1024)
    try:
        assert lib.qs_tuning_set(b"exchange_lower", -1) == BAD_EXTENT
        assert lib.qs_tuning_set(b"exchange_lower", 3) == BAD_EXTENT
        for value in (0, 1, 2):
            assert lib.qs_tuning_set(b"exchange_lower", value) == 0
            # how the route feeds its d launch is not whether it is taken, nor how it contracts its leading indices
            assert lib.qs_transform_two_body_exchange_wanted(F64, 192, 192) == 1
            assert upper(F64, 192, 192) == 1 and upper(F64, 256, 256) == 1
        # automatic (the default): from 256 orbitals, where the column-triangle pass runs and the launch exists
        assert lib.qs_tuning_reset() == 0
        assert [lower(F64, l, l) for l in sizes] == [0, 0, 0, 0, 1, 0, 1, 1, 1]
        assert lower(F64, 256, 384) == 1 and lower(F64, 320, 384) == 1 and lower(F64, 384, 256) == 0
        assert lower(F64, 192, 256) == 0                                        # below the smallest size measured
        assert lower(F64, 256, 320) == 0 and lower(F64, 272, 384) == 0          # M no multiple of 128, L none of 64
        assert all(lower(C128, l, l) == 0 for l in sizes)
        assert lower(7, 256, 256) == 0 and lower(F64, 0, 256) == 0
        # ... and only while exchange_upper is at its own automatic value: an explicit 2 keeps the fill
        assert lib.qs_tuning_set(b"exchange_upper", 2) == 0
        assert all(lower(F64, l, l) == 0 for l in sizes) and upper(F64, 256, 256) == 1
        assert lib.qs_tuning_set(b"exchange_upper", 0) == 0
        assert all(lower(F64, l, l) == 0 for l in sizes)
        # 2: wherever the pass runs and the launch exists, M < L included
        assert lib.qs_tuning_set(b"exchange_order", 2) == 0 and lib.qs_tuning_set(b"exchange_upper", 2) == 0
        assert lib.qs_tuning_set(b"exchange_lower", 2) == 0
        assert lower(F64, 128, 128) == 1 and lower(F64, 64, 128) == 1 and lower(F64, 256, 128) == 1
        assert lower(F64, 64, 64) == 0 and lower(F64, 128, 64) == 0             # M = 64: no 128-column tile
        assert lower(F64, 48, 64) == 0 and lower(F64, 80, 128) == 0             # the edge forms
        assert upper(F64, 64, 64) == 1 and upper(F64, 80, 128) == 1             # ... keep the pass, with its fill
        assert lower(C128, 128, 128) == 0
        # not without the single d launch over the pairs, nor without the pass, nor in the other order
        assert lib.qs_tuning_set(b"exchange_pairs", 0) == 0
        assert lower(F64, 128, 128) == 0
        assert lib.qs_tuning_set(b"exchange_pairs", 1) == 0 and lower(F64, 128, 128) == 1
        assert lib.qs_tuning_set(b"exchange_order", 0) == 0
        assert lower(F64, 128, 128) == 0 and lower(F64, 256, 256) == 0
        assert lib.qs_tuning_set(b"exchange_order", 2) == 0 and lib.qs_tuning_set(b"exchange_upper", 0) == 0
        assert lower(F64, 128, 128) == 0
        assert lib.qs_tuning_set(b"exchange_upper", 2) == 0 and lib.qs_tuning_set(b"gemm_fast", 0) == 0
        assert lower(F64, 128, 128) == 0                                        # the general kernel fetches no mirror blocks
        assert lib.qs_tuning_set(b"gemm_fast", 1) == 0 and lib.qs_tuning_set(b"exchange_lower", 0) == 0
        assert lower(F64, 128, 128) == 0 and lower(F64, 256, 256) == 0
        # a reset restores 1, not 0 and not 2
        assert lib.qs_tuning_set(b"exchange_lower", 2) == 0 and lower(F64, 128, 128) == 1
        assert lib.qs_tuning_reset() == 0
        assert lower(F64, 128, 128) == 0 and lower(F64, 256, 256) == 1
    finally:
        assert lib.qs_tuning_reset() == 0
    assert lib.qs_abi_version() == 4


def test_matmul_pairs_lower_refuses_before_any_launch(lib):
    fn = lib.qs_matmul_pairs_lower
    A, B, C = 1 << 20, 2 << 20, 3 << 20

    def call(dtype=F64, a=A, b=B, c=C, m=128, n=128, k=None, lda=None, ldb=None, ldc=None, grid=2, sa=None, sb=0, sc=None,
             accumulate=0):
        k = m if k is None else k
        return fn(dtype, a, b, c, m, n, k, k if lda is None else lda, n if ldb is None else ldb, n if ldc is None else ldc,
                  grid, m * k if sa is None else sa, sb, m * n if sc is None else sc, accumulate, None)

    assert call(dtype=7) == BAD_DTYPE
    assert call(a=None) == NULL_POINTER and call(b=None) == NULL_POINTER and call(c=None) == NULL_POINTER
    assert call(a=A + 4) == MISALIGNED and call(b=B + 4) == MISALIGNED and call(c=C + 4) == MISALIGNED
    assert call(sa=-1) == BAD_EXTENT and call(sb=-1) == BAD_EXTENT and call(sc=-1) == BAD_EXTENT
    assert call(grid=0) == BAD_EXTENT and call(grid=-1) == BAD_EXTENT
    assert call(dtype=C128) == BAD_EXTENT                               # complex128: not built
    assert call(accumulate=1) == BAD_EXTENT
    for m in (0, 16, 40, 96, 136):                                      # side a multiple of 16 AND of the row tile
        assert call(m=m) == BAD_EXTENT
    assert call(k=64) == BAD_EXTENT and call(m=64, k=128) == BAD_EXTENT  # m != k
    assert call(lda=130) == BAD_EXTENT and call(lda=64) == BAD_EXTENT   # a side x side entry: lda == side
    assert call(sa=128 * 128 - 2) == BAD_EXTENT and call(sa=0) == BAD_EXTENT      # entries at least side^2 apart
    assert call(n=64) == BAD_EXTENT and call(n=136) == BAD_EXTENT       # whole 128-column tiles
    assert call(ldb=64) == BAD_EXTENT and call(ldc=64) == BAD_EXTENT
    assert call(a=A + 8) == BAD_EXTENT and call(ldc=129) == BAD_EXTENT  # 16-byte items
    try:
        assert lib.qs_tuning_set(b"gemm_fast", 0) == 0                  # the general kernel fetches no mirror blocks
        assert call() == BAD_EXTENT
        assert lib.qs_tuning_reset() == 0
        assert lib.qs_tuning_set(b"gemm_f64_cfg", 1) == 0               # a forced shape of the general kernel
        assert call() == BAD_EXTENT
    finally:
        assert lib.qs_tuning_reset() == 0
    assert lib.qs_last_dispatch() == b""
