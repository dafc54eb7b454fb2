"""CPU-only checks of the exchange-symmetry entry points (include/qs_amd.h): argument validation that is refused
before any HIP call, the tuning keys, and the policy ``qs_transform_two_body_exchange_wanted`` -- never at
min(L, M) <= 128, where existing tests pin the plain route's dispatch for symmetric inputs."""

import pytest

BAD_EXTENT, NULL_POINTER, MISALIGNED, WORKSPACE, BAD_DTYPE, ALIAS = -1, -2, -3, -4, -6, -7
F64, C128 = 0, 1


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as entry

    entry.build()
    from quantum_systems_amd import _lib

    return _lib.load()


def test_check_entry_refuses_bad_arguments(lib):
    assert lib.qs_two_body_exchange_symmetric(5, 16, 4, 16, None) == BAD_DTYPE
    assert lib.qs_two_body_exchange_symmetric(F64, 16, 0, 16, None) == BAD_EXTENT
    assert lib.qs_two_body_exchange_symmetric(F64, 16, 5000, 16, None) == BAD_EXTENT
    assert lib.qs_two_body_exchange_symmetric(F64, None, 4, 16, None) == NULL_POINTER
    assert lib.qs_two_body_exchange_symmetric(F64, 16, 4, None, None) == NULL_POINTER
    assert lib.qs_two_body_exchange_symmetric(F64, 12, 4, 16, None) == MISALIGNED
    assert lib.qs_two_body_exchange_symmetric(C128, 24, 4, 16, None) == MISALIGNED
    assert lib.qs_two_body_exchange_symmetric(F64, 16, 4, 18, None) == MISALIGNED


def test_transform_entries_validate_like_the_plain_ones(lib):
    for fn in (lib.qs_transform_two_body_exchange, lib.qs_transform_two_body):
        assert fn(F64, None, None, None, None, None, 0, 4, 4, None) == NULL_POINTER
        assert fn(5, 8, 8, 8, 8, 8, 0, 4, 4, None) == BAD_DTYPE
        assert fn(F64, 8, 8, 8, 16, 32, 0, -1, 4, None) == BAD_EXTENT
        assert fn(F64, 8, 8, 8, 16, 32, 1, 4, 4, None) == WORKSPACE
        assert fn(F64, 8, 8, 8, 8, 32, 1 << 40, 4, 4, None) == ALIAS
        assert fn(F64, 12, 8, 8, 16, 32, 1 << 40, 4, 4, None) == MISALIGNED
    for fn in (lib.qs_transform_two_body_inplace_exchange, lib.qs_transform_two_body_inplace):
        assert fn(F64, None, None, None, None, 0, 4, 4, None) == NULL_POINTER
        assert fn(5, 8, 8, 8, 32, 0, 4, 4, None) == BAD_DTYPE
        assert fn(F64, 8, 8, 8, 32, 1 << 40, 4, 5, None) == BAD_EXTENT          # M > L
        assert fn(F64, 8, 8, 8, 32, 1, 4, 4, None) == WORKSPACE
        assert fn(F64, 32, 8, 8, 32, 1 << 40, 4, 4, None) == ALIAS
        assert fn(F64, 12, 8, 8, 32, 1 << 40, 4, 4, None) == MISALIGNED


def test_mirror_entry_refuses_bad_arguments(lib):
    assert lib.qs_exchange_mirror(7, 16, 4, 4, 1, None) == BAD_DTYPE
    assert lib.qs_exchange_mirror(F64, None, 4, 4, 1, None) == NULL_POINTER
    assert lib.qs_exchange_mirror(F64, 12, 4, 4, 1, None) == MISALIGNED
    for n, m, block in [(0, 4, 1), (4, 0, 1), (4, 4, 0), (4, 4, -2), (5000, 4, 1), (4, 5000, 1)]:
        assert lib.qs_exchange_mirror(F64, 16, n, m, block, None) == BAD_EXTENT


def test_tuning_keys(lib):
    try:
        for bad in (-1, 3):
            assert lib.qs_tuning_set(b"exchange", bad) == BAD_EXTENT
        for key in (b"exchange_block", b"exchange_block_d"):
            assert lib.qs_tuning_set(key, -1) == BAD_EXTENT
            assert lib.qs_tuning_set(key, 4097) == BAD_EXTENT
            assert lib.qs_tuning_set(key, 64) == 0 and lib.qs_tuning_set(key, 0) == 0
        for ok in (0, 1, 2):
            assert lib.qs_tuning_set(b"exchange", ok) == 0
    finally:
        lib.qs_tuning_reset()


def _threshold(lib, dtype):
    """Smallest square size the automatic policy takes."""
    return next((l for l in range(1, 1025) if lib.qs_transform_two_body_exchange_wanted(dtype, l, l)), None)


def test_policy_without_a_gpu(lib):
    wanted = lib.qs_transform_two_body_exchange_wanted
    lib.qs_tuning_reset()
    for dtype in (F64, C128):
        for l in (1, 55, 64, 127, 128):
            assert wanted(dtype, l, l) == 0
            assert wanted(dtype, l, 512) == 0 and wanted(dtype, 512, l) == 0     # min(L, M) decides
        t = _threshold(lib, dtype)
        assert t is not None and 129 <= t <= 256                                # the headline size takes the route
        assert wanted(dtype, t - 1, t - 1) == 0 and wanted(dtype, t, t) == 1
        for l in range(t, 1025, 37):                                             # ... and every size above it
            assert wanted(dtype, l, l) == 1
        assert wanted(dtype, t, t + 40) == 1 and wanted(dtype, t + 40, t) == 1
        assert wanted(dtype, t - 1, t + 40) == 0
    assert wanted(9, 256, 256) == 0 and wanted(F64, 0, 256) == 0 and wanted(F64, 256, 5000) == 0
    try:
        assert lib.qs_tuning_set(b"exchange", 0) == 0
        assert wanted(F64, 256, 256) == 0 and wanted(C128, 512, 512) == 0
        assert lib.qs_tuning_set(b"exchange", 2) == 0
        for l in (1, 5, 33, 128, 129, 256):
            assert wanted(F64, l, l) == 1 and wanted(C128, l, 7) == 1
        assert wanted(F64, 2048, 8) == 0                                         # the check's grid does not fit 31 bits
    finally:
        lib.qs_tuning_reset()
    assert wanted(F64, 128, 128) == 0 and wanted(F64, 256, 256) == 1
