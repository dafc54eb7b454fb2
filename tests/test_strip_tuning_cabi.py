"""CPU-only checks of the strip kernels' two tuning keys (include/qs_amd.h): ``gemm_strip_wide`` takes 0, 1, 2 and
``gemm_strip_wgs`` 0 ... 4096; ``qs_tuning_set`` refuses everything else before any HIP call and leaves the value."""

import pytest

BAD_EXTENT = -1


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as entry

    entry.build()
    from quantum_systems_amd import _lib

    return _lib.load()


def test_the_strip_tuning_keys(lib):
    try:
        for bad in (-1, 3, 2**31, -2**40):
            assert lib.qs_tuning_set(b"gemm_strip_wide", bad) == BAD_EXTENT, bad
        for ok in (0, 1, 2, 0):
            assert lib.qs_tuning_set(b"gemm_strip_wide", ok) == 0, ok
        for bad in (-1, 4097, 2**32 + 1, -2**40):
            assert lib.qs_tuning_set(b"gemm_strip_wgs", bad) == BAD_EXTENT, bad
        for ok in (0, 1, 3, 4096, 0):
            assert lib.qs_tuning_set(b"gemm_strip_wgs", ok) == 0, ok
    finally:
        lib.qs_tuning_reset()
    assert lib.qs_abi_version() == 4
