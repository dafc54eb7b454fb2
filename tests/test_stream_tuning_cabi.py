"""CPU-only check of the stream kernels' tuning key (include/qs_amd.h): ``gemm_stream_wgs`` takes 0 ... 4096;
``qs_tuning_set`` refuses everything else before any HIP call and leaves the value."""

import pytest

BAD_EXTENT = -1


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as entry

    entry.build()
    from quantum_systems_amd import _lib

    return _lib.load()


def test_the_stream_tuning_key(lib):
    try:
        for bad in (-1, 4097, 2**32 + 1, -2**40):
            assert lib.qs_tuning_set(b"gemm_stream_wgs", bad) == BAD_EXTENT, bad
        for ok in (0, 1, 3, 4096, 0):
            assert lib.qs_tuning_set(b"gemm_stream_wgs", ok) == 0, ok
        assert lib.qs_tuning_set(b"gemm_stream", 2) == 0          # (the neighbouring key is another one)
    finally:
        lib.qs_tuning_reset()
    assert lib.qs_abi_version() == 4
