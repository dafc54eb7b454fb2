"""CPU-only checks of ``qs_det_ci_transition_density1`` and ``qs_det_ci_density2``: the symbols, every refused argument
and the order of the refusals (dtype, extents, null, alignment, alias -- all before any HIP call, so no GPU is touched),
``bra == ket`` accepted as far as these checks go, and the GPU-only wrappers.  Follows tests/test_det_ci_cabi.py."""

import pytest

F64, C128 = 0, 1
BAD_EXTENT, NULL, MISALIGNED, BAD_DTYPE, ALIAS = -1, -2, -3, -6, -7
NAMES = ("qs_det_ci_transition_density1", "qs_det_ci_density2")
# fake, well-separated device addresses: every call below returns before any HIP call is made
DETS, BRA, KET, OUT = (k << 40 for k in range(1, 5))
M, N, DIM = 8, 4, 70
OUT_ELEMS = {"qs_det_ci_transition_density1": M * M, "qs_det_ci_density2": M ** 4}


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as entry

    entry.build()
    from quantum_systems_amd import _lib

    return _lib.load()


def test_symbols_are_exported_and_bound(lib):
    import ctypes

    from quantum_systems_amd import _lib

    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name in NAMES:
        assert hasattr(raw, name) and name in _lib.SIGNATURES
    assert _lib.SIGNATURES[NAMES[0]] == _lib.SIGNATURES[NAMES[1]]
    assert lib.qs_abi_version() == 4


@pytest.mark.parametrize("name", NAMES)
def test_refusals_and_their_order(lib, name):
    entry, n_out = getattr(lib, name), OUT_ELEMS[name]

    def call(c_dt=F64, dets=DETS, bra=BRA, ket=KET, out=OUT, m=M, N=N, dim=DIM):
        return entry(c_dt, dets, bra, ket, out, m, N, dim, None)

    assert call(c_dt=2) == BAD_DTYPE and call(c_dt=-1) == BAD_DTYPE
    assert call(m=0) == BAD_EXTENT and call(m=64) == BAD_EXTENT and call(N=0) == BAD_EXTENT and call(N=M + 1) == BAD_EXTENT
    assert call(dim=0) == BAD_EXTENT and call(dim=1 << 31) == BAD_EXTENT and call(dim=-5) == BAD_EXTENT
    for arg in ("dets", "bra", "ket", "out"):
        assert call(**{arg: None}) == NULL, arg
    for arg, base in (("dets", DETS), ("bra", BRA), ("ket", KET), ("out", OUT)):
        assert call(**{arg: base + 4}) == MISALIGNED, arg
    for arg, base in (("bra", BRA), ("ket", KET), ("out", OUT)):                       # a complex element is 16 bytes
        assert call(c_dt=C128, **{arg: base + 8}) == MISALIGNED, arg
    # the output against each input, at both ends of both
    assert call(out=DETS) == ALIAS and call(out=BRA) == ALIAS and call(out=KET) == ALIAS
    assert call(out=DETS + 8 * (DIM - 1)) == ALIAS and call(out=BRA + 8 * (DIM - 1)) == ALIAS
    assert call(out=KET + 8 * (DIM - 1)) == ALIAS and call(out=KET - 8 * (n_out - 1)) == ALIAS
    assert call(out=BRA - 8 * (n_out - 1)) == ALIAS and call(out=DETS - 8 * (n_out - 1)) == ALIAS
    assert call(c_dt=C128, out=KET + 16 * (DIM - 1)) == ALIAS and call(c_dt=C128, out=BRA - 16 * (n_out - 1)) == ALIAS
    assert call(bra=BRA, ket=BRA, out=BRA) == ALIAS
    # order: dtype, extents, null, alignment, alias
    assert call(c_dt=2, m=0, bra=None) == BAD_DTYPE
    assert call(m=0, bra=None) == BAD_EXTENT
    assert call(ket=None, out=OUT + 4) == NULL
    assert call(out=DETS + 4) == MISALIGNED and call(bra=BRA + 4, out=KET) == MISALIGNED


@pytest.mark.parametrize("name", NAMES)
def test_bra_equal_to_ket_is_not_refused(lib, name):
    """No check compares ``bra`` with ``ket``: with equal pointers the answers are those of distinct ones, and only the
    output is held against the inputs.  (A call that passes every check would launch; the GPU tests make that call.)"""
    entry = getattr(lib, name)
    for dt in (F64, C128):
        assert entry(dt, None, BRA, BRA, OUT, M, N, DIM, None) == NULL
        assert entry(dt, DETS, BRA, BRA, BRA, M, N, DIM, None) == ALIAS                # only the output may not overlap
        assert entry(dt, DETS, BRA, BRA, OUT + 4, M, N, DIM, None) == MISALIGNED
    # one particle is legal for the two-body density as well: the extents pass and the next check answers
    assert entry(F64, DETS, BRA, BRA, None, M, 1, M, None) == NULL


def test_wrappers_are_gpu_only():
    import torch

    from quantum_systems_amd import kernels

    dets = torch.tensor([3, 5, 6, 9, 10, 12], dtype=torch.int64)
    c = torch.zeros(6, dtype=torch.float64)
    with pytest.raises(RuntimeError, match="GPU only"):
        kernels.det_ci_transition_density1(dets, c, c, 4, 2)
    with pytest.raises(RuntimeError, match="GPU only"):
        kernels.det_ci_density2(dets, c, c.clone(), 4, 2)
    with pytest.raises(ValueError):
        kernels.det_ci_density2(dets.to(torch.int32), c, c, 4, 2)
