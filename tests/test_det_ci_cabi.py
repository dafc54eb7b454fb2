"""CPU-only checks of the determinant-CI entries (``qs_det_ci_diagonal`` / ``_sigma`` / ``_density1`` /
``_workspace``): the symbols, every refused argument and the order of the refusals (no GPU is touched: the checks run
before any HIP call), the workspace query, the tuning key, and the GPU-only wrappers."""

import pytest

F64, C128 = 0, 1
BAD_EXTENT, NULL, MISALIGNED, WORKSPACE, BAD_DTYPE, ALIAS = -1, -2, -3, -4, -6, -7
NAMES = ("qs_det_ci_workspace", "qs_det_ci_diagonal", "qs_det_ci_sigma", "qs_det_ci_density1")


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
    assert lib.qs_abi_version() == 4


def test_workspace_query(lib):
    q = lib.qs_det_ci_workspace
    for dt in (F64, C128):
        for m, N, dim, K in [(1, 1, 1, 1), (8, 4, 70, 19), (63, 63, 1, 1), (40, 4, 91390, 8), (63, 5, (1 << 31) - 1, 1 << 20)]:
            assert q(dt, dt, m, N, dim, K) == 0
        assert q(dt, dt, 0, 1, 5, 1) == BAD_EXTENT and q(dt, dt, 64, 2, 5, 1) == BAD_EXTENT
        assert q(dt, dt, 8, 0, 5, 1) == BAD_EXTENT and q(dt, dt, 8, 9, 5, 1) == BAD_EXTENT
        assert q(dt, dt, 8, 4, 0, 1) == BAD_EXTENT and q(dt, dt, 8, 4, 1 << 31, 1) == BAD_EXTENT
        assert q(dt, dt, 8, 4, 70, 0) == BAD_EXTENT and q(dt, dt, 8, 4, 70, -3) == BAD_EXTENT
    assert q(F64, C128, 8, 4, 70, 1) == BAD_DTYPE and q(C128, F64, 8, 4, 70, 1) == BAD_DTYPE
    assert q(2, 2, 8, 4, 70, 1) == BAD_DTYPE and q(F64, -1, 8, 4, 70, 1) == BAD_DTYPE
    assert q(F64, C128, 64, 4, 70, 1) == BAD_DTYPE                                    # the dtype pair comes first


# fake, well-separated device addresses: every call below returns before any HIP call is made
HT, UT, DETS, D, C, S, RHO, WORK = (k << 40 for k in range(1, 9))
M, N, DIM, K = 8, 4, 70, 3


def test_sigma_refusals_and_their_order(lib):
    def call(h=F64, c_dt=F64, ht=HT, ut=UT, dets=DETS, D=D, c=C, s=S, m=M, N=N, dim=DIM, K=K, ldc=K, work=None, n=0):
        return lib.qs_det_ci_sigma(h, c_dt, ht, ut, dets, D, c, s, m, N, dim, K, ldc, work, n, None)

    assert call(h=F64, c_dt=C128) == BAD_DTYPE and call(h=C128, c_dt=F64) == BAD_DTYPE
    assert call(h=3, c_dt=3) == BAD_DTYPE and call(c_dt=-1) == BAD_DTYPE
    assert call(m=0) == BAD_EXTENT and call(m=64) == BAD_EXTENT and call(N=0) == BAD_EXTENT and call(N=M + 1) == BAD_EXTENT
    assert call(dim=0) == BAD_EXTENT and call(dim=1 << 31) == BAD_EXTENT and call(dim=-5) == BAD_EXTENT
    assert call(K=0, ldc=1) == BAD_EXTENT and call(K=-1) == BAD_EXTENT and call(ldc=K - 1) == BAD_EXTENT
    for name in ("ht", "ut", "dets", "D", "c", "s"):
        assert call(**{name: None}) == NULL, name
    for name, base in (("ht", HT), ("ut", UT), ("dets", DETS), ("D", D), ("c", C), ("s", S)):
        assert call(**{name: base + 4}) == MISALIGNED, name
    for name, base in (("ht", HT), ("ut", UT), ("c", C), ("s", S)):                     # a complex element is 16 bytes
        assert call(h=C128, c_dt=C128, **{name: base + 8}) == MISALIGNED, name
    # an output that overlaps an input
    assert call(s=HT) == ALIAS and call(s=UT) == ALIAS and call(s=DETS) == ALIAS and call(s=D) == ALIAS and call(s=C) == ALIAS
    assert call(s=HT + 8 * (M * M - 1)) == ALIAS and call(s=UT + 8 * (M ** 4 - 1)) == ALIAS
    assert call(s=DETS + 8 * (DIM - 1)) == ALIAS and call(s=D - 8 * K * DIM + 8) == ALIAS
    assert call(s=C + 8 * (DIM * K - 1)) == ALIAS and call(s=C + 8 * ((DIM - 1) * 5 + K - 1), ldc=5) == ALIAS
    assert call(n=-1) == WORKSPACE                                                      # below the query (0)
    # order: dtype pair, extents, null, alignment, alias, workspace
    assert call(h=3, m=0, ht=None) == BAD_DTYPE
    assert call(m=0, ht=None) == BAD_EXTENT
    assert call(ht=None, ut=UT + 4) == NULL
    assert call(ut=UT + 4, s=HT) == MISALIGNED
    assert call(s=HT, n=-1) == ALIAS


def test_diagonal_refusals_and_their_order(lib):
    def call(h=F64, ht=HT, ut=UT, dets=DETS, D=D, m=M, N=N, dim=DIM):
        return lib.qs_det_ci_diagonal(h, ht, ut, dets, D, m, N, dim, None)

    assert call(h=2) == BAD_DTYPE and call(h=-1) == BAD_DTYPE
    assert call(m=0) == BAD_EXTENT and call(m=64) == BAD_EXTENT and call(N=0) == BAD_EXTENT and call(N=M + 1) == BAD_EXTENT
    assert call(dim=0) == BAD_EXTENT and call(dim=1 << 31) == BAD_EXTENT
    for name in ("ht", "ut", "dets", "D"):
        assert call(**{name: None}) == NULL, name
    for name, base in (("ht", HT), ("ut", UT), ("dets", DETS), ("D", D)):
        assert call(**{name: base + 4}) == MISALIGNED, name
    assert call(h=C128, ht=HT + 8) == MISALIGNED and call(h=C128, ut=UT + 8) == MISALIGNED
    assert call(D=HT) == ALIAS and call(D=UT + 8 * (M ** 4 - 1)) == ALIAS and call(D=DETS - 8 * (DIM - 1)) == ALIAS
    assert call(h=2, m=0, ht=None) == BAD_DTYPE and call(m=0, ht=None) == BAD_EXTENT
    assert call(ht=None, ut=UT + 4) == NULL and call(ut=UT + 4, D=HT) == MISALIGNED


def test_density_refusals_and_their_order(lib):
    def call(c_dt=F64, dets=DETS, c=C, rho=RHO, m=M, N=N, dim=DIM):
        return lib.qs_det_ci_density1(c_dt, dets, c, rho, m, N, dim, None)

    assert call(c_dt=2) == BAD_DTYPE and call(c_dt=-1) == BAD_DTYPE
    assert call(m=0) == BAD_EXTENT and call(m=64) == BAD_EXTENT and call(N=0) == BAD_EXTENT and call(N=M + 1) == BAD_EXTENT
    assert call(dim=0) == BAD_EXTENT and call(dim=1 << 31) == BAD_EXTENT
    for name in ("dets", "c", "rho"):
        assert call(**{name: None}) == NULL, name
    for name, base in (("dets", DETS), ("c", C), ("rho", RHO)):
        assert call(**{name: base + 4}) == MISALIGNED, name
    assert call(c_dt=C128, c=C + 8) == MISALIGNED and call(c_dt=C128, rho=RHO + 8) == MISALIGNED
    assert call(rho=DETS) == ALIAS and call(rho=C + 8 * (DIM - 1)) == ALIAS and call(rho=C - 8 * (M * M - 1)) == ALIAS
    assert call(c_dt=2, m=0, c=None) == BAD_DTYPE and call(m=0, c=None) == BAD_EXTENT
    assert call(c=None, rho=RHO + 4) == NULL and call(rho=DETS + 4) == MISALIGNED


def test_tuning_key_accepts_group_sizes_only(lib):
    from quantum_systems_amd import kernels

    try:
        for good in (0, 1, 2, 4, 8):
            assert lib.qs_tuning_set(b"det_ci_g", good) == 0
        for bad in (-1, 3, 5, 6, 7, 9, 16, 1 << 40):
            assert lib.qs_tuning_set(b"det_ci_g", bad) == BAD_EXTENT
    finally:
        lib.qs_tuning_reset()
    with kernels.tuning(det_ci_g=2):
        pass
    with pytest.raises(Exception):
        with kernels.tuning(det_ci_g=3):
            pass


def test_wrappers_are_gpu_only():
    import torch

    from quantum_systems_amd import kernels

    ht, ut = torch.zeros(4, 4, dtype=torch.float64), torch.zeros(4, 4, 4, 4, dtype=torch.float64)
    dets = torch.tensor([3, 5, 6, 9, 10, 12], dtype=torch.int64)
    with pytest.raises(RuntimeError, match="GPU only"):
        kernels.det_ci_diagonal(ht, ut, dets, 2)
    with pytest.raises(RuntimeError, match="GPU only"):
        kernels.det_ci_sigma(ht, ut, dets, 2, torch.zeros(6, dtype=torch.float64), torch.zeros(2, 6, dtype=torch.float64))
    with pytest.raises(RuntimeError, match="GPU only"):
        kernels.det_ci_density1(dets, torch.zeros(6, dtype=torch.float64), 4, 2)
