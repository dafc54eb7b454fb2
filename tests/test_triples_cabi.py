"""CPU-only checks of the triples entry points (``qs_triples_energy`` / ``_workspace`` / ``_tile`` / ``_budget``): the
symbols, the workspace query, the budget and its tuning key, every refused argument (no GPU is touched: the checks run
before any HIP call), and the Python wrapper's own refusals."""

import ctypes

import pytest

F64, C128 = 0, 1
NAMES = ("qs_triples_energy", "qs_triples_energy_workspace", "qs_triples_energy_tile", "qs_triples_energy_budget")


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as entry

    entry.build()
    from quantum_systems_amd import _lib

    return _lib.load()


def sets(v, tile):
    nt = -(-v // tile)
    return nt * (nt + 1) * (nt + 2) // 6


def test_symbols_are_exported_and_bound(lib):
    import __graft_entry__ as entry
    from quantum_systems_amd import _lib

    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name in NAMES:
        assert hasattr(raw, name) and name in _lib.SIGNATURES
    assert lib.qs_abi_version() == 4
    assert "qs_triples.hip" in entry.SOURCES


def test_tile_and_workspace_query(lib):
    tile = {F64: lib.qs_triples_energy_tile(F64), C128: lib.qs_triples_energy_tile(C128)}
    # 36 tiles of T^3 elements inside the 160 KiB of a CU, and the largest such T
    for code, es in ((F64, 8), (C128, 16)):
        assert 36 * tile[code] ** 3 * es <= 160 * 1024 < 36 * (tile[code] + 1) ** 3 * es
    assert lib.qs_triples_energy_tile(2) == -6 and lib.qs_triples_energy_tile(-1) == -6
    q = lib.qs_triples_energy_workspace
    for code in (F64, C128):
        for v in (1, 5, tile[code], tile[code] + 1, 2 * tile[code] + 1, 250, 4096):
            for n in (1, 3, 40):
                assert q(code, v, n) == 8 * n * sets(v, tile[code])           # one partial per (triple, tile set)
    assert q(7, 4, 4) == -6 and q(-1, 4, 4) == -6
    assert q(F64, 0, 4) == -1 and q(F64, -3, 4) == -1 and q(F64, 4, 0) == -1 and q(F64, 4, -1) == -1
    assert q(F64, 4097, 1) == -1
    most = (2 ** 31 - 1) // sets(4096, tile[F64])                            # one workgroup per (triple, tile set)
    assert q(F64, 4096, most) > 0 and q(F64, 4096, most + 1) == -1


def test_budget_follows_the_tuning_key(lib):
    from quantum_systems_amd import kernels

    assert kernels.triples_budget() == kernels.TRIPLES_BYTES
    assert lib.qs_triples_energy_budget(12345) == 12345 and lib.qs_triples_energy_budget(-1) == -1
    try:
        assert lib.qs_tuning_set(b"triples_bytes", 4096) == 0
        assert kernels.triples_budget() == 4096 and lib.qs_triples_energy_budget(12345) == 4096
        assert lib.qs_tuning_set(b"triples_bytes", 0) == 0                   # 0 = the shipped value again
        assert kernels.triples_budget() == kernels.TRIPLES_BYTES
        assert lib.qs_tuning_set(b"triples_bytes", -1) == -1
        with kernels.tuning(triples_bytes=1 << 20):
            assert kernels.triples_budget() == 1 << 20
        assert kernels.triples_budget() == kernels.TRIPLES_BYTES
    finally:
        lib.qs_tuning_reset()


def test_refused_arguments_without_gpu(lib):
    # fake, well-separated device addresses: every call below returns before any HIP call is made
    X, S, EO, EV, E, W = (x << 40 for x in range(1, 7))
    v, n, nblocks = 9, 4, 24

    def call(dtype=F64, x=X, nblocks=nblocks, slots=S, eo3=EO, ev=EV, v=v, n=n, e=E, work=W, nbytes=None):
        if nbytes is None:
            nbytes = max(lib.qs_triples_energy_workspace(F64, v, n), 0)
        return lib.qs_triples_energy(dtype, x, nblocks, slots, eo3, ev, v, n, e, work, nbytes, None)

    for name in ("x", "slots", "eo3", "ev", "e", "work"):
        assert call(**{name: None}) == -2, name
    assert call(dtype=2) == -6 and call(dtype=-1) == -6
    assert call(v=0) == -1 and call(v=-2) == -1 and call(v=4097) == -1
    assert call(n=0) == -1 and call(n=-1) == -1 and call(n=1 << 31) == -1
    assert call(nblocks=0) == -1 and call(nblocks=-3) == -1 and call(nblocks=1 << 31) == -1
    assert call(v=4096, nblocks=(1 << 63) // (4096 ** 3 * 8) + 1, nbytes=1 << 50) == -1   # the bytes of X past int64
    assert call(dtype=9, x=None) == -6 and call(v=0, x=None) == -1           # order: dtype, extents, null
    assert call(x=X + 4) == -3 and call(slots=S + 2) == -3 and call(eo3=EO + 4) == -3 and call(ev=EV + 4) == -3
    assert call(e=E + 4) == -3 and call(work=W + 4) == -3
    assert call(dtype=C128, x=X + 8) == -3                                   # a complex element is 16 bytes
    need = lib.qs_triples_energy_workspace(F64, v, n)
    assert call(nbytes=need - 1) == -4 and call(nbytes=0) == -4
    assert call(x=X + 4, nbytes=0) == -3                                     # alignment is reported before the size
    assert call(e=X + 8 * v ** 3) == -7 and call(e=W + 8) == -7 and call(work=X) == -7     # e in X, e in work, work in X
    assert call(e=EO) == -7 and call(e=EV + 8) == -7 and call(e=S + 16) == -7


def test_wrapper_refuses_without_gpu():
    import torch

    from quantum_systems_amd import kernels

    X = torch.zeros(6, 3, 3, 3, dtype=torch.float64)
    slots = torch.zeros((2, 6), dtype=torch.int32)
    eo3, ev = torch.zeros(2, dtype=torch.float64), torch.zeros(3, dtype=torch.float64)
    with pytest.raises(RuntimeError, match="GPU only"):
        kernels.triples_energy(X, slots, eo3, ev)
    with pytest.raises(TypeError):
        kernels.triples_energy(X.float(), slots, eo3, ev)
    with pytest.raises(ValueError, match="nblocks, v, v, v"):
        kernels.triples_energy(X[:, :, :2], slots, eo3, ev)
    with pytest.raises(ValueError, match="slots"):
        kernels.triples_energy(X, slots.long(), eo3, ev)
    with pytest.raises(ValueError, match="slots"):
        kernels.triples_energy(X, slots[:, :5], eo3, ev)
    with pytest.raises(ValueError, match="eo3"):
        kernels.triples_energy(X, slots, eo3[:1], ev)
    with pytest.raises(ValueError, match="ev"):
        kernels.triples_energy(X, slots, eo3, torch.zeros(4, dtype=torch.float64))
