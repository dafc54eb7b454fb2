"""CPU-only checks of the entry points of (T) with singles (``qs_triples_energy_singles`` / ``_workspace``): the symbols,
the workspace query, every refused argument (no GPU is touched: the checks run before any HIP call), and the Python
wrapper's own refusals.  The entry points are additions: the ABI version stays 4."""

import ctypes

import pytest

F64, C128 = 0, 1
NAMES = ("qs_triples_energy_singles", "qs_triples_energy_singles_workspace")


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as entry

    entry.build()
    from quantum_systems_amd import _lib

    return _lib.load()


def test_symbols_are_exported_and_bound(lib):
    import __graft_entry__ as entry
    from quantum_systems_amd import _lib, kernels

    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name in NAMES:
        assert hasattr(raw, name) and name in _lib.SIGNATURES
    assert lib.qs_abi_version() == 4 and _lib.ABI_VERSION == 4
    assert "qs_triples.hip" in entry.SOURCES and not any("singles" in s for s in entry.SOURCES)     # no new source file
    assert callable(kernels.triples_energy_singles)
    with open(entry.os.path.join(entry.ROOT, "include", "qs_amd.h")) as fh:
        header = fh.read()
    for name in NAMES:
        assert name + "(" in header


def test_workspace_query(lib):
    q, base = lib.qs_triples_energy_singles_workspace, lib.qs_triples_energy_workspace
    tile = {F64: lib.qs_triples_energy_tile(F64), C128: lib.qs_triples_energy_tile(C128)}
    for code in (F64, C128):
        for v in (1, 5, tile[code], tile[code] + 1, 2 * tile[code] + 1, 250, 4096):
            nt = -(-v // tile[code])
            for n in (1, 3, 40):
                assert q(code, v, n) == 16 * n * (nt * (nt + 1) * (nt + 2) // 6)      # two partials per (triple, tile set)
                assert q(code, v, n) == 2 * base(code, v, n)
    assert q(7, 4, 4) == -6 and q(-1, 4, 4) == -6
    assert q(F64, 0, 4) == -1 and q(F64, -3, 4) == -1 and q(F64, 4, 0) == -1 and q(F64, 4, -1) == -1
    assert q(F64, 4097, 1) == -1
    nt = -(-4096 // tile[F64])
    most = (2 ** 31 - 1) // (nt * (nt + 1) * (nt + 2) // 6)
    assert q(F64, 4096, most) > 0 and q(F64, 4096, most + 1) == -1


def test_refused_arguments_without_gpu(lib):
    # fake, well-separated device addresses: every call below returns before any HIP call is made
    X, S, EO, EV, A, G, SS, E, ES, W = (x << 40 for x in range(1, 11))
    v, n, nblocks, na, ng = 9, 4, 24, 3, 9

    def call(dtype=F64, x=X, nblocks=nblocks, slots=S, eo3=EO, ev=EV, a=A, na=na, g=G, ng=ng, sslots=SS, v=v, n=n, e=E,
             es=ES, work=W, nbytes=None):
        if nbytes is None:
            nbytes = max(lib.qs_triples_energy_singles_workspace(F64, v, n), 0)
        return lib.qs_triples_energy_singles(dtype, x, nblocks, slots, eo3, ev, a, na, g, ng, sslots, v, n, e, es, work,
                                             nbytes, None)

    for name in ("x", "slots", "eo3", "ev", "a", "g", "sslots", "e", "es", "work"):
        assert call(**{name: None}) == -2, name
    assert call(dtype=2) == -6 and call(dtype=-1) == -6
    assert call(v=0) == -1 and call(v=-2) == -1 and call(v=4097) == -1
    assert call(n=0) == -1 and call(n=-1) == -1 and call(n=1 << 31) == -1
    assert call(nblocks=0) == -1 and call(nblocks=-3) == -1 and call(nblocks=1 << 31) == -1
    assert call(na=0) == -1 and call(na=-1) == -1 and call(na=1 << 31) == -1
    assert call(ng=0) == -1 and call(ng=-1) == -1 and call(ng=1 << 31) == -1
    assert call(v=4096, nblocks=(1 << 63) // (4096 ** 3 * 8) + 1, nbytes=1 << 50) == -1   # the bytes of X past int64
    assert call(dtype=9, x=None) == -6 and call(v=0, x=None) == -1 and call(na=0, a=None) == -1   # order: dtype, extents, null
    assert call(x=X + 4) == -3 and call(slots=S + 2) == -3 and call(eo3=EO + 4) == -3 and call(ev=EV + 4) == -3
    assert call(a=A + 4) == -3 and call(g=G + 4) == -3 and call(sslots=SS + 2) == -3
    assert call(e=E + 4) == -3 and call(es=ES + 4) == -3 and call(work=W + 4) == -3
    assert call(dtype=C128, x=X + 8) == -3 and call(dtype=C128, a=A + 8) == -3 and call(dtype=C128, g=G + 8) == -3
    need = lib.qs_triples_energy_singles_workspace(F64, v, n)
    assert call(nbytes=need - 1) == -4 and call(nbytes=need // 2) == -4 and call(nbytes=0) == -4
    assert call(x=X + 4, nbytes=0) == -3                                     # alignment is reported before the size
    # an output inside an input, inside the workspace, inside the other output; the workspace inside an input
    for out in ("e", "es"):
        assert call(**{out: X + 8 * v ** 3}) == -7 and call(**{out: W + 8}) == -7 and call(**{out: W + need - 8}) == -7
        assert call(**{out: EO}) == -7 and call(**{out: EV + 8}) == -7 and call(**{out: S + 16}) == -7
        assert call(**{out: A + 8}) == -7 and call(**{out: G + 8 * v * v}) == -7 and call(**{out: SS + 40}) == -7
    assert call(e=ES) == -7 and call(es=E + 8) == -7
    assert call(work=X) == -7 and call(work=G) == -7 and call(work=A - 8) == -7 and call(work=SS) == -7


def test_wrapper_refuses_without_gpu():
    import torch

    from quantum_systems_amd import kernels

    v = 3
    X = torch.zeros(6, v, v, v, dtype=torch.float64)
    slots = torch.zeros((2, 6), dtype=torch.int32)
    eo3, ev = torch.zeros(2, dtype=torch.float64), torch.zeros(v, dtype=torch.float64)
    A, G = torch.zeros(2, v, dtype=torch.float64), torch.zeros(4, v, v, dtype=torch.float64)
    sslots = torch.zeros((2, 6, 2), dtype=torch.int32)
    f = kernels.triples_energy_singles
    with pytest.raises(RuntimeError, match="GPU only"):
        f(X, slots, eo3, ev, A, G, sslots)
    with pytest.raises(TypeError):
        f(X.float(), slots, eo3, ev, A, G, sslots)
    with pytest.raises(ValueError, match="nblocks, v, v, v"):
        f(X[:, :, :2], slots, eo3, ev, A, G, sslots)
    with pytest.raises(ValueError, match="slots"):
        f(X, slots.long(), eo3, ev, A, G, sslots)
    with pytest.raises(ValueError, match="eo3"):
        f(X, slots, eo3[:1], ev, A, G, sslots)
    with pytest.raises(ValueError, match="ev"):
        f(X, slots, eo3, torch.zeros(4, dtype=torch.float64), A, G, sslots)
    with pytest.raises(ValueError, match="A must be"):
        f(X, slots, eo3, ev, A[:, :2], G, sslots)
    with pytest.raises(ValueError, match="A must be"):
        f(X, slots, eo3, ev, A.to(torch.complex128), G, sslots)
    with pytest.raises(ValueError, match="G must be"):
        f(X, slots, eo3, ev, A, G[:, :, :2], sslots)
    with pytest.raises(ValueError, match="G must be"):
        f(X, slots, eo3, ev, A, G[0], sslots)
    with pytest.raises(ValueError, match="sslots"):
        f(X, slots, eo3, ev, A, G, sslots[:, :, 0])
    with pytest.raises(ValueError, match="sslots"):
        f(X, slots, eo3, ev, A, G, sslots.long())
    with pytest.raises(ValueError, match="sslots"):
        f(X, slots, eo3, ev, A, G, sslots[:1])
