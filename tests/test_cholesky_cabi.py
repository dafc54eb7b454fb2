"""CPU-only checks of the Cholesky entry points (``qs_cholesky_two_body`` / ``_workspace`` / ``_block``): the symbols,
every refused argument (no GPU is touched: the checks run before any HIP call), the workspace query, the prototypes
against the header, and the Python layer's own refusals."""

import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F64, C128 = 0, 1
NAMES = ("qs_cholesky_two_body", "qs_cholesky_two_body_workspace", "qs_cholesky_two_body_block")


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as entry

    entry.build()
    from quantum_systems_amd import _lib

    return _lib.load()


def test_symbols_are_exported_and_bound(lib):
    import __graft_entry__ as entry
    from quantum_systems_amd import _lib

    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name in NAMES:
        assert hasattr(raw, name) and name in _lib.SIGNATURES
    assert lib.qs_abi_version() == 4
    assert "qs_cholesky.hip" in entry.SOURCES


def test_signatures_match_the_header():
    from quantum_systems_amd import _lib

    text = open(os.path.join(ROOT, "include", "qs_amd.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    kinds = {"int": ctypes.c_int, "int64_t": ctypes.c_int64, "double": ctypes.c_double}

    def ctype(decl):
        decl = decl.replace("const", "").strip()
        if decl == "void":
            return None
        if "*" in decl:
            base = decl.split("*")[0].strip()
            return ctypes.c_void_p if base == "void" else ("ptr", kinds[base])
        return kinds[decl.rsplit(" ", 1)[0].strip()]

    for name in NAMES:
        ret, args = re.search(r"(\w+)\s+" + name + r"\s*\(([^)]*)\)\s*;", text).groups()
        want = [ctype(a) for a in args.split(",")]
        want = [w for w in want if w is not None]
        restype, argtypes = _lib.SIGNATURES[name]
        assert restype is kinds[ret], name
        assert len(argtypes) == len(want), name
        for got, w in zip(argtypes, want):
            if isinstance(w, tuple):          # a typed pointer: bound as such or as a raw address
                assert got in (ctypes.c_void_p, ctypes.POINTER(w[1])), (name, got, w)
            else:
                assert got is w, (name, got, w)


def test_workspace_query(lib):
    q = lib.qs_cholesky_two_body_workspace
    for m in (1, 5, 16, 17, 21, 253, 512):
        small = q(F64, m, 1)
        assert small >= 64 + 24 * ((m * m + 255) // 256) and small % 16 == 0
        # the state and one partial result per workgroup of 256 elements: independent of the capacity and the dtype
        assert q(F64, m, m * m) == small and q(C128, m, 8 * m) == small
    assert q(F64, 16, 4) < q(F64, 17, 4)
    assert q(7, 4, 4) == -6 and q(-1, 4, 4) == -6
    assert q(F64, 0, 4) == -1 and q(F64, -3, 4) == -1 and q(F64, 4, 0) == -1 and q(F64, 4, -1) == -1
    assert q(F64, 46340, 1) > 0 and q(F64, 46341, 1) == -1            # m^2 <= 2^31 - 1
    assert q(F64, 1 << 40, 1) == -1 and q(F64, 1000, 1 << 62) == -1   # the buffer's bytes fit 63 bits
    assert lib.qs_cholesky_two_body_block() >= 1


def test_refused_arguments_without_gpu(lib):
    # fake, well-separated device addresses: every call below returns before any HIP call is made
    U, V, D, P, W = 1 << 40, 2 << 40, 3 << 40, 4 << 40, 5 << 40
    m, cap = 5, 12
    need = lib.qs_cholesky_two_body_workspace(F64, m, cap)
    extremes = (ctypes.c_double * 2)(7.0, 7.0)

    def call(dtype=F64, u=U, m=m, tau=1e-9, vec=V, cap=cap, rank=0, d=D, piv=P, ext=extremes, work=W, n=need):
        r = None if rank is None else ctypes.byref(ctypes.c_int64(rank))
        return lib.qs_cholesky_two_body(dtype, u, m, tau, vec, cap, r, d, piv, ext, work, n, None)

    assert call(u=None) == -2 and call(vec=None) == -2 and call(d=None) == -2 and call(piv=None) == -2
    assert call(work=None) == -2 and call(rank=None) == -2 and call(ext=None) == -2
    assert call(dtype=2) == -6 and call(dtype=-1) == -6
    assert call(m=0) == -1 and call(m=-4) == -1 and call(m=46341) == -1
    assert call(tau=-1e-300) == -1 and call(tau=float("nan")) == -1 and call(tau=-float("inf")) == -1
    assert call(cap=0) == -1 and call(cap=-2) == -1
    assert call(rank=cap + 1) == -1 and call(rank=-1) == -1
    assert call(dtype=9, u=None) == -6 and call(m=0, u=None) == -1     # order: dtype, extents, null
    assert call(u=U + 4) == -3 and call(vec=V + 4) == -3 and call(d=D + 4) == -3 and call(piv=P + 4) == -3
    assert call(work=W + 8) == -3
    assert call(dtype=C128, u=U + 8) == -3 and call(dtype=C128, vec=V + 8) == -3   # a complex element is 16 bytes
    assert call(n=need - 1) == -4 and call(n=0) == -4
    assert call(u=U + 4, n=0) == -3                                     # alignment is reported before the size
    assert list(extremes) == [7.0, 7.0]                                 # a refused call writes nothing


def test_wrapper_and_module_refuse_without_gpu():
    import torch

    from quantum_systems_amd import cholesky, kernels

    with pytest.raises(RuntimeError, match="GPU only"):
        kernels.cholesky_two_body(torch.zeros(3, 3, 3, 3, dtype=torch.float64), 1e-9)
    with pytest.raises(TypeError):
        kernels.cholesky_two_body([[1.0]], 1e-9)
    with pytest.raises(ValueError, match="step 1"):
        cholesky._index_range(slice(0, 4, 2), 6)
    with pytest.raises(ValueError):
        cholesky._index_range(range(2, 9), 6)
    assert cholesky._index_range(slice(None, 3), 6) == (0, 3) and cholesky._index_range(range(2, 6), 6) == (2, 6)
