"""CPU-only checks of the Coulomb-vector entry points (``qs_tdho_coulomb_vectors`` / ``_workspace`` / ``_rank``): the
symbols, the prototypes against the header, the queries, every refused argument (the checks run before any HIP call, so
no GPU is touched) in the documented order, and the Python layer's own refusals."""

import ctypes
import os
import re

import numpy as np
import pytest

import _tdho_quadrature_ref as qref
import _tdho_vectors_ref as vref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("qs_tdho_coulomb_vectors", "qs_tdho_coulomb_vectors_workspace", "qs_tdho_coulomb_vectors_rank")


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as entry

    entry.build()
    from quantum_systems_amd import _lib

    return _lib.load()


def rank_of(lib, l, shells, nm=None):
    out = ctypes.c_int64(-7)
    table = None if nm is None else np.ascontiguousarray(np.asarray(nm, dtype=np.int32).T)
    rc = lib.qs_tdho_coulomb_vectors_rank(None if table is None else table.ctypes.data, l, shells, ctypes.byref(out))
    return rc, out.value


def test_symbols_are_exported_and_bound(lib):
    from quantum_systems_amd import _lib

    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name in NAMES:
        assert hasattr(raw, name) and name in _lib.SIGNATURES
    assert lib.qs_abi_version() == 4


def test_signatures_match_the_header():
    from quantum_systems_amd import _lib

    text = open(os.path.join(ROOT, "include", "qs_amd.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    kinds = {"int": ctypes.c_int, "int64_t": ctypes.c_int64, "double": ctypes.c_double}

    def ctype(decl):
        decl = decl.replace("const", "").strip()
        if "*" in decl:
            base = decl.split("*")[0].strip()
            return ctypes.c_void_p if base == "void" else ctypes.POINTER(kinds[base])
        return kinds[decl.rsplit(" ", 1)[0].strip()]

    for name in NAMES:
        ret, args = re.search(r"(\w+)\s+" + name + r"\s*\(([^)]*)\)\s*;", text).groups()
        restype, argtypes = _lib.SIGNATURES[name]
        assert restype is kinds[ret], name
        assert argtypes == [ctype(a) for a in args.split(",")], name
    assert _lib.SIGNATURES["qs_tdho_coulomb_vectors"] == _lib.SIGNATURES["qs_tdho_coulomb_quadrature"]


def test_workspace_is_the_quadrature_workspace(lib):
    for l, shells in ((1, 1), (3, 2), (28, 7), (253, 22), (528, 32), (528, 0), (2048, 32), (10, 9)):
        a, b = ctypes.c_int64(-7), ctypes.c_int64(-9)
        assert lib.qs_tdho_coulomb_vectors_workspace(l, shells, ctypes.byref(a)) == 0
        assert lib.qs_tdho_coulomb_quadrature_workspace(l, shells, ctypes.byref(b)) == 0
        assert a.value == b.value and a.value % 16 == 0
    need = ctypes.c_int64(-7)
    for l, shells in ((529, 0), (0, 4), (2049, 4), (10, 33)):
        assert lib.qs_tdho_coulomb_vectors_workspace(l, shells, ctypes.byref(need)) == -1 and need.value == -7
    assert lib.qs_tdho_coulomb_vectors_workspace(10, 4, None) == -2


def test_rank_query(lib):
    for R in range(1, 33):
        assert rank_of(lib, R * (R + 1) // 2, 0) == (0, R * (4 * R - 3))
    for l in (1, 2, 3, 4, 8, 10, 15, 21, 28, 56, 100, 527, 528):
        nm = qref.shell_table(l)
        assert rank_of(lib, l, -3) == (0, vref.rank(nm))                       # shell order: max_shell is derived
        assert rank_of(lib, l, qref.max_shell(nm), nm) == (0, vref.rank(nm))   # the same table, spelled out
    asym = vref.table(nm=vref.ASYMMETRIC)
    assert rank_of(lib, 7, 6, asym) == (0, 66) and rank_of(lib, 7, 9, asym) == (0, 99)
    # refusals: null, extents (l, a 33rd shell, max_shell, a table wider than its max_shell), alignment
    assert lib.qs_tdho_coulomb_vectors_rank(None, 4, 0, None) == -2
    assert rank_of(lib, 0, 0) == (-1, -7) and rank_of(lib, 529, 0) == (-1, -7) and rank_of(lib, 2049, 4, asym) == (-1, -7)
    assert rank_of(lib, 7, 0, asym) == (-1, -7) and rank_of(lib, 7, 33, asym) == (-1, -7)
    assert rank_of(lib, 7, 3, asym) == (-1, -7)
    buf = np.zeros(16, dtype=np.int32)
    out = ctypes.c_int64(-7)
    assert lib.qs_tdho_coulomb_vectors_rank(buf.ctypes.data + 2, 7, 6, ctypes.byref(out)) == -3 and out.value == -7


def test_refused_arguments_without_gpu(lib):
    # fake, well-separated device addresses: every call below returns before any HIP call is made
    OUT, TAB, WORK = 1 << 40, 2 << 40, 3 << 40
    l, shells = 10, 5
    need = ctypes.c_int64(0)
    assert lib.qs_tdho_coulomb_vectors_workspace(l, shells, ctypes.byref(need)) == 0
    need = need.value
    _, rank = rank_of(lib, l, 0)                     # 4 shells in shell order: 52
    assert rank == 52

    def call(out=OUT, tab=TAB, l=l, shells=shells, x_lo=0, x_hi=1, work=WORK, n=need):
        return lib.qs_tdho_coulomb_vectors(out, tab, l, shells, x_lo, x_hi, work, n, None)

    assert call(out=None) == -2 and call(work=None) == -2
    assert call(l=0) == -1 and call(l=-1) == -1 and call(l=2049) == -1
    assert call(x_lo=-1) == -1 and call(x_lo=4, x_hi=4) == -1 and call(x_lo=5, x_hi=4) == -1
    assert call(shells=0) == -1 and call(shells=-2) == -1 and call(shells=33) == -1
    # under a table x_hi is bounded by what max_shell allows, R (4 R - 3); the shell order knows its rank
    assert call(x_hi=5 * 17 + 1) == -1 and call(x_hi=5 * 17, n=0) == -4
    assert call(tab=None, x_hi=rank + 1) == -1 and call(tab=None, x_hi=rank, n=0) == -4
    # without a table max_shell is ignored and derived: nonsense is accepted, a 33rd shell is not
    assert call(tab=None, shells=-5, n=0) == -4 and call(tab=None, shells=99, n=0) == -4
    assert call(tab=None, l=529, n=1 << 40) == -1 and call(tab=None, l=528, x_hi=4000, n=0) == -4
    assert call(tab=None, l=528, x_hi=4001, n=1 << 40) == -1
    assert call(out=OUT + 4) == -3 and call(tab=TAB + 2) == -3 and call(work=WORK + 8) == -3
    assert call(n=need - 1) == -4 and call(n=0) == -4 and call(n=-1) == -4
    # order: null, extents, alignment, workspace
    assert call(out=None, l=0) == -2 and call(l=0, out=OUT + 4) == -1 and call(x_hi=0, out=OUT + 4) == -1
    assert call(out=OUT + 4, n=0) == -3


def test_python_layer_refuses_without_gpu():
    import torch

    from quantum_systems_amd import two_dim_ho as td

    assert td.COULOMB_METHODS == ("closed_form", "quadrature")
    with pytest.raises(ValueError, match="at most 32 shells"):
        td.get_coulomb_vectors(529)
    with pytest.raises(ValueError, match="at most 32 shells"):
        td.get_coulomb_vectors(3, nm=[(0, 0), (0, 32), (16, 0)])
    with pytest.raises(ValueError, match="at most 32 shells"):
        td.coulomb_vectors(529)
    with pytest.raises(ValueError, match="every orbital"):
        td.get_coulomb_vectors(3, nm=[(0, 0), (0, 1)])
    with pytest.raises(ValueError, match="x_lo:x_hi"):
        td.get_coulomb_vectors(10, x_lo=3, x_hi=3)
    with pytest.raises(ValueError, match="x_lo:x_hi"):
        td.get_coulomb_vectors(10, x_hi=53)
    for cls in (td.TwoDimensionalHarmonicOscillator, td.TwoDimensionalDoubleWell, td.TwoDimHarmonicOscB):
        with pytest.raises(ValueError, match='needs coulomb="quadrature"'):
            cls(3, 5, 11, two_body="vectors")
        with pytest.raises(ValueError, match="two_body must be one of"):
            cls(3, 5, 11, coulomb="quadrature", two_body="factors")
    with pytest.raises(ValueError, match="at most 32 shells"):
        td.TwoDimensionalHarmonicOscillator(529, 5, 11, coulomb="quadrature", two_body="vectors")
    assert td.coulomb_vectors_rank(528) == 4000 and td.coulomb_vectors_rank(7, nm=vref.ASYMMETRIC) == 66
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError, match="GPU only"):
            td.get_coulomb_vectors(6)
