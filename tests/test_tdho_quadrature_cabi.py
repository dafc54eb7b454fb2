"""CPU-only checks of the quadrature Coulomb entry points (``qs_tdho_coulomb_quadrature`` / ``_workspace`` and
``qs_tdho_quadrature_nodes``): the symbols, the prototypes against the header, the workspace query, every refused
argument (the checks run before any HIP call, so no GPU is touched), the host-side nodes against NumPy's Gauss-Hermite
rule, and the Python layer's own refusals."""

import ctypes
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("qs_tdho_coulomb_quadrature", "qs_tdho_coulomb_quadrature_workspace", "qs_tdho_quadrature_nodes")


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as entry

    entry.build()
    from quantum_systems_amd import _lib

    return _lib.load()


def workspace(lib, l, shells):
    need = ctypes.c_int64(-7)
    return lib.qs_tdho_coulomb_quadrature_workspace(l, shells, ctypes.byref(need)), need.value


def test_symbols_are_exported_and_bound(lib):
    import __graft_entry__ as entry
    from quantum_systems_amd import _lib

    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name in NAMES:
        assert hasattr(raw, name) and name in _lib.SIGNATURES
    assert lib.qs_abi_version() == 4
    assert "qs_tdho_quadrature.hip" in entry.SOURCES


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


def test_workspace_query(lib):
    for l, shells in ((1, 1), (3, 2), (28, 7), (78, 12), (253, 22), (528, 32), (2048, 32), (10, 9)):
        rc, need = workspace(lib, l, shells)
        # F (l, l, shells) in fp64, m of every orbital, the orbitals grouped by m and where each group starts
        assert rc == 0 and need >= 8 * l * l * shells + 4 * (2 * l + 2 * shells) and need % 16 == 0
        assert need < 8 * l * l * shells + 4 * (2 * l + 2 * shells) + 16
    # max_shell <= 0: the shell order, derived from l
    for l, shells in ((1, 1), (2, 2), (3, 2), (4, 3), (28, 7), (29, 8), (253, 22), (528, 32)):
        assert workspace(lib, l, 0) == workspace(lib, l, shells)
    assert workspace(lib, 529, 0) == (-1, -7)                 # a 33rd shell
    assert workspace(lib, 0, 4) == (-1, -7) and workspace(lib, -3, 4) == (-1, -7) and workspace(lib, 2049, 4) == (-1, -7)
    assert workspace(lib, 10, 33) == (-1, -7)
    assert lib.qs_tdho_coulomb_quadrature_workspace(10, 4, None) == -2


def test_refused_arguments_without_gpu(lib):
    # fake, well-separated device addresses: every call below returns before any HIP call is made
    OUT, TAB, WORK = 1 << 40, 2 << 40, 3 << 40
    l, shells = 10, 5
    _, need = workspace(lib, l, shells)

    def call(out=OUT, tab=TAB, l=l, shells=shells, p_lo=0, p_hi=l, work=WORK, n=need):
        return lib.qs_tdho_coulomb_quadrature(out, tab, l, shells, p_lo, p_hi, work, n, None)

    assert call(out=None) == -2 and call(work=None) == -2
    assert call(l=0) == -1 and call(l=-1) == -1 and call(l=2049, p_hi=1) == -1
    assert call(p_lo=-1) == -1 and call(p_hi=l + 1) == -1 and call(p_lo=4, p_hi=4) == -1 and call(p_lo=5, p_hi=4) == -1
    assert call(shells=0) == -1 and call(shells=-2) == -1 and call(shells=33) == -1
    # without a table max_shell is ignored and derived: nonsense is accepted, a 33rd shell is not
    _, need_shell = workspace(lib, l, 0)
    assert call(tab=None, shells=-5, n=need_shell - 1) == -4 and call(tab=None, shells=99, n=need_shell - 1) == -4
    assert call(tab=None, l=529, p_hi=1, n=1 << 40) == -1 and call(tab=None, l=528, p_hi=1, n=0) == -4
    assert call(out=OUT + 4) == -3 and call(tab=TAB + 2) == -3 and call(work=WORK + 8) == -3
    assert call(n=need - 1) == -4 and call(n=0) == -4 and call(n=-1) == -4
    # order: null, extents, alignment, workspace
    assert call(out=None, l=0) == -2 and call(l=0, out=OUT + 4) == -1 and call(out=OUT + 4, n=0) == -3


@pytest.mark.parametrize("R", [1, 2, 7, 22, 32])
def test_nodes_against_numpy(lib, R):
    k, w = (ctypes.c_double * R)(), (ctypes.c_double * R)()
    assert lib.qs_tdho_quadrature_nodes(R, k, w) == 0
    k, w = np.array(k), np.array(w)
    t, wt = np.polynomial.hermite.hermgauss(2 * R)
    t, wt = t[R:], wt[R:]
    assert (np.diff(k) > 0).all() and k[0] > 0
    node_err = np.abs(k / (np.sqrt(2) * t) - 1).max()
    weight_err = np.abs(w / (np.sqrt(2) * wt * np.exp(t * t)) - 1).max()
    print(f"R = {R}: nodes {node_err:.2e}, weights {weight_err:.2e}")
    assert node_err <= 1e-13 and weight_err <= 1e-12
    # the rule integrates exp(-k^2 / 2) exactly: sum wt_g exp(-k_g^2 / 2) = int_0^inf = sqrt(pi / 2) = max |u|
    assert abs(np.sum(w * np.exp(-0.5 * k * k)) - np.sqrt(np.pi / 2)) <= 1e-13


def test_nodes_match_the_reference(lib):
    import _tdho_quadrature_ref as qref

    for R in (1, 3, 12, 22, 32):
        k, w = (ctypes.c_double * R)(), (ctypes.c_double * R)()
        assert lib.qs_tdho_quadrature_nodes(R, k, w) == 0
        rk, rw = qref.nodes(R)
        np.testing.assert_allclose(np.array(k), rk, rtol=1e-14, atol=0)
        np.testing.assert_allclose(np.array(w), rw, rtol=1e-13, atol=0)


def test_nodes_refusals(lib):
    k, w = (ctypes.c_double * 40)(*([7.0] * 40)), (ctypes.c_double * 40)(*([7.0] * 40))
    assert lib.qs_tdho_quadrature_nodes(0, k, w) == -1 and lib.qs_tdho_quadrature_nodes(33, k, w) == -1
    assert lib.qs_tdho_quadrature_nodes(-4, k, w) == -1
    assert lib.qs_tdho_quadrature_nodes(4, None, w) == -2 and lib.qs_tdho_quadrature_nodes(4, k, None) == -2
    assert list(k) == [7.0] * 40 and list(w) == [7.0] * 40          # a refused call writes nothing
    assert lib.qs_tdho_quadrature_nodes(4, k, w) == 0 and list(k)[4:] == [7.0] * 36


def test_python_layer_refuses_without_gpu():
    import torch

    from quantum_systems_amd import two_dim_ho as td

    with pytest.raises(ValueError, match="method"):
        td.get_coulomb_elements(6, method="series")
    with pytest.raises(ValueError, match="at most 32 shells"):
        td.get_coulomb_elements(529, method="quadrature")
    with pytest.raises(ValueError, match="at most 32 shells"):
        td.get_coulomb_elements(3, nm=[(0, 0), (0, 32), (16, 0)], method="quadrature")
    with pytest.raises(ValueError, match="every orbital"):
        td.get_coulomb_elements(3, nm=[(0, 0), (0, 1)], method="quadrature")
    with pytest.raises(ValueError, match="coulomb"):
        td.TwoDimensionalHarmonicOscillator(3, 5, 11, coulomb="exact")
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError, match="GPU only"):
            td.get_coulomb_elements(6, method="quadrature")
