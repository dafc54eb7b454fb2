"""CPU-only checks of the Coulomb vectors' NumPy reference (``_tdho_vectors_ref``): the full ``sum_x M_x (x) L_x`` is
the quadrature tensor, the rank formula, the band structure and the transpose pairing of the layout."""

import numpy as np
import pytest

import _tdho_quadrature_ref as qref
import _tdho_vectors_ref as vref

EPS = np.finfo(np.float64).eps
SIZES = (1, 2, 3, 4, 8, 10, 15, 21, 28)


def tables():
    return [(f"l{l}", qref.shell_table(l)) for l in SIZES] + [("asymmetric", vref.table(nm=vref.ASYMMETRIC))]


@pytest.mark.parametrize("name,nm", tables(), ids=[n for n, _ in tables()])
def test_vectors_rebuild_the_quadrature_tensor(name, nm):
    quad = qref.Quadrature(nm)
    want = quad.slab()
    got = vref.reconstruct(vref.vectors(nm, quad))
    err = np.abs(got - want).max()
    print(f"{name}: rank {vref.rank(nm)}, max |sum_x M_x (x) L_x - u| = {err:.2e}, max |u| = {np.abs(want).max():.3f}")
    assert err <= 8 * EPS * np.abs(want).max()
    # elements that do not conserve m come out as exact zeros: every product of two bands that do not match is 0 * 0
    m = nm[:, 1]
    keep = (m[:, None, None, None] + m[None, :, None, None]) == (m[None, None, :, None] + m[None, None, None, :])
    assert not got[~keep].any()


def test_rank_formula():
    for R in range(1, 33):
        l = R * (R + 1) // 2
        nm = qref.shell_table(l)
        assert vref.rank(nm) == vref.full_shell_rank(R) == R * (4 * R - 3)
    assert vref.rank(qref.shell_table(528)) == 4000
    # a cut shell keeps m_min = -(R - 1); m_max is the larger of the cut shell's last m and R - 2
    assert vref.rank(qref.shell_table(4)) == 3 * 7 and vref.rank(qref.shell_table(8)) == 4 * 11
    assert vref.rank(vref.table(nm=vref.ASYMMETRIC)) == 6 * 11
    for l in SIZES:
        assert vref.vectors(qref.shell_table(l)).shape == (vref.rank(qref.shell_table(l)), l, l)


@pytest.mark.parametrize("l", [3, 8, 15])
def test_layout_bands_slabs_and_transpose_pairs(l):
    nm = qref.shell_table(l)
    quad = qref.Quadrature(nm)
    L = vref.vectors(nm, quad)
    R, span, m = len(quad.k), vref.m_span(nm), nm[:, 1]
    n_mu = 2 * span + 1
    assert L.shape[0] == R * n_mu
    for x in range(L.shape[0]):
        j, g = divmod(x, R)
        band = (m[None, :] - m[:, None]) == j - span
        assert not L[x][~band].any() and not np.signbit(L[x][~band]).any()
        np.testing.assert_array_equal(L[x][band], (np.sqrt(quad.w[g]) * quad.F[:, :, g])[band])
        # out[(j, g)][q][s] == out[(N - 1 - j, g)][s][q]
        np.testing.assert_array_equal(L[x], L[(n_mu - 1 - j) * R + g].T)
    np.testing.assert_array_equal(vref.vectors(nm, quad, 2, 7), L[2:7])
