"""Pins the NumPy reference of the quadrature Coulomb elements (``tests/_tdho_quadrature_ref.py``) on the CPU: against
the C oracle where the oracle's closed form is still exact enough, and against 80-digit values of that closed form at
12, 16 and 22 shells (``tests/golden/tdho_coulomb_mp.npz``, written by ``tools/gen_tdho_mp_golden.py``).

Every comparison with a quadrature value is absolute at 1e-13 (max |u| = sqrt(pi / 2)): a cap, not a measurement --
the values measured here are in DESIGN 3.19."""

import numpy as np
import pytest

import _tdho_quadrature_ref as qref
from oracle import coulomb_oracle as co

ATOL = 1e-13
PINNED = [          # four 22-shell elements evaluated independently: (n, m) of p, q, r, s and the 80-digit value
    (((0, -19), (1, 18), (0, -21), (0, 20)), -0.029671737635106804),
    (((3, 13), (1, -18), (2, 15), (0, -20)), 0.02292945290759265),
    (((2, -17), (1, -19), (3, -15), (0, -21)), 0.021930132211655042),
    (((1, -18), (1, -17), (2, -17), (1, -18)), -0.015000211350296038),
]


def index_p(n, m):
    shell = 2 * n + abs(m) + 1
    return shell * (shell - 1) // 2 + (m + shell - 1) // 2


@pytest.fixture(scope="module")
def quadratures():
    return {R: qref.Quadrature(qref.shell_table(R * (R + 1) // 2)) for R in (12, 16, 22)}


def test_shell_order_is_the_oracles():
    for p in range(300):
        assert qref.indices_nm(p) == co.indices_nm(p)
        assert index_p(*qref.indices_nm(p)) == p


def test_against_the_oracle_at_three_shells():
    err = np.abs(qref.coulomb_elements(6) - co.coulomb_elements(6)).max()
    print(f"3 shells: {err:.2e}")
    assert err <= 1e-14


def test_against_the_oracle_at_five_shells():
    got, ref = qref.coulomb_elements(15), co.coulomb_elements(15)
    err = np.abs(got - ref).max()
    print(f"5 shells: {err:.2e}")
    assert err <= 1e-12                      # the oracle's own error there
    assert np.array_equal(got == 0, ref == 0)
    assert abs(np.abs(got).max() - np.sqrt(np.pi / 2)) <= ATOL


def test_fixture_holds_the_pinned_elements(golden):
    g = golden("tdho_coulomb_mp")
    assert sorted(set(g["shells"].tolist())) == [12, 16, 22] and 36 <= len(g["val"]) <= 48
    quads = [tuple(map(tuple, q)) for q in g["nm"].tolist()]
    for quad, want in PINNED:
        at = quads.index(quad)
        assert g["shells"][at] == 22 and abs(g["val"][at] - want) <= 1e-17
    for R, quad in zip(g["shells"], g["nm"]):
        n, m = quad[:, 0], quad[:, 1]
        assert m[0] + m[1] == m[2] + m[3] and n.sum() <= 8
        assert ((2 * n + abs(m) + 1 >= R - 2) & (2 * n + abs(m) + 1 <= R)).all()      # the top three shells


@pytest.mark.parametrize("R", [12, 16, 22])
def test_against_the_high_precision_values(golden, quadratures, R):
    g = golden("tdho_coulomb_mp")
    sel = g["shells"] == R
    idx = np.array([[index_p(*o) for o in quad] for quad in g["nm"][sel]])
    err = np.abs(quadratures[R].elements(idx) - g["val"][sel]).max()
    print(f"{R} shells: {err:.2e} over {sel.sum()} elements")
    assert err <= ATOL


def test_extra_nodes_change_nothing(quadratures):
    # the rule is exact with R nodes: 8 more move 3000 seeded top-shell elements by rounding only
    R = 22
    l = R * (R + 1) // 2
    rng = np.random.default_rng(22)
    more = qref.Quadrature(qref.shell_table(l), extra=8)
    top = np.arange(l - R, l)
    idx = []
    while len(idx) < 3000:
        p, q, r = rng.choice(top, 3)
        s = np.flatnonzero(more.m == more.m[p] + more.m[q] - more.m[r])
        if len(s):
            idx.append((p, q, r, rng.choice(s)))
    idx = np.array(idx)
    err = np.abs(quadratures[R].elements(idx) - more.elements(idx)).max()
    print(f"8 extra nodes: {err:.2e}")
    assert err <= ATOL


def test_form_factors_are_symmetric_and_bounded(quadratures):
    F = quadratures[16].F
    assert np.array_equal(F, F.transpose(1, 0, 2)) and np.abs(F).max() <= 1.0 + 1e-15
    k = quadratures[16].k
    # F_pp(k) -> 1 as k -> 0, and the diagonal of the lowest orbital is the Gaussian exp(-k^2 / 4)
    np.testing.assert_allclose(F[0, 0], np.exp(-0.25 * k * k), rtol=1e-15)


def test_table_order_and_slabs():
    nm, _ = co.level_table(np.arange(6), np.arange(-9, 10), omega_c=0.5, omega=np.sqrt(1 + 0.25 / 4))
    l = 10
    Q = qref.Quadrature(nm[:l])
    full = Q.slab()
    assert np.array_equal(Q.slab(3, 5), full[3:5])
    rng = np.random.default_rng(3)
    for p, q, r, s in rng.integers(0, l, size=(300, 4)):
        assert abs(full[p, q, r, s] - co.coulomb_element_nm(nm, p, q, r, s)) <= 1e-12
        assert full[p, q, r, s] == Q.element(p, q, r, s) or abs(full[p, q, r, s] - Q.element(p, q, r, s)) <= 1e-15
