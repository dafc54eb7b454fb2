"""Writes tests/golden/tdho_coulomb_mp.npz: Coulomb elements of the 2-D
harmonic oscillator from the top three shells at 12, 16 and 22 shells, from an
80-digit mpmath evaluation of the closed form of Anisimovas & Matulis (the sums
that csrc/qs_tdho.hip and oracle/coulomb_ho.c evaluate in fp64, where they lose
everything to cancellation from about 9 shells on).

Every factorial ratio of the closed form is an integer binomial here, and the two
innermost sums over (l0, l1) and (l2, l3) at fixed l0 + l1 = l2 + l3 are integer
convolutions; the Gamma functions, the powers of sqrt(2), the sums over them and
the closing square root are mpmath at 80 digits.  Elements are picked with
sum(n) <= 8, seeded; the four 22-shell elements of PINNED are always included and
checked against the values recorded with them.

    python tools/gen_tdho_mp_golden.py            # writes the fixture (seconds)
"""

import math
import os
import sys

import mpmath
import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "tests", "golden", "tdho_coulomb_mp.npz")

mpmath.mp.dps = 80

# (n, m) of p, q, r, s at 22 shells and the value to reproduce
PINNED = [
    (((0, -19), (1, 18), (0, -21), (0, 20)), -0.029671737635106804),
    (((3, 13), (1, -18), (2, 15), (0, -20)), 0.02292945290759265),
    (((2, -17), (1, -19), (3, -15), (0, -21)), 0.021930132211655042),
    (((1, -18), (1, -17), (2, -17), (1, -18)), -0.015000211350296038),
]


def _signed_convolution(ga, gb):
    """c[s] = sum_{la + lb = s} C(ga, la) * (-1)^(gb - lb) C(gb, lb): exact integers."""
    out = [0] * (ga + gb + 1)
    for la in range(ga + 1):
        ca = math.comb(ga, la)
        for lb in range(gb + 1):
            out[la + lb] += ca * math.comb(gb, lb) * (-1 if (gb - lb) & 1 else 1)
    return out


def coulomb_ho_mp(p, q, r, s):
    """<pq|u|rs> for p, q, r, s = (n, m), omega = 1, as an mpf.  The closed form's
    parameter order is (i, j, l, k) = (p, q, r, s)."""
    (n_i, m_i), (n_j, m_j), (n_l, m_l), (n_k, m_k) = p, q, r, s
    if m_i + m_j != m_k + m_l:
        return mpmath.mpf(0)
    am = [abs(m) for m in (m_i, m_j, m_k, m_l)]
    M_i, M_j, M_k, M_l = ((a + m) // 2 for a, m in zip(am, (m_i, m_j, m_k, m_l)))
    d_i, d_j, d_k, d_l = ((a - m) // 2 for a, m in zip(am, (m_i, m_j, m_k, m_l)))
    half = mpmath.mpf(1) / 2
    element = mpmath.mpf(0)
    for j0 in range(n_i + 1):
        for j1 in range(n_j + 1):
            for j2 in range(n_k + 1):
                for j3 in range(n_l + 1):
                    g0, g1 = j0 + j3 + M_i + d_l, j1 + j2 + M_j + d_k
                    g2, g3 = j2 + j1 + M_k + d_j, j3 + j0 + M_l + d_i
                    G = g0 + g1 + g2 + g3
                    A = _signed_convolution(g0, g1)          # over (l0, l1): sign (-1)^(g1 - l1)
                    B = _signed_convolution(g3, g2)          # over (l3, l2): sign (-1)^(g2 - l2)
                    temp = mpmath.mpf(0)
                    for t in range(min(len(A), len(B))):
                        if A[t] and B[t]:
                            temp += mpmath.gamma(1 + t) * mpmath.gamma((G - 2 * t + 1) * half) * (A[t] * B[t])
                    lead = (math.comb(n_i + am[0], n_i - j0) * math.comb(n_j + am[1], n_j - j1)
                            * math.comb(n_k + am[2], n_k - j2) * math.comb(n_l + am[3], n_l - j3))
                    below = math.factorial(j0) * math.factorial(j1) * math.factorial(j2) * math.factorial(j3)
                    w = mpmath.mpf(lead) / below * mpmath.power(2, -(G + 1) * half) * temp
                    element += -w if (j0 + j1 + j2 + j3) & 1 else w
    norm = mpmath.mpf(1)
    for n, a in zip((n_i, n_j, n_k, n_l), am):
        norm *= mpmath.mpf(math.factorial(n)) / math.factorial(n + a)
    return element * mpmath.sqrt(norm)


def _top_orbitals(shells):
    """(n, m) of the top three shells."""
    return [(n, m) for e in range(shells - 3, shells) for n in range(e // 2 + 1)
            for m in ((e - 2 * n, -(e - 2 * n)) if e - 2 * n else (0,))]


def pick(shells, count, rng, have=()):
    """count elements of the top three shells, `have` among them; every other one has p among the last three orbitals
    (the slab that the GPU test generates at 22 shells)."""
    orbitals = _top_orbitals(shells)
    known = set(orbitals)
    last = [(0, shells - 1), (1, shells - 3), (2, shells - 5)]
    chosen = list(have)
    while len(chosen) < count:
        p, q, r = (orbitals[i] for i in rng.integers(0, len(orbitals), 3))
        if len(chosen) % 2:
            p = last[rng.integers(0, 3)]
        m_s = p[1] + q[1] - r[1]
        fits = [(n, m_s) for n in range(shells) if (n, m_s) in known]
        if not fits:
            continue
        s = fits[rng.integers(0, len(fits))]
        quad = (p, q, r, s)
        if sum(o[0] for o in quad) <= 8 and quad not in chosen:
            chosen.append(quad)
    return chosen


def main():
    rng = np.random.default_rng(20261020)
    shells, nm, val = [], [], []
    for R, count in ((12, 14), (16, 14), (22, 14)):
        quads = pick(R, count, rng, have=[q for q, _ in PINNED] if R == 22 else ())
        for quad in quads:
            v = coulomb_ho_mp(*quad)
            shells.append(R)
            nm.append(quad)
            val.append(float(v))
            print(R, quad, mpmath.nstr(v, 20), flush=True)
    for (quad, want) in PINNED:
        got = val[nm.index(quad)]
        assert abs(got - want) <= 1e-17, (quad, got, want)
    np.savez(OUT, shells=np.array(shells, dtype=np.int32), nm=np.array(nm, dtype=np.int32), val=np.array(val))
    print("wrote", OUT, len(val), "elements")


if __name__ == "__main__":
    sys.exit(main())
