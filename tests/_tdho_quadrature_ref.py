"""NumPy restatement of the quadrature form of the 2-D harmonic-oscillator
Coulomb elements -- TEST INFRASTRUCTURE ONLY, the CPU reference of
``qs_tdho_coulomb_quadrature``.

    u[p,q,r,s] = delta(m_p + m_q, m_r + m_s) * sum_g wt_g F_pr(k_g) F_qs(k_g)

``F_pr`` is the form factor of the orbital pair: with the circular quanta
a = n + (|m| + m) / 2, b = n + (|m| - m) / 2 and x = k^2 / 4 it is a signed
product of two displacement-operator elements D(a_p, a_r; x) D(b_p, b_r; x),

    D(a, a'; x) = sqrt(lo! / hi!) x^((hi - lo) / 2) exp(-x / 2) L_lo^(hi - lo)(x).

The nodes k_g = sqrt(2) t_g and weights wt_g = sqrt(2) w_g exp(t_g^2) are the R
positive nodes of the 2R-point Gauss-Hermite rule, which is exact here: F_pr F_qs
is exp(-k^2 / 2) times an even polynomial of degree <= 4 (R - 1) in k.

Nothing alternates: every D is an orthonormal Laguerre function (|D| <= 1) from
its three-term recurrence in normalised form, and the weights come from the
orthonormal Hermite functions, so no intermediate leaves the fp64 range.
"""

import numpy as np


def indices_nm(p):
    """(n, m) of orbital p in shell order (shells of 1, 2, 3, ... states, m ascending)."""
    shell = 1
    while shell * (shell + 1) // 2 <= p:
        shell += 1
    m = -(shell - 1) + 2 * (p - shell * (shell - 1) // 2)
    return (shell - 1 - abs(m)) // 2, m


def shell_table(l):
    return np.array([indices_nm(p) for p in range(l)], dtype=np.int64).reshape(l, 2)


def max_shell(nm):
    nm = np.asarray(nm)
    return int((2 * nm[:, 0] + np.abs(nm[:, 1]) + 1).max())


def _hermite_functions(t, N):
    """psi_{N-1}(t), psi_N(t): orthonormal Hermite functions (Gaussian included)."""
    lo = np.zeros_like(t)
    hi = np.pi ** -0.25 * np.exp(-0.5 * t * t)
    for n in range(N):
        lo, hi = hi, t * np.sqrt(2.0 / (n + 1)) * hi - np.sqrt(n / (n + 1.0)) * lo
    return lo, hi


def nodes(R, extra=0):
    """k_g and wt_g, ascending, of the (2 R + 2 extra)-point rule: its positive half."""
    N = 2 * (R + extra)
    off = np.sqrt(np.arange(1, N) / 2.0)
    t = np.linalg.eigvalsh(np.diag(off, 1) + np.diag(off, -1))[N // 2:]        # Golub-Welsch start
    for _ in range(3):                                                         # Newton on psi_N
        lo, hi = _hermite_functions(t, N)
        t = t - hi / (np.sqrt(2.0 * N) * lo - t * hi)
    lo, _ = _hermite_functions(t, N)
    # w_g = 1 / (N p_{N-1}(t_g)^2) for orthonormal polynomials p: w_g exp(t_g^2) = 1 / (N psi_{N-1}(t_g)^2)
    return np.sqrt(2.0) * t, np.sqrt(2.0) / (N * lo * lo)


def displacement(a, b, x):
    """D(a, b; x) for integers a, b >= 0 and an array x > 0."""
    lo, al = min(a, b), abs(a - b)
    prod = np.ones_like(x)
    for j in range(1, al + 1):
        prod = prod * (x / j)
    prev, cur = np.zeros_like(x), np.sqrt(prod) * np.exp(-0.5 * x)
    for n in range(lo):
        prev, cur = cur, ((2 * n + 1 + al - x) * cur - np.sqrt(n * (n + al)) * prev) / np.sqrt((n + 1.0) * (n + 1 + al))
    return cur


def form_factors(nm, k):
    """F[p, r, g] for the orbital table nm (l, 2) at the nodes k."""
    nm = np.asarray(nm, dtype=np.int64)
    n, m = nm[:, 0], nm[:, 1]
    a, b = n + (np.abs(m) + m) // 2, n + (np.abs(m) - m) // 2
    x = 0.25 * k * k
    top = int(max(a.max(), b.max())) + 1
    D = np.zeros((top, top, len(k)))
    for i in range(top):
        for j in range(i, top):
            D[i, j] = D[j, i] = displacement(i, j, x)
    da, db, dm = np.abs(a[:, None] - a[None, :]), np.abs(b[:, None] - b[None, :]), np.abs(m[:, None] - m[None, :])
    sign = 1.0 - 2.0 * ((n[:, None] + n[None, :] + (da + db - dm) // 2) % 2)
    return sign[:, :, None] * D[a[:, None], a[None, :]] * D[b[:, None], b[None, :]]


class Quadrature:
    """Form factors of one orbital table, once; elements and slabs from them."""

    def __init__(self, nm, extra=0):
        self.nm = np.asarray(nm, dtype=np.int64)
        self.m = self.nm[:, 1]
        self.k, self.w = nodes(max_shell(self.nm), extra)
        self.F = form_factors(self.nm, self.k)

    def element(self, p, q, r, s):
        if self.m[p] + self.m[q] != self.m[r] + self.m[s]:
            return 0.0
        return float(np.sum(self.F[p, r] * self.F[q, s] * self.w))

    def elements(self, idx):
        """u at the rows of idx (K, 4)."""
        p, q, r, s = np.asarray(idx, dtype=np.int64).T
        val = np.einsum("kg,kg,g->k", self.F[p, r], self.F[q, s], self.w)
        return np.where(self.m[p] + self.m[q] == self.m[r] + self.m[s], val, 0.0)

    def slab(self, p_lo=0, p_hi=None):
        """u[p_lo:p_hi] in full."""
        l = len(self.nm)
        p_hi = l if p_hi is None else p_hi
        u = np.einsum("prg,qsg,g->pqrs", self.F[p_lo:p_hi], self.F, self.w, optimize=True)
        m = self.m
        keep = (m[p_lo:p_hi, None, None, None] + m[None, :, None, None]) == (m[None, None, :, None] + m[None, None, None, :])
        return np.where(keep, u, 0.0)


def coulomb_elements(l, p_lo=0, p_hi=None, nm=None):
    return Quadrature(shell_table(l) if nm is None else nm).slab(p_lo, p_hi)
