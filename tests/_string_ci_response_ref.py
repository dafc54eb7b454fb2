"""Host restatement of ``kernels.string_ci_one_body`` and of the Lanczos response on it (``response.lanczos``,
``response.SpectralFunction``, ``StringCI.spectral_function``), sharing nothing with either:

  * ``one_body``: the operator on two string lists in ``numpy.longdouble`` from the ladder oracle's ``E`` of each list
    (``_string_ci_ref.list_E``), in the style of ``_string_ci_ref.kh_sigma``; applied to the moduli it is the kernel's
    error bound;
  * ``lanczos_dense``: the three-term recurrence on a dense Hermitian matrix in float64;
  * ``dense_spectrum``: poles and weights of ``S(omega) = sum_j |<j|A|c0>|^2 delta(omega - (E_j - E_0))`` from ``eigh``;
  * the sums both are compared through (``moments``, ``response``) and the shared cases of the host and the GPU test."""

import functools

import numpy as np

import _string_ci_ref as ref
from _string_ci_ref import _wide

CASES = [(4, 2, 2, False), (4, 2, 2, True), (4, 2, 1, False)]          # (m, Na, Nb, complex Hamiltonian)
WEIGHT_FLOOR = 1e-24          # a dense pole counts where its weight is above this fraction of the total


def one_body(Aa, Ab, Ea, Eb, c):
    """``out[x, k] = sum_pq (Aa[x,p,q] E^alpha_pq + Ab[x,p,q] E^beta_pq) c[k]`` in longdouble: ``Aa``, ``Ab`` (d, m, m),
    ``Ea`` (m, m, na, na), ``Eb`` (m, m, nb, nb), ``c`` (K, na, nb) -> (d, K, na, nb)."""
    return _one_body(Aa, Ab, Ea, Eb, c, True)


def _one_body(Aa, Ab, Ea, Eb, c, wide):
    """``einsum("xa,aij,kjb->xkib", Aa, Ea, c) + einsum("xa,abj,kij->xkib", Ab, Eb, c)`` with a = (pq), summed over the non-zero
    elements of every ``E[a]`` (at most one per row: the row indices of one ``a`` are distinct), so that a list of 330
    strings stays cheap."""
    m, na, nb = Ea.shape[0], Ea.shape[2], Eb.shape[2]
    up = _wide if wide else np.asarray
    cw, Aa, Ab = up(np.asarray(c)), up(np.asarray(Aa)), up(np.asarray(Ab))
    dt = np.result_type(cw.dtype, Aa.dtype, Ab.dtype)
    Aa, Ab, cw = Aa.reshape(-1, m * m).astype(dt), Ab.reshape(-1, m * m).astype(dt), cw.astype(dt)
    Ea, Eb = Ea.reshape(m * m, na, na), Eb.reshape(m * m, nb, nb)
    out = np.zeros((Aa.shape[0], cw.shape[0], na, nb), dtype=dt)
    for a in range(m * m):
        i, j = np.nonzero(Ea[a])
        assert len(set(i.tolist())) == len(i)
        out[:, :, i, :] += Aa[:, a][:, None, None, None] * (Ea[a][i, j].astype(dt)[None, :, None] * cw[:, j, :])[None]
        i, j = np.nonzero(Eb[a])
        assert len(set(i.tolist())) == len(i)
        out[:, :, :, i] += Ab[:, a][:, None, None, None] * (Eb[a][i, j].astype(dt)[None, None, :] * cw[:, :, j])[None]
    return out


def one_body_bound(Aa, Ab, Ea, Eb, c):
    """``|got - exact| <= gamma_(2 m^2 + 2) one_body(|Aa|, |Ab|, |Ea|, |Eb|, |c|)``: at most 2 m^2 terms, each one fma on
    an exactly signed copy of c; a complex product (a complex A) costs a further 2 sqrt 2, a real A against a complex c does
    not: its real and imaginary parts are two real sums."""
    m = Ea.shape[0]
    # the same function on the moduli, in float64: the rounding of the bound itself is far below it
    b = _one_body(np.abs(Aa), np.abs(Ab), np.abs(Ea), np.abs(Eb), np.abs(c), False)
    cplx = np.iscomplexobj(Aa) or np.iscomplexobj(Ab)
    return ref.gamma(2 * m * m + 2) * b * (2.0 * np.sqrt(2.0) if cplx else 1.0)


def lanczos_dense(H, phi, n, reorth):
    """``(alpha, beta, norm2)`` of ``n`` steps on the dense Hermitian ``H`` from ``phi`` (float64 / complex128); with
    ``reorth`` two Gram-Schmidt sweeps against the kept basis per step.  No early stop."""
    phi = np.asarray(phi)
    norm2 = float(np.vdot(phi, phi).real)
    q, before, b = phi / np.sqrt(norm2), None, 0.0
    alpha, beta, basis = [], [], []
    for j in range(n):
        w = H @ q
        a = float(np.vdot(q, w).real)
        w = w - a * q - (b * before if before is not None else 0.0)
        if reorth:
            basis.append(q)
            Q = np.array(basis)
            for _ in range(2):
                w = w - Q.T @ (Q.conj() @ w)
        alpha.append(a)
        if j + 1 == n:
            break
        b = float(np.linalg.norm(w))
        beta.append(b)
        before, q = q, w / b
    return np.array(alpha), np.array(beta), norm2


def poles_weights(alpha, beta, norm2, E):
    """Poles ``theta_j - E`` (ascending) and weights ``norm2 |y_j[0]|^2`` of a tridiagonal matrix."""
    T = np.diag(alpha) + np.diag(beta, 1) + np.diag(beta, -1)
    theta, Y = np.linalg.eigh(T)
    return theta - E, norm2 * np.abs(Y[0]) ** 2


def dense_spectrum(H, Aop, c0):
    """``(omega_j, w_j)`` of the dense operator ``Aop`` on the unit vector ``c0``: ``omega_j = E_j - <c0|H|c0>``,
    ``w_j = |<j|(Aop - <Aop>)|c0>|^2``, the poles below ``WEIGHT_FLOOR`` of the total weight left out."""
    lam, V = np.linalg.eigh(H)
    E0 = float(np.vdot(c0, H @ c0).real)
    phi = Aop @ c0
    phi = phi - np.vdot(c0, phi) * c0
    w = np.abs(V.conj().T @ phi) ** 2
    keep = w > WEIGHT_FLOOR * w.sum()
    return lam[keep] - E0, w[keep]


def moments(om, w, orders):
    """``(sum_j w_j omega_j^p, sum_j w_j |omega_j|^p)`` for p in ``orders``."""
    return (np.array([np.sum(w * om ** p) for p in orders]), np.array([np.sum(w * np.abs(om) ** p) for p in orders]))


def response(om, w, freq):
    """``(sum_j w_j (1 / (omega_j - f) + 1 / (omega_j + f)), sum_j w_j (1 / |omega_j - f| + 1 / (omega_j + f)))`` for f in
    ``freq``: the value and the scale its error is taken against."""
    f = np.asarray(freq)[:, None]
    return np.sum(w * (1.0 / (om - f) + 1.0 / (om + f)), axis=1), np.sum(w * (1.0 / np.abs(om - f) + 1.0 / (om + f)), axis=1)


def kept_frequencies(om):
    """41 frequencies in [0, 1.2 omega_max] without those closer than 0.02 omega_max to a (weighted) pole."""
    top = float(om.max())
    f = np.linspace(0.0, 1.2 * top, 41)
    return f[np.abs(f[:, None] - om[None, :]).min(axis=1) >= 0.02 * top]


@functools.lru_cache(maxsize=None)
def case(m, Na, Nb, cplx):
    """``(ht, ut, H, A, Aop, c0, omega, w)`` of one shared case: the seeded Hamiltonian of the string tests, ``A = B + B^T``
    with ``B`` from ``default_rng(5)``, the dense ground vector and its dense spectrum.  Computed once, read-only."""
    ht, ut = ref.random_hamiltonian(m, 100 + 10 * m + 3 * Na + Nb, cplx)
    H = ref.dense_hamiltonian(ht, ut, Na, Nb)
    B = np.random.default_rng(5).standard_normal((m, m))
    A = B + B.T
    Aop = np.einsum("pq,pqij->ij", A, ref.dense_E(m, Na, Nb))
    c0 = np.linalg.eigh(H)[1][:, 0].copy()
    om, w = dense_spectrum(H, Aop, c0)
    out = (ht, ut, H, A, Aop, c0, om, w)
    for a in out:
        a.setflags(write=False)
    return out


def worst_moment_error(om, w, got_om, got_w, orders):
    """The largest ``|moment_p(got) - moment_p(dense)| / sum_j w_j |omega_j|^p`` over ``orders``."""
    want, scale = moments(om, w, orders)
    got, _ = moments(got_om, got_w, orders)
    return float((np.abs(got - want) / scale).max())


def worst_response_error(om, w, got_om, got_w, freq):
    want, scale = response(om, w, freq)
    got, _ = response(got_om, got_w, freq)
    return float((np.abs(got - want) / scale).max())
