"""Host restatement of ``kernels.string_ci_ladder_table`` / ``string_ci_ladder`` and of the removal and addition spectra on
them, sharing nothing with either:

  * ``ladder``: the signed map of ONE spin between two string lists, from the textbook ``a_p`` / ``a+_p`` of ``_det_ci_ref``
    (``_ladder``, ``_land``) -- no table, no search of the package's;
  * ``apply``: ``sum_p phi[x,p] a_p c`` (or ``a+_p``: the lists decide) in ``numpy.longdouble``, with the ``(-1)^n_alpha`` of a
    beta ladder; on the moduli it is the kernel's error bound (``bound``);
  * ``dense_ladder``: ``a_p,spin`` between two sectors in ``(Ia, Ib)`` order from the Jordan-Wigner matrices on the 2 m spin
    orbitals and ``_string_ci_ref.sector_map`` of both sectors;
  * ``dense_removal_spectrum`` / ``dense_addition_spectrum``: poles and weights from ``eigh`` of the dense Hamiltonian of the
    neighbouring sector, and the sums the spectra are compared through."""

import functools

import numpy as np

import _det_ci_ref as dref
import _string_ci_ref as ref
from _string_ci_ref import _wide

WEIGHT_FLOOR = 1e-24          # a dense pole counts where its weight is above this fraction of the total


def ladder(strs_t, strs_s, m):
    """``M[p, J, I] = <target J| a_p |source I>`` where the source is a particle richer, ``<target J| a+_p |source I>`` where it
    is a particle poorer: (m, n_t, n_s), entries 0 and +-1; a mask outside the target list contributes nothing."""
    dets_t, _ = dref._start(strs_t)
    _, start = dref._start(strs_s)
    M = np.zeros((m, len(dets_t), len(start[0])))
    for p in range(m):
        for fill in (False, True):
            col, row, sign = dref._land(dets_t, dref._ladder(start, p, fill))
            M[p, row, col] += sign
    return M


def table(M):
    """The ladder table (n_t, m) int32 of the map ``M``: ``+-(I + 1)``, at most one source per (J, p)."""
    m, n_t, _ = M.shape
    T = np.zeros((n_t, m), dtype=np.int32)
    for p in range(m):
        J, I = np.nonzero(M[p])
        assert len(set(J.tolist())) == len(J)
        T[J, p] = (M[p][J, I] * (I + 1)).astype(np.int32)
    return T


def _apply(phi, spin, n_alpha, M, c, wide):
    up = _wide if wide else np.asarray
    phi, cw = up(np.asarray(phi)), up(np.asarray(c))
    dt = np.result_type(phi.dtype, cw.dtype)
    phi, cw = phi.astype(dt), cw.astype(dt)
    m, n_t = M.shape[0], M.shape[1]
    K, na, nb = cw.shape
    out = np.zeros((phi.shape[0], K) + ((n_t, nb) if spin == 0 else (na, n_t)), dtype=dt)
    parity = -1.0 if (spin == 1 and n_alpha % 2) else 1.0
    for p in range(m):
        J, I = np.nonzero(M[p])
        s = (parity * M[p][J, I]).astype(dt)
        if spin == 0:
            out[:, :, J, :] += phi[:, p][:, None, None, None] * (s[None, :, None] * cw[:, I, :])[None]
        else:
            out[:, :, :, J] += phi[:, p][:, None, None, None] * (s[None, None, :] * cw[:, :, I])[None]
    return out


def apply(phi, spin, n_alpha, M, c):
    """``out[x, k] = sum_p phi[x, p] (a_p or a+_p) c[k]`` in longdouble: ``phi`` (d, m), ``M`` from ``ladder`` for the lists of
    ``spin`` (0 alpha, 1 beta), ``c`` (K, na_s, nb_s) -> (d, K, na_t, nb_t); a beta ladder carries ``(-1)^n_alpha``."""
    return _apply(phi, spin, n_alpha, M, c, True)


def moduli(phi, spin, M, x):
    """``apply`` on the moduli of everything, in float64 (no sign, no ``n_alpha``): how an error ``x`` of the argument grows
    through the operator, and the sum behind ``bound``."""
    return _apply(np.abs(phi), spin, 0, np.abs(M), np.abs(x), False)


def bound(phi, spin, M, c):
    """``|got - exact| <= gamma_(m + 2) apply(|phi|, |M|, |c|)``: at most m terms, each one fma of a coefficient with an
    exactly signed copy of c; a complex product (a complex phi) costs a further 2 sqrt 2, a real phi against a complex c
    does not."""
    return ref.gamma(M.shape[0] + 2) * moduli(phi, spin, M, c) * (2.0 * np.sqrt(2.0) if np.iscomplexobj(phi) else 1.0)


@functools.lru_cache(maxsize=None)
def _annihilators(n):
    return dref.annihilators(n)


@functools.lru_cache(maxsize=None)
def dense_ladder(m, Na, Nb, p, spin):
    """``a_p,spin`` from the (Na, Nb) sector to the one with a particle of ``spin`` less, both in ``(Ia, Ib)`` order:
    (dim_t, dim_s).  Its transpose is ``a+_p,spin`` the other way."""
    Nat, Nbt = (Na - 1, Nb) if spin == 0 else (Na, Nb - 1)
    op = _annihilators(2 * m)[2 * p + spin]
    block = op[np.ix_(dref.sector(2 * m, Nat + Nbt), dref.sector(2 * m, Na + Nb))]
    pos_s, phase_s = ref.sector_map(m, Na, Nb)
    pos_t, phase_t = ref.sector_map(m, Nat, Nbt)
    out = block[np.ix_(pos_t, pos_s)] * phase_t[:, None] * phase_s[None, :]
    out.setflags(write=False)
    return out


def _spectrum(Hn, phi, E0):
    lam, V = np.linalg.eigh(Hn)
    w = np.abs(V.conj().T @ phi) ** 2
    keep = w > WEIGHT_FLOOR * w.sum()
    return lam[keep] - E0, w[keep]


def dense_removal_spectrum(ht, ut, Na, Nb, v, spin, c0):
    """``(E_j(N - 1) - E_0, |<j| sum_p v[p] a_p,spin |c0>|^2)`` of the unit vector ``c0`` (dim,) of the (Na, Nb) sector, from
    ``eigh`` of the dense Hamiltonian of the smaller sector; ``E_0 = <c0|H|c0>``."""
    m = ht.shape[0]
    E0 = float(np.vdot(c0, ref.dense_hamiltonian(ht, ut, Na, Nb) @ c0).real)
    phi = sum(v[p] * (dense_ladder(m, Na, Nb, p, spin) @ c0) for p in range(m))
    Nat, Nbt = (Na - 1, Nb) if spin == 0 else (Na, Nb - 1)
    return _spectrum(ref.dense_hamiltonian(ht, ut, Nat, Nbt), phi, E0)


def dense_addition_spectrum(ht, ut, Na, Nb, v, spin, c0):
    """``(E_j(N + 1) - E_0, |<j| sum_p v[p] a+_p,spin |c0>|^2)``, as ``dense_removal_spectrum``."""
    m = ht.shape[0]
    E0 = float(np.vdot(c0, ref.dense_hamiltonian(ht, ut, Na, Nb) @ c0).real)
    Nat, Nbt = (Na + 1, Nb) if spin == 0 else (Na, Nb + 1)
    phi = sum(v[p] * (dense_ladder(m, Nat, Nbt, p, spin).T @ c0) for p in range(m))
    return _spectrum(ref.dense_hamiltonian(ht, ut, Nat, Nbt), phi, E0)


def response(om, w, freq):
    """``(sum_j w_j (1 / (omega_j - f) + 1 / (omega_j + f)), sum_j w_j (1 / |omega_j - f| + 1 / |omega_j + f|))`` for f in
    ``freq``: ``SpectralFunction.response`` and the scale its error is taken against.  The poles of a removal or addition
    spectrum have either sign, so both terms of the scale carry moduli."""
    f = np.asarray(freq)[:, None]
    return np.sum(w * (1.0 / (om - f) + 1.0 / (om + f)), axis=1), np.sum(w * (1.0 / np.abs(om - f) + 1.0 / np.abs(om + f)), axis=1)


def green(add, rem, omega, eta):
    """``(G, scale)``: the retarded ``sum_j w+_j / (omega - p+_j + i eta) + sum_j w-_j / (omega + p-_j + i eta)`` of two
    ``(poles, weights)`` pairs, and the sum of the moduli of its terms."""
    z = np.asarray(omega)[:, None] + 1j * eta
    terms = np.concatenate([add[1] / (z - add[0]), rem[1] / (z + rem[0])], axis=1)
    return terms.sum(axis=1), np.abs(terms).sum(axis=1)
