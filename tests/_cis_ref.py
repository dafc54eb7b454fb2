"""Dense NumPy configuration interaction singles, for the tests of ``configuration_interaction.CIS``:

    A[ia,jb] = (e_a - e_i) d_ij d_ab + cj <aj|ib> + ck <aj|bi>,      u[p,q,r,s] = <pq|rs>

with ``u`` transformed to the canonical orbitals by ``einsum``, the spectrum by ``eigvalsh`` / ``eigh`` and the dense
transition moments.  Flavours (cj, ck): spin orbitals with an anti-symmetrised u (1, 0), with a plain u (1, -1);
closed-shell singlets (2, -1), triplets (0, -1).  Nothing here imports the package under test; the problems, the plain
SCF and the mean-field sums come from tests/_mean_field_ref.py."""

import numpy as np

import _mean_field_ref as ref

FLAVOURS = {"gos": (1.0, 0.0), "gos_plain": (1.0, -1.0), "singlet": (2.0, -1.0), "triplet": (0.0, -1.0)}


def scf_orbitals(h, u, s, n_occ, occupation, cj, ck, tol=1e-10, max_iter=500):
    """The fixed-point iteration of ``ref.plain_scf`` (core guess, Loewdin, no DIIS), returning what that function
    keeps to itself: ``(energy, epsilon, C)`` of the converged Fock matrix, ``C^H s C = 1``."""
    sv, sU = np.linalg.eigh(s)
    X = (sU / np.sqrt(sv)) @ sU.conj().T

    def diagonalise(F):
        eps, Cp = np.linalg.eigh(X.conj().T @ F @ X)
        return eps, X @ Cp

    _, C = diagonalise(h)
    for _ in range(max_iter):
        rho = occupation * C[:, :n_occ] @ C[:, :n_occ].conj().T
        W = ref.mean_field(u, rho, cj, ck)
        F = h + W
        energy = np.einsum("pq,qp->", h + 0.5 * W, rho).real
        err = X.conj().T @ (F @ rho @ s - s @ rho @ F) @ X
        if np.abs(err).max() < tol:
            eps, C = diagonalise(F)
            return energy, eps, C
        _, C = diagonalise(F)
    raise RuntimeError("plain SCF did not converge")


def to_canonical(u, C):
    return np.einsum("pa,qb,pqrs,rc,sd->abcd", C.conj(), C.conj(), u, C, C, optimize=True)


def cis_matrix(eps, u_mo, n_occ, cj, ck):
    """A over (ia, jb), (o v) x (o v), from the two-body elements in the canonical orbitals."""
    l = len(eps)
    o, v = slice(0, n_occ), slice(n_occ, l)
    no, nv = n_occ, l - n_occ
    A = cj * u_mo[v, o, o, v].transpose(2, 0, 1, 3) + ck * u_mo[v, o, v, o].transpose(3, 0, 1, 2)   # [i,a,j,b]
    A = A.reshape(no * nv, no * nv).astype(np.result_type(u_mo.dtype, np.float64))
    gap = (eps[None, v] - eps[o, None]).reshape(no * nv)
    return A + np.diag(gap)


def spectrum(eps, u_mo, n_occ, flavour):
    return np.linalg.eigvalsh(cis_matrix(eps, u_mo, n_occ, *FLAVOURS[flavour]))


def transition_moments(X, position_mo, n_occ, factor):
    """mu_n = factor * sum_ia X_n[i,a] x[i,a]; ``X`` (n, o, v), ``position_mo`` (dim, l, l) in the canonical orbitals."""
    return factor * np.einsum("nia,dia->nd", X, position_mo[:, :n_occ, n_occ:])
