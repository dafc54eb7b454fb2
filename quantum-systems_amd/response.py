"""Response of a state to a perturbation from a Lanczos recurrence on ``H``: generic, like
``determinant_ci.block_davidson`` -- the operator is a callable ``sigma(V) -> H V`` on row vectors.

With ``|phi> = (A - <A>)|Psi_k>`` as start, ``n`` steps give a tridiagonal matrix whose eigenvalues ``theta_j`` and first
eigenvector components ``y_j[0]`` are ``n`` poles and weights of

    S(omega) = sum_j |<j|A|Psi_k>|^2 delta(omega - (E_j - E_k)),     omega_j = theta_j - E_k,   w_j = <phi|phi> |y_j[0]|^2

that reproduce the first ``2 n`` moments ``sum_j w_j omega_j^p`` (p = 0 ... 2 n - 1) of ``S`` exactly, and with them the
polarizability as a finite sum.  The recurrence keeps three vectors.

    alpha, beta, norm2 = lanczos(sigma, phi, 64)
    S = SpectralFunction(alpha, beta, norm2, E_k)
    S.poles, S.weights, S.response(0.0), S.broadened(omega, 0.01)

``StringCI.spectral_function`` / ``dipole_spectrum`` / ``polarizability`` build on it."""

import numpy
import torch

from . import kernels


def lanczos(sigma, start, n_steps, reorthogonalize=False, beta_tol=0.0):
    """The three-term recurrence of a Hermitian operator ``sigma(V) -> H V`` on row vectors (1, dim) from ``start`` (any
    shape with dim elements), on the device of ``start``.  Returns ``(alpha, beta, norm2)``: the diagonal and the
    off-diagonal of the tridiagonal matrix as host float64 arrays of the steps actually taken
    (``len(beta) == len(alpha) - 1``), and ``norm2 = <start|start>``; a zero ``start`` gives empty arrays.

    The recurrence stops early only where ``beta_j <= beta_tol * max(|alpha|, beta so far)`` or where ``beta_j`` is 0 or
    not finite.  The default is no early stop: at the exhaustion of a Krylov space the computed ``beta`` is small but far
    from machine epsilon, the recurrence continues through rounding, and moments and response stay right.

    ``reorthogonalize=True`` keeps the basis (n_steps, dim) and removes it from every new vector in two Gram-Schmidt
    sweeps; it raises ``ValueError`` where those ``n_steps * dim`` elements exceed ``kernels.STRING_CI_BYTES`` (tuning key
    ``string_ci_bytes``)."""
    n_steps = int(n_steps)
    if n_steps < 0:
        raise ValueError(f"n_steps must not be negative, got {n_steps}")
    with torch._C.DisableTorchFunctionSubclass():
        q = start.reshape(1, -1)
        dim = q.shape[1]
        if reorthogonalize and n_steps * dim * q.element_size() > kernels.string_ci_budget():
            raise ValueError(f"the basis of {n_steps} x {dim} elements of a reorthogonalised recurrence exceeds the byte budget "
                             "kernels.STRING_CI_BYTES: fewer steps, or reorthogonalize=False")
        norm2 = float(torch.vdot(q[0], q[0]).real.item())
        alpha, beta = [], []
        if n_steps == 0 or not norm2 > 0.0 or not numpy.isfinite(norm2):
            return numpy.zeros(0), numpy.zeros(0), norm2
        q = q / norm2 ** 0.5
        basis = torch.empty(n_steps, dim, dtype=q.dtype, device=q.device) if reorthogonalize else None
        before, b, scale = None, 0.0, 0.0
        for j in range(n_steps):
            w = sigma(q)
            a = float(torch.vdot(q[0], w[0]).real.item())
            w = w - a * q
            if before is not None:
                w = w - b * before
            if basis is not None:
                basis[j] = q[0]
                Q = basis[:j + 1]
                for _ in range(2):
                    w = w - (w @ Q.conj().transpose(0, 1)) @ Q
            alpha.append(a)
            if j + 1 == n_steps:
                break
            b = float(torch.linalg.vector_norm(w).item())
            scale = max(scale, abs(a))
            if not b > 0.0 or not numpy.isfinite(b) or b <= beta_tol * scale:
                break
            scale = max(scale, b)
            beta.append(b)
            before, q = q, w / b
    return numpy.array(alpha, dtype=numpy.float64), numpy.array(beta, dtype=numpy.float64), norm2


class SpectralFunction:
    """Poles and weights of ``S(omega) = sum_j w_j delta(omega - omega_j)`` from the tridiagonal matrix ``(alpha, beta)`` of a
    Lanczos run started at ``|phi> = (A - <A>)|Psi>``, ``norm2 = <phi|phi>``, ``E_state`` the energy of ``|Psi>`` on the
    scale of the operator of the run: ``poles`` = ``theta_j - E_state`` ascending, ``weights`` = ``norm2 |y_j[0]|^2``, from
    one host ``eigh``.  Empty arrays are the empty spectrum."""

    def __init__(self, alpha, beta, norm2, E_state):
        self.alpha = numpy.asarray(alpha, dtype=numpy.float64).reshape(-1)
        self.beta = numpy.asarray(beta, dtype=numpy.float64).reshape(-1)
        n = self.alpha.shape[0]
        if self.beta.shape[0] != max(n - 1, 0):
            raise ValueError(f"{n} diagonal elements go with {max(n - 1, 0)} off-diagonal ones, got {self.beta.shape[0]}")
        self.norm2, self.E_state = float(norm2), float(E_state)
        if n == 0:
            self.poles, self.weights = numpy.zeros(0), numpy.zeros(0)
            return
        T = numpy.diag(self.alpha) + numpy.diag(self.beta, 1) + numpy.diag(self.beta, -1)
        theta, Y = numpy.linalg.eigh(T)
        self.poles = theta - self.E_state
        self.weights = self.norm2 * numpy.abs(Y[0]) ** 2

    def moment(self, p):
        """``sum_j w_j omega_j^p``."""
        return float(numpy.sum(self.weights * self.poles ** p))

    def response(self, omega, eta=0.0):
        """``sum_j w_j (1 / (omega_j - omega - i eta) + 1 / (omega_j + omega + i eta))``: the polarizability
        ``alpha_AA(omega)`` of a Hermitian ``A``; real for ``eta == 0``.  ``omega`` is a number or an array."""
        om = numpy.asarray(omega, dtype=numpy.float64)
        z = om[..., None] + (1j * float(eta) if eta != 0.0 else 0.0)
        out = numpy.sum(self.weights * (1.0 / (self.poles - z) + 1.0 / (self.poles + z)), axis=-1)
        return out if om.ndim else out[()]

    def broadened(self, omega, eta):
        """``sum_j w_j (eta / pi) / ((omega - omega_j)^2 + eta^2)``: the spectrum with Lorentzians of half width ``eta``."""
        om = numpy.asarray(omega, dtype=numpy.float64)
        out = numpy.sum(self.weights * (float(eta) / numpy.pi) / ((om[..., None] - self.poles) ** 2 + float(eta) ** 2), axis=-1)
        return out if om.ndim else out[()]

    def oscillator_strengths(self):
        """``2 omega_j w_j``."""
        return 2.0 * self.poles * self.weights
