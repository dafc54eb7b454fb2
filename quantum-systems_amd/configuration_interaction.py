"""Excited states by configuration interaction singles (CIS, the Tamm-Dancoff form of TDHF) on top of
``kernels.mean_field_batch``.

What follows a converged ``HartreeFock.scf()``: the lowest eigenpairs of

    A[ia,jb] = (e_a - e_i) d_ij d_ab + cj <aj|ib> + ck <aj|bi>

by a block Davidson iteration.  A sigma vector is a mean-field contraction of ``u`` with a transition density,

    D_k      = C_v X_k^T C_o^H                                 (AO basis; l x l products in torch)
    W_k      = cj u[p,r,q,s] D_k[s,r] + ck u[p,r,s,q] D_k[s,r]  (ONE mean_field_batch call for all trial vectors of a step)
    sigma_k[i,a] = (e_a - e_i) X_k[i,a] + (C_v^H W_k C_o)[a,i]

so a Davidson step reads ``u`` once per group of trial vectors, never once per vector, and ``u`` is never transformed.

    (cj, ck):  GeneralOrbitalSystem, anti-symmetrised u (1, 0);  plain u (1, -1);
               SpatialOrbitalSystem, singlets (2, -1);  triplets (0, -1)

``u[p,q,r,s] = <pq|rs>`` is taken to be Hermitian (as ``moller_plesset`` states), so ``A`` is Hermitian.

    hf = HartreeFock(system); hf.scf()
    cis = hf.cis()
    omega, X = cis.solve(n_roots=4)                  # spin="triplet" for the triplets of a closed shell
    mu = cis.transition_dipole_moments()
"""

import math

import torch

from . import kernels
from .basis_set import _deliver, _stage, refuse_vectors_only
from .general_orbital_system import GeneralOrbitalSystem
from .sharded_module import is_sharded
from .spatial_orbital_system import SpatialOrbitalSystem


def _plain(arr):
    return _stage(arr).as_subclass(torch.Tensor)


def _dagger(A):
    return A.conj().transpose(-2, -1)


class CIS:
    """CIS of ``system`` on the canonical orbitals ``C`` with energies ``epsilon`` (both as ``HartreeFock.scf`` returns
    them; the system stays in its basis), or with neither: the system IS in its Hartree-Fock basis already and
    ``epsilon`` is the diagonal of its Fock matrix -- the convention of ``mp2_energy``.

    ``batched=False`` sends the trial vectors of a step through the same kernel one by one (the same numbers bit for
    bit, one read of ``u`` per vector): the baseline of the timing in ``examples/cis_quantum_dot.py``."""

    def __init__(self, system, C=None, epsilon=None, batched=True):
        refuse_vectors_only(system, "CIS")
        if not isinstance(system, (SpatialOrbitalSystem, GeneralOrbitalSystem)):
            raise TypeError("CIS needs a SpatialOrbitalSystem or a GeneralOrbitalSystem")
        n_occ = system.n
        if not 0 < n_occ < system.l:
            raise ValueError(f"{n_occ} occupied of {system.l} orbitals leave no occupied-virtual block")
        if (C is None) != (epsilon is None):
            raise ValueError("give both C and epsilon, or neither (system already in its canonical basis)")
        if is_sharded(system.u):
            raise NotImplementedError("CIS does not take a sharded u: the batched mean-field contraction is not sharded")
        self.system, self.batched = system, batched
        self.n_occ, self.n_virt = n_occ, system.l - n_occ
        with torch._C.DisableTorchFunctionSubclass():
            self._u = _plain(system.u)
            if C is None:
                f = _plain(system.construct_fock_matrix(system.h, system.u))
                eps = f.diagonal()
                C = torch.eye(system.l, dtype=f.dtype, device=f.device)
            else:
                C, eps = _plain(C), _plain(epsilon)
            eps = (eps.real if eps.is_complex() else eps).to(torch.float64)
            self._dt = torch.complex128 if (C.is_complex() or self._u.is_complex()) else torch.float64
            C = C.to(self._dt)
            self._Co, self._Cv = C[:, :n_occ].contiguous(), C[:, n_occ:].contiguous()
            self._gap = (eps[None, n_occ:] - eps[:n_occ, None]).contiguous()       # (o, v): e_a - e_i
        self.omega = self.X = self.spin = None
        self.converged, self.iterations, self.residuals = False, 0, None
        self.sigma_history = []              # trial vectors sent through u, per Davidson iteration

    def _weights(self, spin):
        if isinstance(self.system, GeneralOrbitalSystem):
            if spin != "singlet":
                raise ValueError("spin= applies to a SpatialOrbitalSystem; spin orbitals carry every multiplicity")
            return self.system._mean_field_weights()
        if spin == "singlet":
            return 2.0, -1.0
        if spin == "triplet":
            return 0.0, -1.0
        raise ValueError(f"spin must be 'singlet' or 'triplet', got {spin!r}")

    def sigma(self, X, spin="singlet"):
        """``A X_k`` for trial vectors ``X`` (k, o, v), device tensor in and out: one pass over ``u`` per group."""
        cj, ck = self._weights(spin)
        X = X.to(self._dt)
        D = (self._Cv @ X.transpose(1, 2) @ _dagger(self._Co)).contiguous()        # (k, l, l)
        if self.batched:
            W = kernels.mean_field_batch(self._u, D, cj=cj, ck=ck)
        else:
            W = torch.cat([kernels.mean_field_batch(self._u, D[k:k + 1], cj=cj, ck=ck) for k in range(D.shape[0])])
        W = W.to(self._dt)
        return self._gap * X + (_dagger(self._Cv) @ W @ self._Co).transpose(1, 2)

    def solve(self, n_roots, tol=1e-8, max_iter=100, max_space=None, spin="singlet"):
        """The ``n_roots`` lowest excitation energies and their vectors by a block Davidson iteration: unit guesses on
        the ``min(o v, 2 n_roots)`` lowest ``e_a - e_i``, the diagonal preconditioner ``(e_a - e_i - theta)^-1``, new
        vectors orthonormalised against the space, collapse to the Ritz vectors above ``max_space`` vectors.  A root is
        converged when its residual 2-norm is below ``tol``.  Returns ``(omega, X)`` in the system's array module,
        ``omega`` ascending and ``X`` (n_roots, o, v) with unit norm; sets ``converged``, ``iterations``, ``residuals``."""
        o, v = self.n_occ, self.n_virt
        dim = o * v
        if not 1 <= n_roots <= dim:
            raise ValueError(f"n_roots = {n_roots} does not fit the {o} x {v} singles space")
        self._weights(spin)
        n_guess = min(dim, 2 * n_roots)
        if max_space is None:
            max_space = max(20, 10 * n_roots)
        max_space = min(dim, max(int(max_space), 2 * n_guess))
        with torch._C.DisableTorchFunctionSubclass():
            gap = self._gap.reshape(dim)
            order = torch.argsort(gap, stable=True)[:n_guess]
            V = torch.zeros(n_guess, dim, dtype=self._dt, device=gap.device)
            V[torch.arange(n_guess), order] = 1.0
            AV = torch.empty(0, dim, dtype=self._dt, device=gap.device)
            self.sigma_history, self.converged = [], False
            for it in range(1, max_iter + 1):
                self.iterations = it
                new = V[AV.shape[0]:]
                self.sigma_history.append(new.shape[0])
                AV = torch.cat([AV, self.sigma(new.reshape(-1, o, v), spin).reshape(-1, dim)])
                H = V.conj() @ AV.transpose(0, 1)
                theta, Y = torch.linalg.eigh(0.5 * (H + _dagger(H)))
                theta, Y = theta[:n_roots], Y[:, :n_guess].to(self._dt)
                Xr = Y.transpose(0, 1) @ V                                  # Ritz vectors (n_guess, dim)
                AXr = Y.transpose(0, 1) @ AV
                res = AXr[:n_roots] - theta[:, None] * Xr[:n_roots]
                norms = torch.linalg.vector_norm(res, dim=1)
                open_ = (norms >= tol).nonzero().flatten().tolist()
                if not open_ or V.shape[0] >= dim:                          # a full space ends the iteration, converged or not
                    break
                if V.shape[0] + len(open_) > max_space:                     # collapse: the Ritz vectors span the new space
                    V, AV = Xr.contiguous(), AXr.contiguous()
                added = 0
                for k in open_:
                    denom = gap - theta[k]
                    denom = torch.where(denom.abs() < 1e-8, torch.full_like(denom, 1e-8), denom)
                    t = res[k] / denom
                    for _ in range(2):                                      # two Gram-Schmidt sweeps
                        t = t - (V.conj() @ t) @ V
                    nt = float(torch.linalg.vector_norm(t).item())
                    if nt > 1e-10:
                        V = torch.cat([V, (t / nt)[None]])
                        added += 1
                if not added:
                    break
            self.residuals = [float(x) for x in norms.tolist()]
            self.converged = max(self.residuals) < tol
            X = Xr[:n_roots]
            X = X / torch.linalg.vector_norm(X, dim=1, keepdim=True)
            self._X, self.spin = X.reshape(n_roots, o, v), spin
            self.omega = _deliver(theta.contiguous(), self.system.np)
            self.X = _deliver(self._X.contiguous(), self.system.np)
        return self.omega, self.X

    def transition_dipole_moments(self):
        """``mu_n = f sum_ia X_n[i,a] x[i,a]`` for every root of the last ``solve``, (n_roots, dim), from
        ``system.position`` in the canonical orbitals: f = sqrt 2 for the singlets of a closed shell, 1 for spin
        orbitals; triplets of a closed shell carry none."""
        if self.X is None:
            raise RuntimeError("run solve() first")
        with torch._C.DisableTorchFunctionSubclass():
            x = _plain(self.system.position).to(self._dt)                   # (dim, l, l)
            x_ov = _dagger(self._Co) @ x @ self._Cv                         # (dim, o, v)
            if isinstance(self.system, GeneralOrbitalSystem):
                f = 1.0
            else:
                f = math.sqrt(2.0) if self.spin == "singlet" else 0.0
            mu = f * torch.einsum("nia,dia->nd", self._X, x_ov)
            return _deliver(mu.contiguous(), self.system.np)
