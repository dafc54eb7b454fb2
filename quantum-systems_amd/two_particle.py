"""Exact states of TWO particles in the system's basis (full configuration interaction for n = 2) on top of
``kernels.pair_contract``.

A two-particle state is an amplitude matrix ``c`` (m, m), ``|c> = sum_ab c[a,b] psi_a psi_b``, in orbitals
``psi = chi C`` with ``C^H s C = 1``.  The sigma vector of the Hamiltonian is

    T     = C c C^T                                   (AO basis; l x l products in torch)
    S     = sum_rs u[p,q,r,s] T[r,s]                  (ONE pair_contract call for all trial vectors of a step)
    sigma = ht c + c ht^T + f C^H S C^*,    ht = C^H h C

so a Davidson step reads ``u`` once per group of trial vectors and ``u`` is never transformed.

    SpatialOrbitalSystem:  singlets c = c^T, triplets c = -c^T, f = 1
    GeneralOrbitalSystem:  c = -c^T; f = 1/2 with an anti-symmetrised u, f = 1 with a plain one

``u[p,q,r,s] = <pq|rs>`` is taken to be Hermitian (as ``moller_plesset`` and ``configuration_interaction`` state).

    ci = TwoParticleCI(system)                       # or TwoParticleCI(system, C) with HF orbitals
    E, c = ci.solve(n_roots=4)                       # spin="triplet" for the triplets of spatial orbitals
"""

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


class TwoParticleCI:
    """The lowest exact states of the n = 2 particles of ``system`` by a block Davidson iteration, in the orbitals
    ``C`` (l, m) with ``C^H s C = 1`` -- Hartree-Fock orbitals, the eigenvectors of ``h`` -- or, with ``C=None``, in
    the system's own basis, which must then be orthonormal (``s = 1``)."""

    def __init__(self, system, C=None):
        refuse_vectors_only(system, "TwoParticleCI")
        if not isinstance(system, (SpatialOrbitalSystem, GeneralOrbitalSystem)):
            raise TypeError("TwoParticleCI needs a SpatialOrbitalSystem or a GeneralOrbitalSystem")
        # a SpatialOrbitalSystem counts doubly occupied orbitals (its n is half the particle number)
        particles = system.n if isinstance(system, GeneralOrbitalSystem) else 2 * system.n
        if particles != 2:
            raise ValueError(f"TwoParticleCI is the exact solution for n = 2 particles, the system has {particles}")
        if is_sharded(system.u):
            raise NotImplementedError("TwoParticleCI does not take a sharded u: the pair contraction is not sharded")
        self.system = system
        self._general = isinstance(system, GeneralOrbitalSystem)
        # an anti-symmetrised u counts every pair of the sum over (r, s) twice
        self._f = 0.5 if self._general and system._basis_set._anti_symmetrized_u else 1.0
        with torch._C.DisableTorchFunctionSubclass():
            self._u = _plain(system.u)
            h, s = _plain(system.h), _plain(system.s)
            l = h.shape[0]
            if C is None:
                eye = torch.eye(l, dtype=s.dtype, device=s.device)
                if float((s - eye).abs().max().item()) > 1e-12:
                    raise ValueError("the basis is not orthonormal (s != 1): give orbitals C with C^H s C = 1")
                C = torch.eye(l, dtype=h.dtype, device=h.device)
            else:
                C = _plain(C)
                if C.dim() != 2 or C.shape[0] != l:
                    raise ValueError(f"C must be (l, m) with l = {l}, got {tuple(C.shape)}")
            self._dt = torch.complex128 if (C.is_complex() or self._u.is_complex() or h.is_complex()) else torch.float64
            self._C = C.to(self._dt).contiguous()
            self.m = self._C.shape[1]
            ht = _dagger(self._C) @ h.to(self._dt) @ self._C
            self._ht = (0.5 * (ht + _dagger(ht))).contiguous()
            d = self._ht.diagonal().real if self._ht.is_complex() else self._ht.diagonal()
            self._diag = (d[:, None] + d[None, :]).to(torch.float64).contiguous()          # (m, m): ht_aa + ht_bb
        self.E = self.c = self.spin = None
        self.converged, self.iterations, self.residuals = False, 0, None
        self.sigma_history = []              # trial vectors sent through u, per Davidson iteration

    def _sign(self, spin):
        """+1 for the symmetric sector (c = c^T), -1 for the antisymmetric one."""
        if self._general:
            if spin != "singlet":
                raise ValueError("spin= applies to a SpatialOrbitalSystem; spin orbitals carry every multiplicity")
            return -1
        if spin == "singlet":
            return 1
        if spin == "triplet":
            return -1
        raise ValueError(f"spin must be 'singlet' or 'triplet', got {spin!r}")

    def sigma(self, c):
        """``H c_k`` (without the nuclear repulsion) for amplitudes ``c`` (k, m, m) or (m, m), device tensor in and
        out: one pass over ``u`` per group of amplitudes."""
        single = c.dim() == 2
        c = (c[None] if single else c).to(self._dt)
        C = self._C
        T = (C @ c @ C.transpose(0, 1)).contiguous()                                # (k, l, l)
        S = kernels.pair_contract(self._u, T).to(self._dt)
        out = self._ht @ c + c @ self._ht.transpose(0, 1) + self._f * (_dagger(C) @ S @ C.conj())
        return out[0] if single else out

    def solve(self, n_roots, tol=1e-9, max_iter=100, max_space=None, spin="singlet"):
        """The ``n_roots`` lowest energies of the sector and their amplitudes by a block Davidson iteration: unit guesses
        on the ``min(dim, 2 n_roots)`` lowest ``ht_aa + ht_bb`` of the sector, the diagonal preconditioner
        ``(ht_aa + ht_bb - theta)^-1``, every new vector (anti-)symmetrised and orthonormalised against the space,
        collapse to the Ritz vectors above ``max_space`` vectors.  A root is converged when its residual 2-norm is
        below ``tol``.  Returns ``(E, c)`` in the system's array module, ``E`` ascending and including the nuclear
        repulsion, ``c`` (n_roots, m, m) with unit Frobenius norm; sets ``converged``, ``iterations``, ``residuals``."""
        sign = self._sign(spin)
        m = self.m
        full = m * m
        dim = m * (m + 1) // 2 if sign > 0 else m * (m - 1) // 2
        if not 1 <= n_roots <= dim:
            raise ValueError(f"n_roots = {n_roots} does not fit the {dim} states of the sector")
        n_guess = min(dim, 2 * n_roots)
        if max_space is None:
            max_space = max(20, 10 * n_roots)
        max_space = min(dim, max(int(max_space), 2 * n_guess))

        def project(t):                                                         # onto c = sign c^T
            t = t.reshape(-1, m, m)
            return (0.5 * (t + sign * t.transpose(1, 2))).reshape(-1, full)

        with torch._C.DisableTorchFunctionSubclass():
            dev = self._diag.device
            a, b = torch.triu_indices(m, m, offset=0 if sign > 0 else 1, device=dev)
            order = torch.argsort(self._diag[a, b], stable=True)[:n_guess]
            a, b = a[order], b[order]
            V = torch.zeros(n_guess, m, m, dtype=self._dt, device=dev)
            rows = torch.arange(n_guess, device=dev)
            V[rows, a, b] += 1.0
            V[rows, b, a] += float(sign)
            V = V.reshape(n_guess, full)
            V = V / torch.linalg.vector_norm(V, dim=1, keepdim=True)
            diag = self._diag.reshape(full)
            HV = torch.empty(0, full, dtype=self._dt, device=dev)
            self.sigma_history, self.converged = [], False
            for it in range(1, max_iter + 1):
                self.iterations = it
                new = V[HV.shape[0]:]
                self.sigma_history.append(new.shape[0])
                HV = torch.cat([HV, self.sigma(new.reshape(-1, m, m)).reshape(-1, full)])
                H = V.conj() @ HV.transpose(0, 1)
                theta, Y = torch.linalg.eigh(0.5 * (H + _dagger(H)))
                theta, Y = theta[:n_roots], Y[:, :n_guess].to(self._dt)
                Xr = Y.transpose(0, 1) @ V                                      # Ritz vectors (n_guess, m m)
                HXr = Y.transpose(0, 1) @ HV
                res = HXr[:n_roots] - theta[:, None] * Xr[:n_roots]
                norms = torch.linalg.vector_norm(res, dim=1)
                open_ = (norms >= tol).nonzero().flatten().tolist()
                if not open_ or V.shape[0] >= dim:                              # a full space ends the iteration, converged or not
                    break
                if V.shape[0] + len(open_) > max_space:                         # collapse: the Ritz vectors span the new space
                    V, HV = Xr.contiguous(), HXr.contiguous()
                added = 0
                for k in open_:
                    denom = diag - theta[k]
                    denom = torch.where(denom.abs() < 1e-8, torch.full_like(denom, 1e-8), denom)
                    t = project(res[k] / denom)[0]
                    t = t / torch.linalg.vector_norm(t)                         # a residual near tol is still a direction
                    for _ in range(2):                                          # two Gram-Schmidt sweeps
                        t = t - (V.conj() @ t) @ V
                    t = project(t)[0]
                    nt = float(torch.linalg.vector_norm(t).item())
                    if nt > 1e-6:                                               # what the space does not hold already
                        V = torch.cat([V, (t / nt)[None]])
                        added += 1
                if not added:
                    break
            self.residuals = [float(x) for x in norms.tolist()]
            self.converged = max(self.residuals) < tol
            X = Xr[:n_roots]
            X = X / torch.linalg.vector_norm(X, dim=1, keepdim=True)
            self._c, self.spin = X.reshape(n_roots, m, m), spin
            E = theta + float(self.system.nuclear_repulsion_energy)
            self.E = _deliver(E.contiguous(), self.system.np)
            self.c = _deliver(self._c.contiguous(), self.system.np)
        return self.E, self.c
