"""Exact states of N particles in a finite orbital basis: configuration interaction on Slater determinants with a
direct sigma kernel (``kernels.det_ci_sigma``, ``csrc/qs_det_ci.hip``).

In orbitals ``psi = chi C`` with ``C^H s C = 1`` the Hamiltonian is

    H = sum_pq ht[p,q] a+_p a_q + 1/4 sum_pqrs ut[p,q,r,s] a+_p a+_q a_s a_r,
    ht = C^H h C,    ut[p,q,r,s] = <pq|rs> - <pq|sr>  (transformed once, anti-symmetrised once)

and a state is a vector over a list of determinants, 64-bit occupation masks (bit p = orbital p occupied) in ascending
order.  The list is data: ``full_space``, ``sz_sector``, ``truncated_space`` or any subset; the Hamiltonian of a subset
is the projection of the full one.  H is never stored: a Davidson step is ONE ``det_ci_sigma`` call.

    ci = DeterminantCI(system, C)                     # a GeneralOrbitalSystem, HF orbitals; dets=None: the full space
    E, c = ci.solve(n_roots=3)
    rho = ci.one_body_density(0)                      # for system.compute_particle_density(rho, C=C)

What a solved state is good for beyond its energy comes from two reductions over the determinants,
``kernels.det_ci_transition_density1`` and ``kernels.det_ci_density2``:

    rho[q, p]       = <c_k| a+_p a_q |c_l>                   ci.transition_density(k, l)
    G[p, q, r, s]   = <c_k| a+_p a+_q a_s a_r |c_l>          ci.two_body_density(k, l)
    <c_k| H |c_l>   = sum_pq ht[p,q] rho[q,p] + 1/4 sum_pqrs ut[p,q,r,s] G[p,q,r,s]

and everything after them is an m^2- or m^4-sized contraction: ``energy_from_densities``, ``expectation_one_body``,
``transition_dipole``, ``spin_squared``, ``natural_orbitals``.
"""

import numpy
import torch

from . import kernels
from .basis_set import _deliver, _stage, refuse_vectors_only
from .general_orbital_system import GeneralOrbitalSystem
from .sharded_module import is_sharded
from .spatial_orbital_system import SpatialOrbitalSystem

M_MAX = 63          # a mask is a non-negative int64


def _plain(arr):
    return _stage(arr).as_subclass(torch.Tensor)


def _dagger(A):
    return A.conj().transpose(-2, -1)


def _check_extents(m, N):
    if not 1 <= m <= M_MAX:
        raise ValueError(f"determinants are 64-bit masks: 1 <= m <= {M_MAX} orbitals, got m = {m}")
    if not 1 <= N <= m:
        raise ValueError(f"need 1 <= N <= m particles, got N = {N}, m = {m}")


def popcounts(dets):
    """Set bits of every mask of an int64 array."""
    d = numpy.ascontiguousarray(dets, dtype=numpy.int64)
    return numpy.unpackbits(d.view(numpy.uint8).reshape(-1, 8), axis=1).sum(axis=1).astype(numpy.int64)


def full_space(m, N):
    """All C(m, N) determinants of N particles in m orbitals, ascending int64 masks."""
    m, N = int(m), int(N)
    _check_extents(m, N)
    # S(k, n): n particles in the lowest k orbitals = S(k - 1, n), then S(k - 1, n - 1) with orbital k - 1 added
    row = [numpy.zeros(1, dtype=numpy.int64)] + [numpy.zeros(0, dtype=numpy.int64)] * N
    for k in range(1, m + 1):
        top = numpy.int64(1) << numpy.int64(k - 1)
        row = [row[0]] + [numpy.concatenate([row[n], row[n - 1] | top]) for n in range(1, N + 1)]
    return row[N]


def sz_sector(m, N, two_sz):
    """The determinants of ``full_space(m, N)`` with ``n_up - n_down = two_sz``; spin orbital 2 p + sigma, sigma = 0 up."""
    dets = full_space(m, N)
    up = numpy.int64(0x5555555555555555)
    n_up = popcounts(dets & up)
    return dets[2 * n_up - int(N) == int(two_sz)]


def truncated_space(m, reference_mask, max_excitation):
    """The determinants that differ from ``reference_mask`` by at most ``max_excitation`` moved particles (2: CISD,
    3: CISDT, ...), ascending."""
    reference_mask = int(reference_mask)
    N = bin(reference_mask).count("1")
    _check_extents(int(m), N)
    if reference_mask < 0 or reference_mask >> int(m):
        raise ValueError(f"the reference {reference_mask:#x} has orbitals at or above m = {m}")
    dets = full_space(m, N)
    moved = popcounts(dets & ~numpy.int64(reference_mask))
    return dets[moved <= int(max_excitation)]


def block_davidson(sigma, diag, guesses, n_roots, tol=1e-9, max_iter=100, max_space=None):
    """The ``n_roots`` lowest eigenpairs of a Hermitian operator given as ``sigma(V) -> H V`` on row vectors (k, dim),
    with its real diagonal ``diag`` (dim,) as preconditioner, from orthonormal ``guesses`` (n_guess, dim): every step
    sends the new vectors through ``sigma`` ONCE, solves the projected problem, and adds the preconditioned residual
    ``r / (diag - theta)`` of every open root after two Gram-Schmidt sweeps; above ``max_space`` vectors the space
    collapses to its Ritz vectors.  A root is converged when its residual 2-norm is below ``tol``; a space that holds
    the whole operator ends the iteration.  Returns ``(theta, X, info)``: energies ascending, unit vectors
    (n_roots, dim), and ``info`` with ``converged``, ``iterations``, ``residuals`` and ``sigma_history`` (vectors per
    sigma call)."""
    V = guesses
    n_guess, dim = V.shape
    if not 1 <= n_roots <= n_guess:
        raise ValueError(f"n_roots = {n_roots} needs at least as many guesses, got {n_guess}")
    if max_space is None:
        max_space = max(20, 10 * n_roots)
    max_space = min(dim, max(int(max_space), 2 * n_guess))
    HV = torch.empty(0, dim, dtype=V.dtype, device=V.device)
    history, it = [], 0
    for it in range(1, max_iter + 1):
        new = V[HV.shape[0]:]
        history.append(new.shape[0])
        HV = torch.cat([HV, sigma(new)])
        H = V.conj() @ HV.transpose(0, 1)
        theta, Y = torch.linalg.eigh(0.5 * (H + _dagger(H)))
        theta, Y = theta[:n_roots], Y[:, :n_guess].to(V.dtype)
        Xr = Y.transpose(0, 1) @ V                                          # Ritz vectors (n_guess, dim)
        HXr = Y.transpose(0, 1) @ HV
        res = HXr[:n_roots] - theta[:, None] * Xr[:n_roots]
        norms = torch.linalg.vector_norm(res, dim=1)
        open_ = (norms >= tol).nonzero().flatten().tolist()
        if not open_ or V.shape[0] >= dim:
            break
        if V.shape[0] + len(open_) > max_space:
            V, HV = Xr.contiguous(), HXr.contiguous()
        added = 0
        for k in open_:
            denom = diag - theta[k]
            denom = torch.where(denom.abs() < 1e-8, torch.full_like(denom, 1e-8), denom)
            t = res[k] / denom
            t = t / torch.linalg.vector_norm(t)
            for _ in range(2):
                t = t - (V.conj() @ t) @ V
            nt = float(torch.linalg.vector_norm(t).item())
            if nt > 1e-6:                                                   # what the space does not hold already
                V = torch.cat([V, (t / nt)[None]])
                added += 1
        if not added:
            break
    residuals = [float(x) for x in norms.tolist()]
    X = Xr[:n_roots]
    X = X / torch.linalg.vector_norm(X, dim=1, keepdim=True)
    info = {"converged": max(residuals) < tol, "iterations": it, "residuals": residuals, "sigma_history": history}
    return theta, X, info


class DeterminantCI:
    """The lowest exact states of the ``system.n`` particles of a ``GeneralOrbitalSystem`` on the determinants ``dets``
    (default: the full space) in the orbitals ``C`` (l, m) with ``C^H s C = 1`` -- or, with ``C=None``, in the system's
    own basis, which must then be orthonormal."""

    def __init__(self, system, C=None, dets=None):
        refuse_vectors_only(system, "DeterminantCI")
        if isinstance(system, SpatialOrbitalSystem):
            raise TypeError("DeterminantCI works on spin orbitals: build the system with "
                            "construct_general_orbital_system() first")
        if not isinstance(system, GeneralOrbitalSystem):
            raise TypeError("DeterminantCI needs a GeneralOrbitalSystem")
        if is_sharded(system.u):
            raise NotImplementedError("DeterminantCI does not take a sharded u: the determinant kernels are not sharded")
        self.system = system
        self.N = int(system.n)
        with torch._C.DisableTorchFunctionSubclass():
            u = _plain(system.u)
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
            self.m = int(C.shape[1])
            _check_extents(self.m, self.N)
            self._dets_host = self._checked(dets)
            self.dim = int(self._dets_host.shape[0])
            self._dt = torch.complex128 if (C.is_complex() or u.is_complex() or h.is_complex()) else torch.float64
            self._C = C.to(self._dt).contiguous()
            ht = _dagger(self._C) @ h.to(self._dt) @ self._C
            self._ht = (0.5 * (ht + _dagger(ht))).contiguous()
            ut = kernels.transform_two_body(u, self._C)                    # a new tensor: system.u is left alone
            if not system._basis_set._anti_symmetrized_u:
                ut = kernels.antisymmetrize(ut, out=ut)
            self._ut = ut.to(self._dt).contiguous()
            self._dets = torch.from_numpy(self._dets_host).to(self._ut.device)
            self._diag = kernels.det_ci_diagonal(self._ht, self._ut, self._dets, self.N)
        self.E = self.c = self._c = None
        self.converged, self.iterations, self.residuals = False, 0, None
        self.sigma_history = []              # trial vectors per Davidson iteration

    def _checked(self, dets):
        if dets is None:
            return full_space(self.m, self.N)
        if isinstance(dets, torch.Tensor):
            dets = dets.detach().cpu().numpy()
        dets = numpy.asarray(dets)
        if dets.ndim != 1 or dets.size < 1 or dets.dtype.kind not in "iu":
            raise ValueError("dets must be a non-empty 1-D integer array of occupation masks")
        if dets.dtype.kind == "u" and (dets >> numpy.uint64(63)).any():
            raise ValueError("a mask has bits at or above m")
        dets = numpy.ascontiguousarray(dets, dtype=numpy.int64)
        if (dets < 0).any() or (dets >> numpy.int64(self.m)).any():
            raise ValueError(f"a mask has bits at or above m = {self.m}")
        if (numpy.diff(dets) <= 0).any():
            raise ValueError("dets must be ascending and free of duplicates")
        if (popcounts(dets) != self.N).any():
            raise ValueError(f"every mask must have exactly N = {self.N} bits set")
        return dets

    @property
    def dets(self):
        """The determinant list, ascending int64 masks (host array)."""
        return self._dets_host

    def sigma(self, c):
        """``H c_k`` (without the nuclear repulsion) for ``c`` (k, dim) or (dim,), device tensor in and out."""
        with torch._C.DisableTorchFunctionSubclass():
            return kernels.det_ci_sigma(self._ht, self._ut, self._dets, self.N, self._diag, _plain(c).to(self._dt))

    def solve(self, n_roots, tol=1e-9, max_iter=100, max_space=None):
        """The ``n_roots`` lowest energies and their vectors by ``block_davidson``: unit guesses on the
        ``min(dim, 2 n_roots)`` lowest diagonal elements.  Returns ``(E, c)`` in the system's array module, ``E``
        ascending and including the nuclear repulsion, ``c`` (n_roots, dim) of unit norm; sets ``converged``,
        ``iterations``, ``residuals`` and ``sigma_history``."""
        if not 1 <= n_roots <= self.dim:
            raise ValueError(f"n_roots = {n_roots} does not fit the {self.dim} determinants of the space")
        n_guess = min(self.dim, 2 * n_roots)
        with torch._C.DisableTorchFunctionSubclass():
            dev = self._diag.device
            order = torch.argsort(self._diag, stable=True)[:n_guess]
            V = torch.zeros(n_guess, self.dim, dtype=self._dt, device=dev)
            V[torch.arange(n_guess, device=dev), order] = 1.0
            theta, X, info = block_davidson(self.sigma, self._diag, V, n_roots, tol, max_iter, max_space)
            self.converged, self.iterations = info["converged"], info["iterations"]
            self.residuals, self.sigma_history = info["residuals"], info["sigma_history"]
            self._c = X.contiguous()
            E = theta + float(self.system.nuclear_repulsion_energy)
            self.E = _deliver(E.contiguous(), self.system.np)
            self.c = _deliver(self._c, self.system.np)
        return self.E, self.c

    def one_body_density(self, k=0):
        """``rho[q, p] = <c_k| a+_p a_q |c_k>`` of solved state ``k`` in the orbitals ``C``: what
        ``system.compute_particle_density(rho, C=C)`` takes."""
        if self._c is None:
            raise RuntimeError("call solve() first")
        with torch._C.DisableTorchFunctionSubclass():
            rho = kernels.det_ci_density1(self._dets, self._c[k].contiguous(), self.m, self.N)
        return _deliver(rho, self.system.np)

    # ---- densities of the solved states and what follows from them ----------------------------------------------------

    def _states(self, k, l=None):
        """Vectors k and l (default: k) of the last solve; the SAME tensor twice when they coincide."""
        if self._c is None:
            raise RuntimeError("call solve() first")
        bra = self._c[k]
        return bra, (bra if l is None or l == k else self._c[l])

    def _rho(self, k, l=None):
        bra, ket = self._states(k, l)
        return kernels.det_ci_transition_density1(self._dets, bra, ket, self.m, self.N)

    def _gamma2(self, k, l=None):
        bra, ket = self._states(k, l)
        return kernels.det_ci_density2(self._dets, bra, ket, self.m, self.N)

    def _in_orbitals(self, A):
        """``C^H A C`` of a matrix (l, l) or a stack (d, l, l) given in the system's basis."""
        A = _plain(A)
        if A.dim() not in (2, 3) or tuple(A.shape[-2:]) != (self._C.shape[0],) * 2:
            raise ValueError(f"need an (l, l) matrix or a (d, l, l) stack with l = {self._C.shape[0]}, got {tuple(A.shape)}")
        dt = torch.complex128 if (A.is_complex() or self._dt == torch.complex128) else torch.float64
        C = self._C.to(dt)
        return _dagger(C) @ A.to(dt) @ C

    def transition_density(self, k, l):
        """``rho[q, p] = <c_k| a+_p a_q |c_l>`` between two solved states; ``transition_density(k, k)`` has the bits of
        ``one_body_density(k)``."""
        with torch._C.DisableTorchFunctionSubclass():
            rho = self._rho(k, l)
        return _deliver(rho, self.system.np)

    def two_body_density(self, k=0, l=None):
        """``G[p, q, r, s] = <c_k| a+_p a+_q a_s a_r |c_l>`` (m, m, m, m) of solved state ``k``, or between ``k`` and
        ``l``: anti-symmetric in (p, q) and in (r, s) exactly, one ``det_ci_density2`` call."""
        with torch._C.DisableTorchFunctionSubclass():
            G = self._gamma2(k, l)
        return _deliver(G, self.system.np)

    def energy_from_densities(self, k=0):
        """``sum ht[p,q] rho[q,p] + 1/4 sum ut[p,q,r,s] G[p,q,r,s]`` plus the nuclear repulsion: the Rayleigh quotient of
        the stored (unit) vector ``k`` -- not the Ritz value ``E[k]``, from which it differs by the square of the
        residual -- without the sigma kernel."""
        with torch._C.DisableTorchFunctionSubclass():
            rho, G = self._rho(k), self._gamma2(k)
            e = (self._ht * rho.transpose(0, 1)).sum() + 0.25 * (self._ut * G).sum()
            return float(e.real.item()) + float(self.system.nuclear_repulsion_energy)

    def expectation_one_body(self, A, k=0, l=None):
        """``<c_k| A |c_l>`` (``l`` defaults to ``k``) of a one-body operator given in the system's basis as a matrix
        (l, l) or a stack (d, l, l): ``sum_pq (C^H A C)[p,q] rho[q,p]``, one value or d of them."""
        with torch._C.DisableTorchFunctionSubclass():
            At = self._in_orbitals(A)
            rho = self._rho(k, l)
            value = (At * rho.transpose(0, 1).to(At.dtype)).sum(dim=(-2, -1))
        return _deliver(value, self.system.np)

    def transition_dipole(self, k, l):
        """``<c_k| dipole_moment |c_l>``, one value per spatial dimension."""
        return self.expectation_one_body(self.system.dipole_moment, k, l)

    def spin_squared(self, k=0):
        """``<c_k| S^2 |c_k>`` from the densities: the one-body part ``spin_2`` and the two-body part
        ``sum_i S_i[p,r] S_i[q,s] a+_p a+_q a_s a_r`` (coefficient 1: the product is not anti-symmetrised), with the
        spin matrices taken to the orbitals ``C``; ``spin_2_tb`` is never built."""
        if self._c is None:
            raise RuntimeError("call solve() first")
        spins = [getattr(self.system, name, None) for name in ("spin_x", "spin_y", "spin_z", "spin_2")]
        if any(a is None for a in spins):
            raise ValueError("the system has no spin matrices: build it with construct_general_orbital_system()")
        with torch._C.DisableTorchFunctionSubclass():
            st = self._in_orbitals(torch.stack([_plain(a).to(torch.complex128) for a in spins[:3]]))
            s2 = self._in_orbitals(_plain(spins[3]).to(torch.complex128))
            rho, G = self._rho(k).to(st.dtype), self._gamma2(k).to(st.dtype)
            one = (s2 * rho.transpose(0, 1)).sum()
            half = torch.einsum("ipr,pqrs->iqs", st, G)
            return float((one + (st * half).sum()).real.item())

    def natural_orbitals(self, k=0):
        """``(n, C_nat)`` of solved state ``k``: the occupations ``n`` (descending eigenvalues of the Hermitian part of
        the matrix ``rho[q, p]``) and ``C_nat = C U`` with its eigenvectors as columns; in ``C_nat`` the one-body
        density of the state is ``diag(n)``."""
        with torch._C.DisableTorchFunctionSubclass():
            rho = self._rho(k)
            n, U = torch.linalg.eigh(0.5 * (rho + _dagger(rho)))
            n, U = n.flip(0).contiguous(), U.flip(1)
            C_nat = (self._C @ U.to(self._dt)).contiguous()
        return _deliver(n, self.system.np), _deliver(C_nat, self.system.np)
