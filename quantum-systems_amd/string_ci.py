"""Exact states of a ``SpatialOrbitalSystem``: spin-free configuration interaction on alpha and beta occupation strings
(Knowles-Handy) with the two-body part of ``H c`` as ONE dense product (``kernels.string_ci_sigma``,
``csrc/qs_string_ci.hip``).

In orbitals ``psi = chi C`` with ``C^H s C = 1`` and ``E_pq = sum_spin a+_p,spin a_q,spin``

    H = sum_pr k[p,r] E_pr + sum_(pr),(qs) W[(pr),(qs)] E_pr E_qs,
    k[p,r] = ht[p,r] - 1/2 sum_q ut[p,q,q,r],     W[(pr),(qs)] = 1/2 ut[p,q,r,s],
    ht = C^H h C,     ut = <pq|rs> in the orbitals C (NOT anti-symmetrised, never spin-doubled)

and a state is ``c[Ia, Ib]`` over a list of alpha and a list of beta strings: ascending 64-bit masks over the m <= 63
SPATIAL orbitals with ``n_up`` and ``n_down`` bits.  The determinant is all alpha creators first, ascending within each
spin.  The lists are data (default: all of them); a replacement whose target string is missing contributes nothing.

    ci = StringCI(system, C)                          # a SpatialOrbitalSystem, e.g. RHF orbitals: hf.string_ci()
    E, c = ci.solve(n_roots=3)                        # c: (n_roots, na, nb)
    rho = ci.one_body_density(0)                      # spin-summed, for system.compute_particle_density(rho, C=C)
    masks, v = ci.to_determinants(c[0])               # the same state in DeterminantCI's convention
    G = ci.two_body_density(0)                        # spin-summed, ci.energy_from_densities(0) == E[0]
    S2 = ci.spin_squared(0)                           # S (S + 1): which root is a singlet, which a triplet
    ci = StringCI(system, C, spin_parity=+1)          # n_up == n_down: the states with c = +c^T, even S (singlets, ...)
    E, c = ci.solve(n_roots=4)                        # spin_parity=-1: odd S (triplets, ...)

A vector whose expanded intermediate is over ``kernels.STRING_CI_BYTES`` goes through sigma in passes over alpha rows,
and its one-body quantities come from the pass-wise ``kernels.string_ci_density2``: the largest state is set by the
vectors themselves.

With ``n_up == n_down`` and one string list for both spins the transposition ``(P c)[Ia, Ib] = c[Ib, Ia]`` commutes with
``H`` and ``S^2``, and in this determinant convention a state of spin ``S`` has ``c = (-1)^S c^T``.  ``spin_parity = +-1``
keeps ``solve`` inside that subspace -- the lowest singlets (and quintets, ...) or the lowest triplets alone -- and sends
every ``H c`` through ``kernels.string_ci_sigma_sym``, which forms only the lower triangle of the intermediate.

Where the up and the down particles are comes from ``kernels.string_ci_density2_spin``, the same passes with the alpha and
the beta replacement kept apart:

    rho_a, rho_b = ci.one_body_density_spin(0)        # rho_a + rho_b == ci.one_body_density(0)
    Gaa, Gab, Gbb = ci.two_body_density_spin(0)       # Gamma^ba[p,q,r,s] = Gab[q,p,s,r]; the four add up to G
    M = ci.pair_density_matrix(phi0, 0, spins="ab")   # up density given a down particle where the orbitals take phi0

A one-body operator on a state is one gather through the tables (``kernels.string_ci_one_body``, no intermediate), and the
response of a state to it a Lanczos recurrence on ``H`` from ``(A - <A>) c`` (``response.lanczos``), three vectors of memory:

    phi = ci.apply_one_body(A, c)                     # A (l, l) or (d, l, l) in the system's basis; A_down= for the other spin
    S = ci.spectral_function(A, k=0, n_steps=64)      # response.SpectralFunction: S.poles, S.weights, S.moment(p), S.response(w)
    Sx, Sy = ci.dipole_spectrum(0)                    # one per spatial dimension: the dipole absorption lines
    a = ci.polarizability(0.0)                        # alpha_xx(omega) per dimension

Removing or adding a particle is one gather through a ladder table between the string lists of two sectors
(``kernels.string_ci_ladder``); the neighbouring sector shares the transformed integrals, and a Lanczos recurrence on its
``H`` gives ionisation energies, affinities and the one-particle Green's function.  ``v`` holds coefficients in the orbitals
``C``:

    ion = ci.neighbour(d_up=-1)                       # the StringCI of (n_up - 1, n_down): no transform is repeated
    phi = ci.annihilate(v, c, spin="up")              # sum_p v[p] a_p c on the lists of ion; ci.create(...) likewise
    S = ci.removal_spectrum(v, k=0, n_steps=64)       # poles E_j(N - 1) - E_k(N), weights |<j| a(v) |Psi_k>|^2
    A = ci.addition_spectrum(v)                       # poles E_j(N + 1) - E_k(N)
    G = ci.green_function(omega, v, eta=0.05)         # retarded G_vv(omega)
    ion.solve(4); g, orbitals = ci.dyson_orbitals(ion)   # g[j, p] = <Psi_j(ion)| a_p |Psi_0>, pole strengths sum_p |g|^2

Out of scope here: full spin adaptation (``S = 0`` apart from ``S = 2``), a sharded ``u`` (refused in the constructor), the
off-diagonal polarizability ``alpha_xy`` and the off-diagonal ``G_vw`` (they need a block recurrence), and the same calls on
``DeterminantCI``.
"""

import weakref

import numpy
import torch

from . import kernels, response
from .basis_set import _deliver, refuse_vectors_only
from .determinant_ci import M_MAX, _dagger, _plain, block_davidson, full_space, popcounts
from .general_orbital_system import GeneralOrbitalSystem
from .sharded_module import is_sharded
from .spatial_orbital_system import SpatialOrbitalSystem


def full_strings(m, N):
    """All C(m, N) occupation strings of N particles of one spin in m spatial orbitals, ascending int64 masks; ``N = 0``
    is the single empty string ``[0]``."""
    m, N = int(m), int(N)
    if not 1 <= m <= M_MAX:
        raise ValueError(f"strings are 64-bit masks: 1 <= m <= {M_MAX} orbitals, got m = {m}")
    if not 0 <= N <= m:
        raise ValueError(f"need 0 <= N <= m particles of one spin, got N = {N}, m = {m}")
    return numpy.zeros(1, dtype=numpy.int64) if N == 0 else full_space(m, N)


def checked_strings(strings, m, N):
    """``strings`` as an ascending, duplicate-free int64 array of masks with ``N`` bits below ``m`` (``None``: all)."""
    if strings is None:
        return full_strings(m, N)
    full_strings(m, 0)                                              # the extents of m
    if isinstance(strings, torch.Tensor):
        strings = strings.detach().cpu().numpy()
    strings = numpy.asarray(strings)
    if strings.ndim != 1 or strings.size < 1 or strings.dtype.kind not in "iu":
        raise ValueError("a string list must be a non-empty 1-D integer array of occupation masks")
    if strings.dtype.kind == "u" and (strings >> numpy.uint64(63)).any():
        raise ValueError("a mask has bits at or above m")
    strings = numpy.ascontiguousarray(strings, dtype=numpy.int64)
    if (strings < 0).any() or (strings >> numpy.int64(m)).any():
        raise ValueError(f"a mask has bits at or above m = {m}")
    if (numpy.diff(strings) <= 0).any():
        raise ValueError("a string list must be ascending and free of duplicates")
    if (popcounts(strings) != int(N)).any():
        raise ValueError(f"every mask must have exactly N = {N} bits set")
    return strings


def _spread(strings):
    """Bit p of every mask moved to bit 2 p."""
    out = numpy.zeros_like(strings)
    for p in range(32):
        out |= ((strings >> numpy.int64(p)) & numpy.int64(1)) << numpy.int64(2 * p)
    return out


def determinant_order(strings_up, strings_down):
    """``(masks, perm, phase)`` that take a vector over ``(Ia, Ib)`` to ``DeterminantCI``'s convention -- spin orbital
    ``2 p + sigma`` with alpha = 0, ascending interleaved masks --: ``v = (phase * c.reshape(-1))[perm]`` belongs to
    ``masks``.  ``phase[Ia, Ib] = (-1)^(sum_{q in Ib} #{p in Ia : p > q})`` takes "all alpha creators first" to ascending
    spin orbitals."""
    sa = numpy.ascontiguousarray(strings_up, dtype=numpy.int64)
    sb = numpy.ascontiguousarray(strings_down, dtype=numpy.int64)
    if (sa >> numpy.int64(31)).any() or (sb >> numpy.int64(31)).any():
        raise ValueError("interleaved determinants are 64-bit masks over 2 m <= 62 spin orbitals: m <= 31")
    masks = (_spread(sa)[:, None] | (_spread(sb)[None, :] << numpy.int64(1))).reshape(-1)
    swaps = numpy.zeros((len(sa), len(sb)), dtype=numpy.int64)
    for q in range(31):
        above = popcounts(sa >> numpy.int64(q + 1))                  # alpha particles in orbitals p > q
        swaps += above[:, None] * ((sb >> numpy.int64(q)) & numpy.int64(1))[None, :]
    phase = numpy.where(swaps & 1, -1.0, 1.0).reshape(-1)
    perm = numpy.argsort(masks, kind="stable")
    return masks[perm], perm, phase


class StringCI:
    """The lowest exact states of ``n_up`` alpha and ``n_down`` beta particles (default: ``system.n`` each) of a
    ``SpatialOrbitalSystem`` on the string lists ``strings_up`` x ``strings_down`` (default: all strings) in the
    orbitals ``C`` (l, m) with ``C^H s C = 1`` -- or, with ``C=None``, in the system's own basis, which must then be
    orthonormal.  ``ht``, ``ut``, ``k``, ``W``, the replacement tables and the diagonal are built once, here.
    ``spin_parity`` = +1 or -1 (needs ``n_up == n_down`` and equal string lists) restricts ``sigma`` and ``solve`` to the
    vectors with ``c = spin_parity * c^T``: the states of even or of odd spin ``S``."""

    def __init__(self, system, C=None, n_up=None, n_down=None, strings_up=None, strings_down=None, spin_parity=None):
        refuse_vectors_only(system, "StringCI")
        if isinstance(system, GeneralOrbitalSystem):
            raise TypeError("StringCI works on spatial orbitals: a GeneralOrbitalSystem goes to DeterminantCI")
        if not isinstance(system, SpatialOrbitalSystem):
            raise TypeError("StringCI needs a SpatialOrbitalSystem")
        if is_sharded(system.u):
            raise NotImplementedError("StringCI does not take a sharded u: the string kernels are not sharded")
        n_up = int(system.n if n_up is None else n_up)
        n_down = int(system.n if n_down is None else n_down)
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
            m = int(C.shape[1])
            sa_host = checked_strings(strings_up, m, n_up)
            sb_host = sa_host if (strings_down is strings_up and n_down == n_up) else checked_strings(strings_down, m, n_down)
            self._set_lists(n_up, n_down, sa_host, sb_host, spin_parity)
            dt = torch.complex128 if (C.is_complex() or u.is_complex() or h.is_complex()) else torch.float64
            C = C.to(dt).contiguous()
            ht = _dagger(C) @ h.to(dt) @ C
            ht = (0.5 * (ht + _dagger(ht))).contiguous()
            ut = kernels.transform_two_body(u, C).to(dt).contiguous()                       # a new tensor: system.u is left alone
            k = (ht - 0.5 * torch.einsum("pqqr->pr", ut)).contiguous()
            W = (0.5 * ut.permute(0, 2, 1, 3)).reshape(m * m, m * m).contiguous()          # the one permuted, scaled copy
        self._set_integrals(system, m, dt, C, ht, ut, k, W)
        self._build()

    # What a StringCI is made of, set in three steps that ``__init__`` and ``neighbour`` share: the sector and its host lists,
    # the orbitals with the transformed integrals, and what is built from both on the device.

    def _set_lists(self, n_up, n_down, sa_host, sb_host, spin_parity):
        self.n_up, self.n_down = n_up, n_down
        self._sa_host, self._sb_host = sa_host, sb_host
        self._same = sb_host is sa_host or numpy.array_equal(sa_host, sb_host)
        self.na, self.nb = int(sa_host.shape[0]), int(sb_host.shape[0])
        self.dim = self.na * self.nb
        if spin_parity is not None:
            if spin_parity not in (1, -1):
                raise ValueError(f"spin_parity must be None, +1 or -1, got {spin_parity!r}")
            if n_up != n_down or not self._same:
                raise ValueError("a spin parity needs n_up == n_down and the same string list for both spins")
        self.spin_parity = None if spin_parity is None else int(spin_parity)

    def _set_integrals(self, system, m, dt, C, ht, ut, k, W):
        self.system, self.m, self._dt = system, m, dt
        self._C, self._ht, self._ut, self._k, self._W = C, ht, ut, k, W

    def _build(self, alpha=None, beta=None):
        """The device lists, the replacement tables and the diagonal; ``alpha`` / ``beta`` = (device list, table) of that
        spin where they exist already.  Ends with no state solved and empty caches."""
        with torch._C.DisableTorchFunctionSubclass():
            dev = self._ut.device
            if alpha is None:
                sa = torch.from_numpy(self._sa_host).to(dev)
                alpha = (sa, kernels.string_ci_table(sa, self.m, self.n_up))
            if beta is None and self._same:
                beta = alpha
            if beta is None:
                sb = torch.from_numpy(self._sb_host).to(dev)
                beta = (sb, kernels.string_ci_table(sb, self.m, self.n_down))
            (self._sa, self._ta), (self._sb, self._tb) = alpha, beta
            self._diag = kernels.string_ci_diagonal(self._ht, self._ut, self._sa, self.n_up, self._sb, self.n_down).reshape(-1)
        self.E = self.c = self._c = None
        self.converged, self.iterations, self.residuals = False, 0, None
        self.sigma_history = []              # trial vectors per Davidson iteration
        self._neighbours = {}                # (d_up, d_down) -> the StringCI of that sector on all strings
        self._ladders = {}                   # (id(other), spin, direction) -> (weak reference to other, ladder table)

    @property
    def strings_up(self):
        """The alpha string list, ascending int64 masks (host array)."""
        return self._sa_host

    @property
    def strings_down(self):
        """The beta string list, ascending int64 masks (host array)."""
        return self._sb_host

    def sigma(self, c):
        """``H c_k`` (without the nuclear repulsion) for ``c`` (k, na, nb) or (na, nb), device tensor in and out; a
        complex ``c`` on a real Hamiltonian keeps ``W`` real.  Under a ``spin_parity`` tau it is ``H`` on the part of
        ``c`` that has the parity, ``1/2 (c + tau c^T)``."""
        with torch._C.DisableTorchFunctionSubclass():
            c = _plain(c)
            if self._dt == torch.complex128:
                c = c.to(self._dt)
            if self.spin_parity is not None:
                c = 0.5 * (c + self.spin_parity * c.transpose(-1, -2))
                return kernels.string_ci_sigma_sym(self._k, self._W, self._ta, c, self.spin_parity)
            return kernels.string_ci_sigma(self._k, self._W, self._ta, self._tb, c)

    def _sigma_rows(self, V):
        return self.sigma(V.reshape(V.shape[0], self.na, self.nb)).reshape(V.shape[0], self.dim)

    def _unpack(self, P):
        """Full vectors (k, n, n) of packed ones (k, n (n + tau) / 2): the entries a > b scaled by sqrt 2 (an orthonormal
        basis of the parity subspace), then the diagonal for tau = +1."""
        n, tau = self.na, self.spin_parity
        low = torch.ones(n, n, dtype=torch.bool, device=P.device).tril(-1)
        pairs = n * (n - 1) // 2
        c = torch.zeros(P.shape[0], n, n, dtype=P.dtype, device=P.device)
        c[:, low] = P[:, :pairs] * (0.5 ** 0.5)
        c = c + tau * c.transpose(1, 2)
        if tau > 0:
            c.diagonal(dim1=1, dim2=2).copy_(P[:, pairs:])
        return c

    def _pack(self, c):
        n, tau = self.na, self.spin_parity
        low = torch.ones(n, n, dtype=torch.bool, device=c.device).tril(-1)
        parts = [c[:, low] * (2.0 ** 0.5)] + ([c.diagonal(dim1=1, dim2=2)] if tau > 0 else [])
        return torch.cat(parts, dim=1)

    def _sigma_packed(self, P):
        c = self._unpack(P).contiguous()
        return self._pack(kernels.string_ci_sigma_sym(self._k, self._W, self._ta, c, self.spin_parity))

    def _solve_parity(self, n_roots, tol, max_iter, max_space):
        n, tau = self.na, self.spin_parity
        sub = n * (n + tau) // 2
        if not 1 <= n_roots <= sub:
            raise ValueError(f"n_roots = {n_roots} does not fit the {sub} dimensions of the subspace c = {tau:+d} c^T")
        n_guess = min(sub, 2 * n_roots)
        with torch._C.DisableTorchFunctionSubclass():
            dev = self._diag.device
            d = self._diag.reshape(n, n)                                # <I|H|I> is even under the exchange of the spins
            low = torch.ones(n, n, dtype=torch.bool, device=dev).tril(-1)
            diag = torch.cat([d[low]] + ([d.diagonal()] if tau > 0 else []))
            order = torch.argsort(diag, stable=True)[:n_guess]
            V = torch.zeros(n_guess, sub, dtype=self._dt, device=dev)
            V[torch.arange(n_guess, device=dev), order] = 1.0
            theta, X, info = block_davidson(self._sigma_packed, diag, V, n_roots, tol, max_iter, max_space)
            c = self._unpack(X)
            c = c / torch.linalg.vector_norm(c.reshape(n_roots, -1), dim=1)[:, None, None]
        return theta, c.contiguous(), info

    def solve(self, n_roots, tol=1e-9, max_iter=100, max_space=None):
        """The ``n_roots`` lowest energies and their vectors by ``determinant_ci.block_davidson``: unit guesses on the
        ``min(dim, 2 n_roots)`` lowest diagonal elements.  Returns ``(E, c)`` in the system's array module, ``E``
        ascending and including the nuclear repulsion, ``c`` (n_roots, na, nb) of unit norm; sets ``converged``,
        ``iterations``, ``residuals`` and ``sigma_history``.  Under a ``spin_parity`` tau the iteration runs unchanged in
        packed coordinates of the subspace ``c = tau c^T`` (dimension ``n (n + tau) / 2``, the packed diagonal as
        preconditioner): the lowest states of even (tau = +1) or odd (tau = -1) spin."""
        if self.spin_parity is not None:
            theta, c, info = self._solve_parity(n_roots, tol, max_iter, max_space)
            with torch._C.DisableTorchFunctionSubclass():
                self.converged, self.iterations = info["converged"], info["iterations"]
                self.residuals, self.sigma_history = info["residuals"], info["sigma_history"]
                self._c = c
                E = theta + float(self.system.nuclear_repulsion_energy)
                self.E = _deliver(E.contiguous(), self.system.np)
                self.c = _deliver(self._c, self.system.np)
            return self.E, self.c
        if not 1 <= n_roots <= self.dim:
            raise ValueError(f"n_roots = {n_roots} does not fit the {self.dim} determinants of the space")
        n_guess = min(self.dim, 2 * n_roots)
        with torch._C.DisableTorchFunctionSubclass():
            dev = self._diag.device
            order = torch.argsort(self._diag, stable=True)[:n_guess]
            V = torch.zeros(n_guess, self.dim, dtype=self._dt, device=dev)
            V[torch.arange(n_guess, device=dev), order] = 1.0
            theta, X, info = block_davidson(self._sigma_rows, self._diag, V, n_roots, tol, max_iter, max_space)
            self.converged, self.iterations = info["converged"], info["iterations"]
            self.residuals, self.sigma_history = info["residuals"], info["sigma_history"]
            self._c = X.reshape(n_roots, self.na, self.nb).contiguous()
            E = theta + float(self.system.nuclear_repulsion_energy)
            self.E = _deliver(E.contiguous(), self.system.np)
            self.c = _deliver(self._c, self.system.np)
        return self.E, self.c

    def _rho(self, k, l=None):
        if self._c is None:
            raise RuntimeError("call solve() first")
        bra = self._c[k]
        ket = bra if l is None or l == k else self._c[l]
        if kernels.string_ci_sigma_plan(self.m, self.na, self.nb, self._dt)[1] > 1:
            # a state that sigma reaches in passes: the pass-wise route, whose panels stay within the budget
            return kernels.string_ci_density2(self._ta, self._tb, self.m, bra, ket)[1]
        return kernels.string_ci_density1(self._ta, self._tb, self.m, bra, ket)

    def one_body_density(self, k=0):
        """Spin-summed ``rho[q, p] = <c_k| E_pq |c_k>`` of solved state ``k`` in the orbitals ``C``: what
        ``system.compute_particle_density(rho, C=C)`` takes."""
        with torch._C.DisableTorchFunctionSubclass():
            rho = self._rho(k)
        return _deliver(rho, self.system.np)

    def transition_density(self, k, l):
        """Spin-summed ``rho[q, p] = <c_k| E_pq |c_l>`` between two solved states."""
        with torch._C.DisableTorchFunctionSubclass():
            rho = self._rho(k, l)
        return _deliver(rho, self.system.np)

    def _pair(self, k, l=None):
        if self._c is None:
            raise RuntimeError("call solve() first")
        bra = self._c[k]
        return bra, (bra if l is None or l == k else self._c[l])

    def two_body_density(self, k=0, l=None):
        """Spin-summed ``Gamma[p,q,r,s] = sum_spins <c_k| a+_p a+_q a_s a_r |c_l>`` (m, m, m, m) in the orbitals ``C``
        (``l`` defaults to ``k``: the density of solved state ``k``), on ``kernels.string_ci_density2``.  Symmetries:
        ``Gamma[p,q,r,s] = Gamma[q,p,s,r]``; for a state it is Hermitian, ``Gamma[p,q,r,s] = conj(Gamma[r,s,p,q])``;
        ``sum_q Gamma[p,q,r,q] = (N - 1) rho[r,p]`` with ``rho`` of ``one_body_density`` / ``transition_density`` and
        ``N = n_up + n_down``, so ``sum_pq Gamma[p,q,p,q] = N (N - 1)`` for a state and 0 between two of them."""
        with torch._C.DisableTorchFunctionSubclass():
            gamma, _ = kernels.string_ci_density2(self._ta, self._tb, self.m, *self._pair(k, l))
        return _deliver(gamma, self.system.np)

    def energy_from_densities(self, k=0):
        """``sum ht[p,q] rho[q,p] + 1/2 sum ut[p,q,r,s] Gamma[p,q,r,s] + nuclear repulsion`` of solved state ``k``
        (real part): the factor is 1/2 with the plain ``ut``, where ``DeterminantCI`` has 1/4 with the anti-symmetrised
        one.  Equals ``E[k]`` to the accuracy of the state."""
        with torch._C.DisableTorchFunctionSubclass():
            gamma, rho = kernels.string_ci_density2(self._ta, self._tb, self.m, *self._pair(k))
            e = (self._ht * rho.transpose(0, 1)).sum() + 0.5 * (self._ut * gamma).sum()
            return float(e.real.item()) + float(self.system.nuclear_repulsion_energy)

    def _spin_blocks(self, k, l=None):
        return kernels.string_ci_density2_spin(self._ta, self._tb, self.m, *self._pair(k, l))

    def one_body_density_spin(self, k=0, l=None):
        """``(rho_a, rho_b)``, ``rho_s[q, p] = <c_k| a+_ps a_qs |c_l>`` (``l`` defaults to ``k``) in the orbitals ``C``, each
        in the index order of ``one_body_density``; they add up to it."""
        with torch._C.DisableTorchFunctionSubclass():
            blocks = self._spin_blocks(k, l)
        return tuple(_deliver(x, self.system.np) for x in blocks[3:])

    def spin_density(self, k=0):
        """``rho_a - rho_b`` of solved state ``k``, in the index order ``system.compute_particle_density(rho, C=C)``
        takes; its trace is ``n_up - n_down``."""
        with torch._C.DisableTorchFunctionSubclass():
            blocks = self._spin_blocks(k)
            rho = blocks[3] - blocks[4]
        return _deliver(rho, self.system.np)

    def two_body_density_spin(self, k=0, l=None):
        """``(Gamma_aa, Gamma_ab, Gamma_bb)``, ``Gamma_st[p,q,r,s] = <c_k| a+_ps a+_qt a_st a_rs |c_l>`` (m, m, m, m) in the
        orbitals ``C`` (``l`` defaults to ``k``), on ``kernels.string_ci_density2_spin``.  The beta-alpha block is
        ``Gamma_ab[q,p,s,r]``; the four add up to ``two_body_density``.  ``Gamma_aa`` and ``Gamma_bb`` change sign under
        ``p <-> q`` and under ``r <-> s``; ``sum_q Gamma_st[p,q,r,q] = (N_t - delta_st) rho_s[r,p]``."""
        with torch._C.DisableTorchFunctionSubclass():
            blocks = self._spin_blocks(k, l)
        return tuple(_deliver(x, self.system.np) for x in blocks[:3])

    def spin_squared_from_densities(self, k=0):
        """``<S^2> = S_z (S_z + 1) + N_b - sum_pq Gamma_ab[q,p,p,q]`` of solved state ``k`` (real part), read off the
        opposite-spin pair density; equals ``spin_squared(k)`` to rounding."""
        with torch._C.DisableTorchFunctionSubclass():
            gab = self._spin_blocks(k)[1]
            sz = 0.5 * (self.n_up - self.n_down)
            return sz * (sz + 1.0) + self.n_down - float(torch.einsum("qppq->", gab).real.item())

    def natural_spin_orbitals(self, k=0):
        """``(n_a, C_a, n_b, C_b)`` of solved state ``k``: per spin the occupations (descending eigenvalues of the
        Hermitian part of ``rho_s[q, p]``, between 0 and 1) and ``C_s = C U_s`` with its eigenvectors as columns."""
        out = []
        with torch._C.DisableTorchFunctionSubclass():
            for rho in self._spin_blocks(k)[3:]:
                n, U = torch.linalg.eigh(0.5 * (rho + _dagger(rho)))
                out += [n.flip(0).contiguous(), (self._C @ U.flip(1).to(self._dt)).contiguous()]
        return tuple(_deliver(x, self.system.np) for x in out)

    def pair_density_matrix(self, phi0, k=0, spins="ab"):
        """``M[r, p] = sum_qs Gamma_st[p,q,r,s] conj(phi0[q]) phi0[s]`` of solved state ``k``, with ``phi0`` the m values
        of the orbitals ``C`` at a reference point: ``system.compute_particle_density(M, C=C)`` is the density of s
        particles given a t particle at that point (the conditional density up to the density at the point).  ``spins``
        = ``"aa"``, ``"ab"``, ``"ba"``, ``"bb"`` names ``st``; ``"sum"`` adds the four."""
        if spins not in ("aa", "ab", "ba", "bb", "sum"):
            raise ValueError(f"spins must be one of 'aa', 'ab', 'ba', 'bb', 'sum', got {spins!r}")
        with torch._C.DisableTorchFunctionSubclass():
            gaa, gab, gbb = self._spin_blocks(k)[:3]
            phi = torch.as_tensor(phi0, device=gaa.device) if not isinstance(phi0, torch.Tensor) else _plain(phi0).to(gaa.device)
            if tuple(phi.shape) != (self.m,):
                raise ValueError(f"phi0 must hold the m = {self.m} orbital values at the reference point, got {tuple(phi.shape)}")
            dt = torch.complex128 if (phi.is_complex() or self._dt == torch.complex128) else torch.float64
            phi = phi.to(dt)
            gba = gab.permute(1, 0, 3, 2)
            gamma = {"aa": gaa, "ab": gab, "ba": gba, "bb": gbb}.get(spins)
            if gamma is None:
                gamma = gaa + gbb + gab + gba
            M = torch.einsum("pqrs,q,s->rp", gamma.to(dt), phi.conj(), phi).contiguous()
        return _deliver(M, self.system.np)

    def apply_spin_squared(self, c):
        """``S^2 c_k`` for ``c`` (k, na, nb) or (na, nb), device tensor in and out
        (``kernels.string_ci_spin_squared``).  On truncated string lists a missing target contributes nothing: ``S^2``
        is then the operator of the truncated formulation, as ``H`` is."""
        with torch._C.DisableTorchFunctionSubclass():
            c = _plain(c)
            if tuple(c.shape[-2:]) != (self.na, self.nb) or c.dim() not in (2, 3):
                raise ValueError(f"c has shape {tuple(c.shape)}: need (k, {self.na}, {self.nb}) or ({self.na}, {self.nb})")
            return kernels.string_ci_spin_squared(self._ta, self._tb, self.m, self.n_up, self.n_down, c)

    def spin_squared(self, k=0):
        """``Re <c_k| S^2 |c_k>`` of solved state ``k``: ``S (S + 1)`` for a spin eigenstate."""
        with torch._C.DisableTorchFunctionSubclass():
            bra, _ = self._pair(k)
            return float(torch.vdot(bra.reshape(-1), self.apply_spin_squared(bra).reshape(-1)).real.item())

    def spin_multiplicity(self, k=0):
        """``2 S + 1 = sqrt(1 + 4 <S^2>)`` of solved state ``k``."""
        return float(numpy.sqrt(max(0.0, 1.0 + 4.0 * self.spin_squared(k))))

    def _in_orbitals(self, A):
        """``C^H A C`` of a matrix (l, l) or a stack (d, l, l) given in the system's basis."""
        A = _plain(A)
        if A.dim() not in (2, 3) or tuple(A.shape[-2:]) != (self._C.shape[0],) * 2:
            raise ValueError(f"need an (l, l) matrix or a (d, l, l) stack with l = {self._C.shape[0]}, got {tuple(A.shape)}")
        dt = torch.complex128 if (A.is_complex() or self._dt == torch.complex128) else torch.float64
        C = self._C.to(dt)
        return _dagger(C) @ A.to(dt) @ C

    def expectation_one_body(self, A, k=0, l=None):
        """``<c_k| A |c_l>`` (``l`` defaults to ``k``) of a spin-free one-body operator given in the system's basis as a
        matrix (l, l) or a stack (d, l, l): ``sum_pq (C^H A C)[p,q] rho[q,p]``, one value or d of them."""
        with torch._C.DisableTorchFunctionSubclass():
            At = self._in_orbitals(A)
            rho = self._rho(k, l)
            value = (At * rho.transpose(0, 1).to(At.dtype)).sum(dim=(-2, -1))
        return _deliver(value, self.system.np)

    def transition_dipole(self, k, l):
        """``<c_k| dipole_moment |c_l>``, one value per spatial dimension."""
        return self.expectation_one_body(self.system.dipole_moment, k, l)

    def _vectors_checked(self, c, what):
        c = _plain(c)
        if c.dim() not in (2, 3) or tuple(c.shape[-2:]) != (self.na, self.nb):
            raise ValueError(f"{what} has shape {tuple(c.shape)}: need (k, {self.na}, {self.nb}) or ({self.na}, {self.nb})")
        return c

    def apply_one_body(self, A, c, A_down=None):
        """``A c_k`` for ``c`` (k, na, nb) or (na, nb), device tensor in and out (``kernels.string_ci_one_body``): ``A`` is a
        matrix (l, l) or a stack (d, l, l) in the system's basis, as in ``expectation_one_body``, and acts as
        ``sum_pq (C^H A C)[p,q] E_pq``; the result has the leading axis of ``A`` (if present), then that of ``c``.  With
        ``A_down`` the up particles see ``A`` and the down particles ``A_down``.  Under a ``spin_parity`` only the spin-free
        form is taken (it commutes with the transposition, so the result keeps the parity)."""
        with torch._C.DisableTorchFunctionSubclass():
            c = self._vectors_checked(c, "c")
            if A_down is not None and self.spin_parity is not None:
                raise ValueError("under a spin parity the operator must be spin-free: A_down would leave the subspace")
            At = self._in_orbitals(A)
            Ad = None if A_down is None else self._in_orbitals(A_down)
            if Ad is not None and tuple(Ad.shape) != tuple(At.shape):
                raise ValueError(f"A_down has shape {tuple(Ad.shape)}: need that of A, {tuple(At.shape)}")
            return kernels.string_ci_one_body(At, self._ta, self._tb, self.m, c, A_down=Ad)

    def _reference(self, k, state):
        """``(c, energy)`` a spectrum starts from: solved state ``k`` and ``E[k]`` without the nuclear repulsion, or the
        given vector (na, nb), normalised, with ``Re <c|H c>`` from one ``sigma``."""
        if state is None:
            if self._c is None:
                raise RuntimeError("call solve() first, or give state=")
            return self._c[k], float(self.E[k]) - float(self.system.nuclear_repulsion_energy)
        c = _plain(state)
        if tuple(c.shape) != (self.na, self.nb):
            raise ValueError(f"state has shape {tuple(c.shape)}: need ({self.na}, {self.nb})")
        c = c.to(self._dt) if self._dt == torch.complex128 else c
        c = (c / torch.linalg.vector_norm(c)).contiguous()
        return c, float(torch.vdot(c.reshape(-1), self.sigma(c).to(c.dtype).reshape(-1)).real.item())

    def spectral_function(self, A, k=0, n_steps=64, A_down=None, reorthogonalize=False, beta_tol=0.0, state=None):
        """The ``response.SpectralFunction`` of ONE one-body operator ``A`` (l, l) on solved state ``k`` -- or, with
        ``state=``, on a given vector (na, nb), which is normalised here and whose energy is ``Re <c|H c>`` from one
        ``sigma`` (no ``solve()`` needed) --: ``n_steps`` of ``response.lanczos`` on ``H`` from
        ``phi = A c - <c|A c> c``.  Poles are excitation energies ``E_j - E_k`` (the nuclear repulsion cancels), weights
        ``|<j|A|c>|^2``; ``phi = 0`` gives the empty spectrum.  ``reorthogonalize`` and ``beta_tol`` as in
        ``response.lanczos``."""
        with torch._C.DisableTorchFunctionSubclass():
            if _plain(A).dim() != 2 or (A_down is not None and _plain(A_down).dim() != 2):
                raise ValueError("spectral_function takes ONE operator (l, l): a stack goes operator by operator")
            c, energy = self._reference(k, state)
            Ac = self.apply_one_body(A, c, A_down)
            c = c.to(Ac.dtype)
            phi = Ac - torch.vdot(c.reshape(-1), Ac.reshape(-1)) * c
            alpha, beta, norm2 = response.lanczos(self._sigma_rows, phi.reshape(1, self.dim), n_steps, reorthogonalize, beta_tol)
        return response.SpectralFunction(alpha, beta, norm2, energy)

    def dipole_spectrum(self, k=0, n_steps=64, **kw):
        """One ``response.SpectralFunction`` per spatial dimension of ``system.dipole_moment`` on solved state ``k``: the
        dipole absorption lines and their weights (``kw``: ``reorthogonalize``, ``beta_tol``, ``state``)."""
        return [self.spectral_function(x, k, n_steps, **kw) for x in _plain(self.system.dipole_moment)]

    def polarizability(self, omega, k=0, n_steps=64, eta=0.0, **kw):
        """The diagonal dynamic polarizability ``alpha_xx(omega)`` per spatial dimension, (dims,) + the shape of
        ``omega``, from ``dipole_spectrum``: ``sum_j w_j (1 / (omega_j - omega - i eta) + 1 / (omega_j + omega + i eta))``;
        real for ``eta == 0``."""
        value = numpy.stack([numpy.asarray(S.response(omega, eta)) for S in self.dipole_spectrum(k, n_steps, **kw)])
        with torch._C.DisableTorchFunctionSubclass():
            value = torch.from_numpy(numpy.ascontiguousarray(value)).to(self._ta.device)
        return _deliver(value, self.system.np)

    def neighbour(self, d_up=0, d_down=0, strings=None):
        """The ``StringCI`` of ``(n_up + d_up, n_down + d_down)`` particles in the same orbitals, exactly one of the two
        steps being +1 or -1.  It shares ``C``, ``ht``, ``ut``, ``k`` and ``W`` with this one (no transform is repeated) and
        keeps the string list and the table of the unchanged spin; the changed spin takes ``strings`` (default: all).  It
        has no spin parity.  Without ``strings`` it is built once per ``(d_up, d_down)``."""
        d_up, d_down = int(d_up), int(d_down)
        if sorted((abs(d_up), abs(d_down))) != [0, 1]:
            raise ValueError(f"exactly one of d_up, d_down must be +1 or -1, got ({d_up}, {d_down})")
        n_up, n_down = self.n_up + d_up, self.n_down + d_down
        if not (0 <= n_up <= self.m and 0 <= n_down <= self.m):
            raise ValueError(f"there is no sector of ({n_up}, {n_down}) particles in {self.m} orbitals")
        if strings is None and (d_up, d_down) in self._neighbours:
            return self._neighbours[(d_up, d_down)]
        other = object.__new__(StringCI)
        changed = checked_strings(strings, self.m, n_up if d_up else n_down)
        other._set_lists(n_up, n_down, changed if d_up else self._sa_host, self._sb_host if d_up else changed, None)
        other._set_integrals(self.system, self.m, self._dt, self._C, self._ht, self._ut, self._k, self._W)
        other._build(alpha=None if d_up else (self._sa, self._ta), beta=(self._sb, self._tb) if d_up else None)
        if strings is None:
            self._neighbours[(d_up, d_down)] = other
        return other

    def _ladder_to(self, other, spin, step):
        """``(other, spin index, table)`` of the ladder of ``spin`` from this sector to ``other`` (default: the neighbour),
        which must hold ``step`` = +1 or -1 more particles of that spin, as many of the other spin, and that spin's list."""
        if spin not in ("up", "down"):
            raise ValueError(f"spin must be 'up' or 'down', got {spin!r}")
        s = 0 if spin == "up" else 1
        if other is None:
            other = self.neighbour(d_up=step) if s == 0 else self.neighbour(d_down=step)
        key = (id(other), s, step)
        cached = self._ladders.get(key)
        if cached is not None and cached[0]() is other:
            return other, s, cached[1]
        want = (self.n_up + (step if s == 0 else 0), self.n_down + (step if s == 1 else 0))
        if not isinstance(other, StringCI) or other.m != self.m or (other.n_up, other.n_down) != want:
            raise ValueError(f"other must be a StringCI of ({want[0]}, {want[1]}) particles in the same {self.m} orbitals")
        kept = (self._sb_host, other._sb_host) if s == 0 else (self._sa_host, other._sa_host)
        if not numpy.array_equal(*kept):
            raise ValueError("other must have this sector's string list of the unchanged spin")
        target, source = (other._sa, self._sa) if s == 0 else (other._sb, self._sb)
        table = kernels.string_ci_ladder_table(target, source, self.m)
        # a weak reference: the cache keeps no sector alive, and an id that a later object took over is seen and replaced
        self._ladders = {k_: v_ for k_, v_ in self._ladders.items() if v_[0]() is not None}
        self._ladders[key] = (weakref.ref(other), table)
        return other, s, table

    def _ladder(self, v, c, spin, other, step):
        with torch._C.DisableTorchFunctionSubclass():
            c = self._vectors_checked(c, "c")
            other, s, table = self._ladder_to(other, spin, step)
            v = _plain(v)
            v = v.to(device=c.device, dtype=torch.complex128 if v.is_complex() else torch.float64)
            if v.dim() not in (1, 2) or v.shape[-1] != self.m:
                raise ValueError(f"v has shape {tuple(v.shape)}: need ({self.m},) or (d, {self.m}) coefficients in the orbitals C")
            return kernels.string_ci_ladder(v, table, s, self.n_up, c), other

    def annihilate(self, v, c, spin="up", other=None):
        """``sum_p v[p] a_p,spin c_k`` for ``c`` (k, na, nb) or (na, nb), device tensor in and out
        (``kernels.string_ci_ladder``): ``v`` (m,) or (d, m) holds coefficients in the orbitals ``C`` and is not conjugated;
        the result lives on the string lists of ``other`` (default: ``neighbour`` with one particle of ``spin`` less) and
        has the leading axis of ``v`` (if present), then that of ``c``."""
        return self._ladder(v, c, spin, other, -1)[0]

    def create(self, v, c, spin="up", other=None):
        """``sum_p v[p] a+_p,spin c_k``, as ``annihilate``, on the lists of ``other`` (default: ``neighbour`` with one
        particle of ``spin`` more)."""
        return self._ladder(v, c, spin, other, +1)[0]

    def _ladder_spectrum(self, step, v, spin, k, n_steps, state, reorthogonalize, beta_tol, other):
        with torch._C.DisableTorchFunctionSubclass():
            c, energy = self._reference(k, state)
            phi, other = self._ladder(v, c, spin, other, step)
            if phi.dim() != 2:
                raise ValueError("a spectrum takes ONE combination v (m,): a stack goes row by row")
            if other._dt == torch.complex128:
                phi = phi.to(other._dt)
            alpha, beta, norm2 = response.lanczos(other._sigma_rows, phi.reshape(1, other.dim), n_steps, reorthogonalize, beta_tol)
        return response.SpectralFunction(alpha, beta, norm2, energy)

    def removal_spectrum(self, v, spin="up", k=0, n_steps=64, state=None, reorthogonalize=False, beta_tol=0.0, other=None):
        """The ``response.SpectralFunction`` of removing a particle of ``spin`` in the orbital ``sum_p v[p] C[:, p]`` from
        solved state ``k`` (or from ``state=``, as in ``spectral_function``): ``n_steps`` of ``response.lanczos`` on the
        ``H`` of ``other`` (default: the neighbour) from ``phi = a(v) c``, not mean-subtracted.  Poles are
        ``E_j(N - 1) - E_k(N)``, the ionisation energies, weights ``|<j| a(v) |c>|^2``; ``phi = 0`` gives the empty
        spectrum."""
        return self._ladder_spectrum(-1, v, spin, k, n_steps, state, reorthogonalize, beta_tol, other)

    def addition_spectrum(self, v, spin="up", k=0, n_steps=64, state=None, reorthogonalize=False, beta_tol=0.0, other=None):
        """As ``removal_spectrum`` for ``phi = a+(v) c``: poles ``E_j(N + 1) - E_k(N)``, minus the electron affinities,
        weights ``|<j| a+(v) |c>|^2``."""
        return self._ladder_spectrum(+1, v, spin, k, n_steps, state, reorthogonalize, beta_tol, other)

    def green_function(self, omega, v, spin="up", eta=0.0, k=0, n_steps=64, **kw):
        """The retarded one-particle Green's function ``G_vv(omega)`` of solved state ``k``, the shape of ``omega``,
        complex: ``sum_j w+_j / (omega - p+_j + i eta) + sum_j w-_j / (omega + p-_j + i eta)`` over the poles and weights of
        ``addition_spectrum`` (+) and ``removal_spectrum`` (-); a sector that does not exist adds nothing (``kw``:
        ``reorthogonalize``, ``beta_tol``, ``state``)."""
        n = self.n_up if spin == "up" else self.n_down
        z = numpy.asarray(omega, dtype=numpy.float64)[..., None] + 1j * float(eta)
        value = numpy.zeros(z.shape[:-1], dtype=numpy.complex128)
        if n < self.m:
            S = self.addition_spectrum(v, spin, k, n_steps, **kw)
            value = value + numpy.sum(S.weights / (z - S.poles), axis=-1)
        if n > 0:
            S = self.removal_spectrum(v, spin, k, n_steps, **kw)
            value = value + numpy.sum(S.weights / (z + S.poles), axis=-1)
        with torch._C.DisableTorchFunctionSubclass():
            value = torch.as_tensor(numpy.asarray(value, dtype=numpy.complex128)).to(self._ta.device)
        return _deliver(value, self.system.np)

    def dyson_orbitals(self, other, k=0, spin="up"):
        """``(g, C @ g.T)`` between solved state ``k`` and every solved state of the neighbour ``other``:
        ``g[j, p] = <Psi_j(other)| a_p,spin |Psi_k>`` where ``other`` has one particle of ``spin`` less,
        ``<Psi_j(other)| a+_p,spin |Psi_k>`` where it has one more -- one ladder call with the m unit vectors and one
        product --, and the same amplitudes in the system's basis, one column per state of ``other``.  The pole strength of
        state j is ``sum_p |g[j, p]|^2``."""
        if not isinstance(other, StringCI):
            raise ValueError("other must be a StringCI of a neighbouring sector")
        if self._c is None:
            raise RuntimeError("call solve() first")
        if other._c is None:
            raise ValueError("other has no states yet: call other.solve() first")
        step = (other.n_up - self.n_up) if spin == "up" else (other.n_down - self.n_down)
        if step not in (1, -1):
            raise ValueError(f"other must hold one particle of spin {spin!r} more or less than this sector")
        with torch._C.DisableTorchFunctionSubclass():
            unit = torch.eye(self.m, dtype=torch.float64, device=self._c.device)
            X, _ = self._ladder(unit, self._c[k], spin, other, step)               # (m, na_t, nb_t)
            bra = other._c.reshape(other._c.shape[0], other.dim)
            dt = torch.complex128 if (bra.is_complex() or X.is_complex()) else torch.float64
            g = (bra.to(dt).conj() @ X.reshape(self.m, other.dim).to(dt).transpose(0, 1)).contiguous()
            orbitals = (self._C.to(dt) @ g.transpose(0, 1)).contiguous()
        return _deliver(g, self.system.np), _deliver(orbitals, self.system.np)

    def natural_orbitals(self, k=0):
        """``(n, C_nat)`` of solved state ``k``: the occupations ``n`` (descending eigenvalues of the Hermitian part of
        the spin-summed ``rho[q, p]``, between 0 and 2) and ``C_nat = C U`` with its eigenvectors as columns."""
        with torch._C.DisableTorchFunctionSubclass():
            rho = self._rho(k)
            n, U = torch.linalg.eigh(0.5 * (rho + _dagger(rho)))
            n, U = n.flip(0).contiguous(), U.flip(1)
            C_nat = (self._C @ U.to(self._dt)).contiguous()
        return _deliver(n, self.system.np), _deliver(C_nat, self.system.np)

    def to_determinants(self, c):
        """``(masks, v)``: the vector(s) ``c`` (na, nb) or (k, na, nb) in ``DeterminantCI``'s convention -- spin orbital
        ``2 p + sigma`` with alpha = 0, ``masks`` the ascending interleaved determinants (host int64 array), ``v`` (dim,)
        or (k, dim) on the device and in the dtype of ``c``, every entry multiplied by
        ``(-1)^(sum_{q in Ib} #{p in Ia : p > q})``.  Needs m <= 31."""
        masks, perm, phase = determinant_order(self._sa_host, self._sb_host)
        with torch._C.DisableTorchFunctionSubclass():
            c = _plain(c)
            flat = c.reshape(*c.shape[:-2], self.dim)
            ph = torch.from_numpy(phase).to(flat.device).to(flat.dtype)
            v = (flat * ph)[..., torch.from_numpy(perm).to(flat.device)].contiguous()
        return masks, v
