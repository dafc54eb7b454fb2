"""Coupled-cluster doubles: ``CCD`` for a ``GeneralOrbitalSystem`` with an anti-symmetrised ``u``, the particle-particle
ladder on the UNTRANSFORMED tensor through ``kernels.pair_contract_antisym``; ``RCCD`` (below) for a closed shell on a
``SpatialOrbitalSystem``, spin-summed, its ladder through ``kernels.pair_contract_exchange``.

The ``n = system.n`` lowest orbitals of ``C`` are occupied (i, j, k, l), the rest virtual (a, b, c, d).  Amplitudes
``t[a,b,i,j]`` are anti-symmetric in both pairs; with ``f`` the Fock matrix of the reference determinant in the orbitals

    R^{ab}_{ij} = u^{ab}_{ij} + P(ab) f^b_c t^{ac}_{ij} - P(ij) f^k_j t^{ab}_{ik}
                + 1/2 u^{ab}_{cd} t^{cd}_{ij} + 1/2 u^{kl}_{ij} t^{ab}_{kl} + P(ab) P(ij) u^{kb}_{cj} t^{ac}_{ik}
                + 1/4 u^{kl}_{cd} t^{cd}_{ij} t^{ab}_{kl} + P(ij) u^{kl}_{cd} t^{ac}_{ik} t^{bd}_{jl}
                - 1/2 P(ij) u^{kl}_{cd} t^{dc}_{ik} t^{ab}_{lj} - 1/2 P(ab) u^{kl}_{cd} t^{ac}_{lk} t^{db}_{ij}
    t <- t + R / D,   D = f_ii + f_jj - f_aa - f_bb,      E_corr = 1/4 sum u^{ij}_{ab} t^{ab}_{ij}

One iteration is ONE pass over the quarter of ``u`` that its symmetries do not repeat, plus O(o^3 v^3) of small products:

    tau[k = (i < j)] = C_v t[:, :, i, j] C_v^T                  (l x l each, anti-symmetric; K = o (o - 1) / 2 of them)
    S = pair_contract_antisym(u, tau)                           (the pass; u is never transformed)
    C_v^H S[k] C_v^*  =  u^{ab}_{cd} t^{cd}_{ij},       C_o^H S[k] C_o^*  =  u^{kl}_{cd} t^{cd}_{ij}   (the 1/4 term)

The blocks ``u^{ab}_{ij}``, ``u^{ij}_{ab}``, ``u^{kl}_{ij}`` and ``u^{kb}_{cj}`` are formed once, at construction
(``transform_two_body_blocks``, or slices of ``u`` when the system is in the orbital basis already); every other term is a
product on them and ``t``, in torch.

    ccd = CCD(system, C, epsilon)            # or CCD(system) after change_basis(C); or HartreeFock.ccd()
    e_corr = ccd.solve(tol=1e-8)             # ccd.t, ccd.residuals, ccd.converged, ccd.iterations

``RCCD.triples()`` adds the perturbative triples correction on the closed-shell amplitudes (``kernels.triples_energy``);
the spin-orbital ``CCD`` has none.  ``RCCSD`` (last) adds single excitations by T1-dressing the Hamiltonian that ``RCCD``
works on, and (T): the triples with their singles term (``kernels.triples_energy_singles``).
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
    return A.conj().transpose(0, 1)


def _sandwich(Ch, S):
    """``Ch S[k] Ch^T`` for every k: ``Ch`` (m, l), ``S`` (K, l, l) -> (K, m, m), two batched products."""
    X = kernels.matmul(Ch, S)                                          # (K, m, l): Ch S
    Y = kernels.matmul(Ch, X.transpose(1, 2).contiguous())             # (K, m, m): Ch (Ch S)^T = (Ch S Ch^T)^T
    return Y.transpose(1, 2)


class CCD:
    """Coupled-cluster doubles on the reference determinant of the ``system.n`` lowest orbitals.

    ``C`` (l, l; columns = orthonormal orbitals, ``C^H s C = 1``, canonical or not) with ``epsilon`` (the diagonal of
    the Fock matrix in them: the orbital energies ``HartreeFock.scf()`` returns) leaves the system in its basis; with
    ``C=None`` the system is taken to be in the orbital basis already.  ``ladder="antisym"`` sends the ladder through
    ``kernels.pair_contract_antisym`` (a quarter of ``u`` per pass), ``ladder="full"`` through ``kernels.pair_contract``
    (all of it): the same numbers by another kernel, kept for comparison."""

    def __init__(self, system, C=None, epsilon=None, ladder="antisym"):
        refuse_vectors_only(system, "CCD")
        if not isinstance(system, GeneralOrbitalSystem):
            raise TypeError("CCD needs a GeneralOrbitalSystem with an anti-symmetrised u: "
                            "pass spatial_system.construct_general_orbital_system(anti_symmetrize=True)")
        if not system._basis_set._anti_symmetrized_u:
            raise ValueError("CCD needs an anti-symmetrised u: build the GeneralOrbitalSystem with anti_symmetrize=True")
        if is_sharded(system.u):
            raise NotImplementedError("CCD does not take a sharded u: the pair contraction is not sharded -- "
                                      "pass a system whose u lives on one device")
        if ladder not in ("antisym", "full"):
            raise ValueError(f"ladder must be 'antisym' or 'full', got {ladder!r}")
        n, l = system.n, system.l
        if not 0 < n < l:
            raise ValueError(f"{n} occupied of {l} orbitals leave no occupied-virtual block")
        if (C is None) != (epsilon is None):
            raise ValueError("give both C and epsilon, or neither (system already in the orbital basis)")
        self.system, self.ladder = system, ladder
        self.n, self.l = n, l
        with torch._C.DisableTorchFunctionSubclass():
            u, h = _plain(system.u), _plain(system.h)
            self._u = u
            o, v = slice(0, n), slice(n, l)
            if C is None:
                self._dt = torch.complex128 if (u.is_complex() or h.is_complex()) else torch.float64
                self._Co = self._Cv = None
                f = _plain(system.construct_fock_matrix(system.h, system.u)).to(self._dt)
                self._vvoo = u[v, v, o, o].to(self._dt).contiguous()
                self._oovv = u[o, o, v, v].to(self._dt).contiguous()
                self._oooo = u[o, o, o, o].to(self._dt).contiguous()
                self._ovvo = u[o, v, v, o].to(self._dt).contiguous()
                eps = f.diagonal()
            else:
                C = _plain(C)
                if C.dim() != 2 or tuple(C.shape) != (l, l):
                    raise ValueError(f"C must be (l, l) with l = {l}, got {tuple(C.shape)}")
                self._dt = torch.complex128 if (C.is_complex() or u.is_complex() or h.is_complex()) else torch.float64
                C = C.to(self._dt)
                self._Co, self._Cv = C[:, o].contiguous(), C[:, v].contiguous()
                self._Coh, self._Cvh = _dagger(self._Co).contiguous(), _dagger(self._Cv).contiguous()
                cj, ck = system._mean_field_weights()
                rho = (self._Co @ self._Coh).contiguous()
                F = h.to(self._dt) + kernels.mean_field(u, rho, cj=cj, ck=ck).to(self._dt)
                f = _dagger(C) @ F @ C
                Co, Cv, Coh, Cvh = self._Co, self._Cv, self._Coh, self._Cvh

                def block(b0, b1, k0, k1):
                    return kernels.transform_two_body_blocks(u, b0, b1, k0, k1).to(self._dt)

                self._vvoo = block(Cvh, Cvh, Co, Co)
                self._oovv = block(Coh, Coh, Cv, Cv)
                self._oooo = block(Coh, Coh, Co, Co)
                self._ovvo = block(Coh, Cvh, Cv, Co)
                eps = _plain(epsilon)
                if eps.dim() != 1 or eps.shape[0] != l:
                    raise ValueError(f"epsilon must hold the {l} diagonal Fock elements, got {tuple(eps.shape)}")
            self._foo, self._fvv = f[o, o].contiguous(), f[v, v].contiguous()
            eps = (eps.real if eps.is_complex() else eps).to(torch.float64)
            eo, ev = eps[:n], eps[n:]
            self._D = ev.neg()[:, None, None, None] - ev[None, :, None, None] + eo[None, None, :, None] + eo[None, None, None, :]
            # the occupied pairs i < j: one amplitude matrix of the pass each
            self._pi, self._pj = torch.triu_indices(n, n, offset=1, device=u.device)
            self._t = self._vvoo / self._D
        self.t = _deliver(self._t, system.np)
        self.residuals, self.converged, self.iterations = [], False, 0

    # -- the pass over u: u^{ab}_{cd} t^{cd}_{ij} and u^{kl}_{cd} t^{cd}_{ij} from one contraction
    def _ladder(self, t):
        n, l, nv = self.n, self.l, self.l - self.n
        K = self._pi.numel()
        vvoo = torch.zeros((nv, nv, n, n), dtype=self._dt, device=t.device)
        oooo = torch.zeros((n, n, n, n), dtype=self._dt, device=t.device)
        if K == 0:                                    # one occupied orbital: t has no anti-symmetric pair
            return vvoo, oooo
        tk = t[:, :, self._pi, self._pj].permute(2, 0, 1).contiguous()              # (K, v, v)
        if self._Cv is None:
            tau = torch.zeros((K, l, l), dtype=self._dt, device=t.device)
            tau[:, n:, n:] = tk
        else:
            tau = _sandwich(self._Cv, tk).contiguous()
        u = self._u
        if self.ladder == "antisym":
            S = kernels.pair_contract_antisym(u, tau)
        else:
            S = kernels.pair_contract(u, tau)
        S = S.to(self._dt)
        if self._Cv is None:
            pp, hh = S[:, n:, n:], S[:, :n, :n]
        else:
            pp, hh = _sandwich(self._Cvh, S), _sandwich(self._Coh, S)
        pp, hh = pp.permute(1, 2, 0), hh.permute(1, 2, 0)
        vvoo[:, :, self._pi, self._pj] = pp
        vvoo[:, :, self._pj, self._pi] = -pp
        oooo[:, :, self._pi, self._pj] = hh
        oooo[:, :, self._pj, self._pi] = -hh
        return vvoo, oooo

    def residual(self, t=None):
        """``R^{ab}_{ij}`` of the amplitudes ``t`` (v, v, o, o), by default the current ones: a device tensor."""
        with torch._C.DisableTorchFunctionSubclass():
            t = self._t if t is None else _plain(t).to(self._dt)
            return self._residual(t)

    def _residual(self, t):
        ein = torch.einsum
        n, nv = self.n, self.l - self.n
        pp, W = self._ladder(t)                                          # u^{ab}_{cd} t^{cd}_{ij},  u^{kl}_{cd} t^{cd}_{ij}
        R = self._vvoo + 0.5 * pp
        X = ein("bc,acij->abij", self._fvv, t)
        R = R + X - X.transpose(0, 1)
        Y = ein("kj,abik->abij", self._foo, t)
        R = R - (Y - Y.transpose(2, 3))
        R = R + 0.5 * ein("klij,abkl->abij", self._oooo, t)
        Z = ein("kbcj,acik->abij", self._ovvo, t)
        R = R + Z - Z.transpose(0, 1) - Z.transpose(2, 3) + Z.transpose(0, 1).transpose(2, 3)
        R = R + 0.25 * ein("abkl,klij->abij", t, W)
        I = ein("klcd,acik->ladi", self._oovv, t)                        # u^{kl}_{cd} t^{ac}_{ik}
        Q = ein("ladi,bdjl->abij", I, t)
        R = R + Q - Q.transpose(2, 3)
        # the two one-index intermediates have a long sum and a small result: batched over the leading indices of the
        # sum and added up afterwards, so that the device is filled (one product of that shape is one workgroup's work)
        A = torch.bmm(self._oovv.permute(0, 2, 1, 3).reshape(n * nv, n, nv),
                      t.permute(3, 1, 0, 2).reshape(n * nv, nv, n)).sum(0)             # u^{kl}_{cd} t^{dc}_{ik} -> [l, i]
        B = ein("li,ablj->abij", A, t)
        R = R - 0.5 * (B - B.transpose(2, 3))
        A2 = torch.bmm(self._oovv.permute(0, 1, 3, 2).reshape(n * n, nv, nv),
                       t.permute(3, 2, 1, 0).reshape(n * n, nv, nv)).sum(0)            # u^{kl}_{cd} t^{ac}_{lk} -> [d, a]
        B2 = ein("da,dbij->abij", A2, t)
        R = R - 0.5 * (B2 - B2.transpose(0, 1))
        return R

    def energy(self, t=None):
        """``1/4 sum u^{ij}_{ab} t^{ab}_{ij}`` of the amplitudes (a float)."""
        with torch._C.DisableTorchFunctionSubclass():
            t = self._t if t is None else _plain(t).to(self._dt)
            e = 0.25 * (self._oovv * t.permute(2, 3, 0, 1)).sum()
            return float(e.real.item())

    def solve(self, tol=1e-8, max_iter=100, mixing=0.0):
        """Iterate ``t <- t + R / D`` (``mixing`` of the old amplitudes kept: ``t <- mixing t + (1 - mixing) (t + R / D)``)
        until the 2-norm of ``R`` is below ``tol``.  Starts from ``t = u^{ab}_{ij} / D``, so ``max_iter=0`` returns the
        MP2 energy.  A strongly correlated system (a shallow dot) may need ``mixing`` around 0.5 to converge.  Returns
        the correlation energy; keeps ``t``, ``residuals`` (the norm per iteration), ``converged`` and ``iterations``."""
        if not 0.0 <= mixing < 1.0:
            raise ValueError(f"mixing must lie in [0, 1), got {mixing}")
        with torch._C.DisableTorchFunctionSubclass():
            t = self._vvoo / self._D
            self.residuals, self.converged, self.iterations = [], False, 0
            for it in range(1, max_iter + 1):
                R = self._residual(t)
                norm = float(torch.linalg.vector_norm(R).item())
                self.residuals.append(norm)
                if norm < tol:
                    self.converged = True
                    break
                self.iterations = it
                t = t + (1.0 - mixing) * (R / self._D)
                # rounding leaves the anti-symmetric amplitudes, and the equations do not damp what it adds outside them
                t = 0.5 * (t - t.transpose(0, 1))
                t = 0.5 * (t - t.transpose(2, 3))
            self._t = t
            self.t = _deliver(t.contiguous(), self.system.np)
        return self.energy()


_EXCHANGE_ROUNDING = 1e-10


def _exchange_symmetric_to_rounding(u):
    """Is ``u[p,q,r,s] - u[q,p,s,r]`` at most ``_EXCHANGE_ROUNDING * max|u|`` everywhere?  What a four-index transform
    leaves of the symmetry where it did not take the mirrored route (``change_basis``): the fp64 rounding of sums of
    4 l terms, about 1e-13 at l = 256, times the growth under a non-unitary ``C`` -- far below any tolerance ``solve``
    is used with, and far above it a tensor simply does not have the symmetry.  Looked at only after the bit-for-bit
    check of ``kernels.two_body_exchange_symmetric`` has failed; one (l, l, l) slab at a time, no copy of ``u``."""
    worst = torch.zeros((), dtype=torch.float64, device=u.device)
    top = torch.zeros((), dtype=torch.float64, device=u.device)
    for p in range(u.shape[0]):
        worst = torch.maximum(worst, (u[p] - u[:, p].transpose(1, 2)).abs().max())
        top = torch.maximum(top, u[p].abs().max())
    return bool(worst <= _EXCHANGE_ROUNDING * top)


def _closed_shell_doubles(t, driver, W, fvv, foo, oovv, L, ovvo, ovov):
    """The closed-shell doubles residual (the formula of ``RCCD``) from ``driver = <ab|ij> + sum_cd <ab|cd> t^{cd}_{ij}``,
    ``W = <kl|ij> + sum_cd <kl|cd> t^{cd}_{ij}``, the Fock blocks and the small integral blocks.  Nothing in it uses
    hermiticity, so the blocks may be T1-dressed ones (``RCCSD``)."""
    ein = torch.einsum
    nv, n = t.shape[0], t.shape[2]
    R = driver + ein("klij,abkl->abij", W, t)
    # the two one-index intermediates have a long sum and a small result: batched over the leading indices of the
    # sum and added up afterwards, so that the device is filled (one product of that shape is one workgroup's work)
    Fvv = fvv - torch.bmm(t.permute(2, 3, 0, 1).reshape(n * n, nv, nv),
                          L.permute(0, 1, 3, 2).reshape(n * n, nv, nv)).sum(0)                 # L_klcd t^{bd}_{kl} -> [b, c]
    Foo = foo + torch.bmm(L.permute(1, 2, 0, 3).reshape(n * nv, n, nv),
                          t.permute(3, 0, 1, 2).reshape(n * nv, nv, n)).sum(0)                 # L_klcd t^{cd}_{jl} -> [k, j]
    Wd = ovvo - 0.5 * ein("klcd,dbjl->kbcj", oovv, t) + 0.5 * ein("klcd,dblj->kbcj", L, t)
    Wx = -ovov + 0.5 * ein("kldc,dbjl->kbjc", oovv, t)
    X = ein("bc,acij->abij", Fvv, t) - ein("kj,abik->abij", Foo, t)
    X = X + ein("acik,kbcj->abij", t - t.transpose(0, 1), Wd)
    X = X + ein("acik,kbcj->abij", t, Wd + Wx.transpose(2, 3))
    X = X + ein("ackj,kbic->abij", t, Wx)
    return R + X + X.transpose(0, 1).transpose(2, 3)


class RCCD:
    """Spin-adapted closed-shell coupled-cluster doubles on a ``SpatialOrbitalSystem``: the ``system.n`` lowest orbitals
    of ``C`` doubly occupied (i, j, k, l), the rest virtual (a, b, c, d), ``u`` as it is (``<pq|rs>``, not
    anti-symmetrised, never spin-doubled).  Amplitudes ``t[a,b,i,j] = t[b,a,j,i]``; with ``P X = X^{ab}_{ij} + X^{ba}_{ji}``

        L_klcd = 2<kl|cd> - <kl|dc>
        W_klij = <kl|ij> + sum_cd <kl|cd> t^{cd}_{ij}
        F_bc = f_bc - sum_kld L_klcd t^{bd}_{kl}                 F_kj = f_kj + sum_lcd L_klcd t^{cd}_{jl}
        Wd_kbcj =  <kb|cj> - 1/2 sum_ld <kl|cd> t^{db}_{jl} + 1/2 sum_ld L_klcd t^{db}_{lj}
        Wx_kbjc = -<kb|jc> + 1/2 sum_ld <kl|dc> t^{db}_{jl}
        R^{ab}_{ij} = <ab|ij> + sum_cd <ab|cd> t^{cd}_{ij} + sum_kl W_klij t^{ab}_{kl}
                    + P{ F_bc t^{ac}_{ij} - F_kj t^{ab}_{ik}
                         + sum_kc [(t^{ac}_{ik} - t^{ca}_{ik}) Wd_kbcj + t^{ac}_{ik} (Wd_kbcj + Wx_kbjc) + t^{ac}_{kj} Wx_kbic] }
        t <- t + R / D,   D = f_ii + f_jj - f_aa - f_bb,      E_corr = sum (2<ij|ab> - <ij|ba>) t^{ab}_{ij}

    One iteration is ONE pass over the half of ``u`` that its particle-exchange symmetry does not repeat:

        tau[k = (i <= j)] = C_v t[:, :, i, j] C_v^T                 (l x l each, generic; K = o (o + 1) / 2 of them)
        S = pair_contract_exchange(u, tau)                          (the pass; u is never transformed)
        C_v^H S[k] C_v^*  =  sum_cd <ab|cd> t^{cd}_{ij},     C_o^H S[k] C_o^*  =  sum_cd <kl|cd> t^{cd}_{ij}

    and the (j, i) results are their transposes.  The blocks vvoo, oovv, oooo, ovvo and ovov are formed once, at
    construction.  ``ladder="exchange"`` sends the ladder through ``kernels.pair_contract_exchange`` (half of ``u`` per
    pass), ``ladder="full"`` through ``kernels.pair_contract`` (all of it): the same numbers by another kernel.
    ``C``, ``epsilon``, ``solve``, ``residual``, ``energy``, ``t``, ``residuals``, ``converged`` and ``iterations`` are
    those of ``CCD``; ``max_iter=0`` gives the closed-shell MP2 energy.  ``u`` is checked for the symmetry once, at
    construction, for either ladder: bit for bit, and where that fails (a ``u`` that went through ``change_basis``) to
    rounding (``_exchange_symmetric_to_rounding``); anything else is refused.  ``triples()`` adds the perturbative
    triples correction on the amplitudes (canonical orbitals only)."""

    def __init__(self, system, C=None, epsilon=None, ladder="exchange"):
        refuse_vectors_only(system, type(self).__name__)
        if isinstance(system, GeneralOrbitalSystem):
            raise TypeError("RCCD needs a SpatialOrbitalSystem: for a GeneralOrbitalSystem call coupled_cluster.CCD")
        if not isinstance(system, SpatialOrbitalSystem):
            raise TypeError("RCCD needs a SpatialOrbitalSystem")
        if is_sharded(system.u):
            raise NotImplementedError("RCCD does not take a sharded u: the pair contraction is not sharded -- "
                                      "pass a system whose u lives on one device")
        if ladder not in ("exchange", "full"):
            raise ValueError(f"ladder must be 'exchange' or 'full', got {ladder!r}")
        n, l = system.n, system.l                     # a SpatialOrbitalSystem keeps the doubly occupied orbitals as its n
        if not 0 < n < l:
            raise ValueError(f"{n} doubly occupied of {l} orbitals leave no occupied-virtual block")
        if (C is None) != (epsilon is None):
            raise ValueError("give both C and epsilon, or neither (system already in the orbital basis)")
        self.system, self.ladder = system, ladder
        self.n, self.l = n, l
        with torch._C.DisableTorchFunctionSubclass():
            u, h = _plain(system.u), _plain(system.h)
            if not kernels.two_body_exchange_symmetric(u) and not _exchange_symmetric_to_rounding(u):
                raise ValueError("RCCD needs a u with particle-exchange symmetry, u[p,q,r,s] = u[q,p,s,r]: "
                                 "both ladders and the equations rest on it")
            self._u, self._h = u, h
            o, v = slice(0, n), slice(n, l)
            if C is None:
                self._dt = torch.complex128 if (u.is_complex() or h.is_complex()) else torch.float64
                self._Co = self._Cv = None
                f = _plain(system.construct_fock_matrix(system.h, system.u)).to(self._dt)
                self._vvoo = u[v, v, o, o].to(self._dt).contiguous()
                self._oovv = u[o, o, v, v].to(self._dt).contiguous()
                self._oooo = u[o, o, o, o].to(self._dt).contiguous()
                self._ovvo = u[o, v, v, o].to(self._dt).contiguous()
                self._ovov = u[o, v, o, v].to(self._dt).contiguous()
                eps = f.diagonal()
            else:
                C = _plain(C)
                if C.dim() != 2 or tuple(C.shape) != (l, l):
                    raise ValueError(f"C must be (l, l) with l = {l}, got {tuple(C.shape)}")
                self._dt = torch.complex128 if (C.is_complex() or u.is_complex() or h.is_complex()) else torch.float64
                C = C.to(self._dt)
                self._Co, self._Cv = C[:, o].contiguous(), C[:, v].contiguous()
                self._Coh, self._Cvh = _dagger(self._Co).contiguous(), _dagger(self._Cv).contiguous()
                cj, ck = system._mean_field_weights()
                rho = (2.0 * (self._Co @ self._Coh)).contiguous()                  # the spin-summed density
                F = h.to(self._dt) + kernels.mean_field(u, rho, cj=cj, ck=ck).to(self._dt)
                f = _dagger(C) @ F @ C
                Co, Cv, Coh, Cvh = self._Co, self._Cv, self._Coh, self._Cvh

                def block(b0, b1, k0, k1):
                    return kernels.transform_two_body_blocks(u, b0, b1, k0, k1).to(self._dt)

                self._vvoo = block(Cvh, Cvh, Co, Co)
                self._oovv = block(Coh, Coh, Cv, Cv)
                self._oooo = block(Coh, Coh, Co, Co)
                self._ovvo = block(Coh, Cvh, Cv, Co)
                self._ovov = block(Coh, Cvh, Co, Cv)
                eps = _plain(epsilon)
                if eps.dim() != 1 or eps.shape[0] != l:
                    raise ValueError(f"epsilon must hold the {l} diagonal Fock elements, got {tuple(eps.shape)}")
            self._foo, self._fvv = f[o, o].contiguous(), f[v, v].contiguous()
            self._fov, self._fvo = f[o, v].contiguous(), f[v, o].contiguous()       # (triples: are the orbitals canonical?)
            self._L = 2.0 * self._oovv - self._oovv.transpose(2, 3)
            eps = (eps.real if eps.is_complex() else eps).to(torch.float64)
            self._eps = eps
            eo, ev = eps[:n], eps[n:]
            self._D = ev.neg()[:, None, None, None] - ev[None, :, None, None] + eo[None, None, :, None] + eo[None, None, None, :]
            # the occupied pairs i <= j: one amplitude matrix of the pass each
            self._pi, self._pj = torch.triu_indices(n, n, device=u.device)
            self._t = self._vvoo / self._D
        self.t = _deliver(self._t, system.np)
        self.residuals, self.converged, self.iterations = [], False, 0
        self._triples_blocks, self.triples_passes = None, []

    # -- the pass over u: sum_cd <ab|cd> t^{cd}_{ij} and sum_cd <kl|cd> t^{cd}_{ij} from one contraction
    def _ladder(self, t):
        n, l, nv = self.n, self.l, self.l - self.n
        K = self._pi.numel()
        tk = t[:, :, self._pi, self._pj].permute(2, 0, 1).contiguous()              # (K, v, v)
        if self._Cv is None:
            tau = torch.zeros((K, l, l), dtype=self._dt, device=t.device)
            tau[:, n:, n:] = tk
        else:
            tau = _sandwich(self._Cv, tk).contiguous()
        u = self._u
        if self.ladder == "exchange":
            S = kernels.pair_contract_exchange(u, tau)
        else:
            S = kernels.pair_contract(u, tau)
        S = S.to(self._dt)
        if self._Cv is None:
            pp, hh = S[:, n:, n:], S[:, :n, :n]
        else:
            pp, hh = _sandwich(self._Cvh, S), _sandwich(self._Coh, S)
        vvoo = torch.empty((nv, nv, n, n), dtype=self._dt, device=t.device)
        oooo = torch.empty((n, n, n, n), dtype=self._dt, device=t.device)
        # the (j, i) results are the transposes: sum_cd <ab|cd> t^{cd}_{ji} = sum_cd <ba|dc> t^{dc}_{ij}
        vvoo[:, :, self._pj, self._pi] = pp.permute(2, 1, 0)
        vvoo[:, :, self._pi, self._pj] = pp.permute(1, 2, 0)
        oooo[:, :, self._pj, self._pi] = hh.permute(2, 1, 0)
        oooo[:, :, self._pi, self._pj] = hh.permute(1, 2, 0)
        return vvoo, oooo

    def residual(self, t=None):
        """``R^{ab}_{ij}`` of the amplitudes ``t`` (v, v, o, o) with ``t[a,b,i,j] = t[b,a,j,i]``, by default the
        current ones: a device tensor."""
        with torch._C.DisableTorchFunctionSubclass():
            t = self._t if t is None else _plain(t).to(self._dt)
            return self._residual(t)

    def _residual(self, t):
        pp, hh = self._ladder(t)                                         # sum_cd <ab|cd> t^{cd}_{ij},  sum_cd <kl|cd> t^{cd}_{ij}
        return _closed_shell_doubles(t, self._vvoo + pp, self._oooo + hh, self._fvv, self._foo, self._oovv, self._L,
                                     self._ovvo, self._ovov)

    def energy(self, t=None):
        """``sum (2<ij|ab> - <ij|ba>) t^{ab}_{ij}`` of the amplitudes (a float)."""
        with torch._C.DisableTorchFunctionSubclass():
            t = self._t if t is None else _plain(t).to(self._dt)
            e = (self._L * t.permute(2, 3, 0, 1)).sum()
            return float(e.real.item())

    def solve(self, tol=1e-8, max_iter=100, mixing=0.0):
        """Iterate ``t <- t + R / D`` (``mixing`` of the old amplitudes kept) until the 2-norm of ``R`` is below ``tol``,
        as ``CCD.solve``.  Starts from ``t = <ab|ij> / D``, so ``max_iter=0`` returns the closed-shell MP2 energy.
        Returns the correlation energy; keeps ``t``, ``residuals``, ``converged`` and ``iterations``."""
        if not 0.0 <= mixing < 1.0:
            raise ValueError(f"mixing must lie in [0, 1), got {mixing}")
        with torch._C.DisableTorchFunctionSubclass():
            t = self._vvoo / self._D
            self.residuals, self.converged, self.iterations = [], False, 0
            for it in range(1, max_iter + 1):
                R = self._residual(t)
                norm = float(torch.linalg.vector_norm(R).item())
                self.residuals.append(norm)
                if norm < tol:
                    self.converged = True
                    break
                self.iterations = it
                t = t + (1.0 - mixing) * (R / self._D)
                # back onto t^{ab}_{ij} = t^{ba}_{ji}: the (j, i) halves of the ladder are taken from it
                t = 0.5 * (t + t.transpose(0, 1).transpose(2, 3))
            self._t = t
            self.t = _deliver(t.contiguous(), self.system.np)
        return self.energy()

    # -- the perturbative triples on the doubles
    def _require_canonical(self, canonical_tol):
        foo, fvv = self._foo, self._fvv
        worst = max(float((foo - torch.diag(foo.diagonal())).abs().max().item()),
                    float((fvv - torch.diag(fvv.diagonal())).abs().max().item()),
                    float(self._fov.abs().max().item()), float(self._fvo.abs().max().item()))
        top = float(self._eps.abs().max().item())
        if worst > canonical_tol * top:
            raise ValueError(f"{type(self).__name__}.triples needs canonical orbitals (a diagonal Fock matrix): the largest "
                             f"off-diagonal element is {worst:.3e}, above canonical_tol * max|epsilon| = {canonical_tol * top:.3e} -- "
                             "pass the C and epsilon of HartreeFock.scf()")

    def _triples_integrals(self):
        """``Vp[k,d,b,c] = <bc|dk>`` (o, v, v, v) and ``Hh[j,k,l,c] = -<lc|jk>`` (o, o, o, v), formed once."""
        if self._triples_blocks is None:
            n, l = self.n, self.l
            o, v = slice(0, n), slice(n, l)
            u = self._u
            if self._Cv is None:
                vvvo, ovoo = u[v, v, v, o], u[o, v, o, o]
            else:
                Co, Cv, Coh, Cvh = self._Co, self._Cv, self._Coh, self._Cvh
                vvvo = kernels.transform_two_body_blocks(u, Cvh, Cvh, Cv, Co)
                ovoo = kernels.transform_two_body_blocks(u, Coh, Cvh, Co, Co)
            self._triples_blocks = (vvvo.to(self._dt).permute(3, 2, 0, 1).contiguous(),
                                    ovoo.to(self._dt).permute(2, 3, 0, 1).neg().contiguous())
        return self._triples_blocks

    def triples(self, t=None, canonical_tol=1e-8):
        """The perturbative triples correction ``E_T`` (a float) on the doubles amplitudes ``t`` (v, v, o, o), by default
        the current ones: "+T(CCD)" on converged amplitudes, the fourth-order triples energy on first-order ones
        (``solve(max_iter=0)``).  With ``T2`` the doubles operator of ``t``,

            E_T = sum_mu |<mu| H T2 |0>|^2 / D_mu,      D_mu = sum eps(holes of mu) - sum eps(particles of mu)

        over the triply excited determinants; in the closed-shell working form

            X_ijk[a,b,c] = sum_d t[a,d,i,j] <bc|dk>  -  sum_l t[a,b,i,l] <lc|jk>
            W_ijk[a,b,c] = X_ijk[a,b,c] + X_ikj[a,c,b] + X_jik[b,a,c] + X_jki[b,c,a] + X_kij[c,a,b] + X_kji[c,b,a]
            Z[a,b,c]     = (4 W_abc + W_bca + W_cab - 2 W_acb - 2 W_cba - 2 W_bac) / 3
            e_ijk        = sum_abc Re(conj(W_abc) Z_abc) / (eps_i + eps_j + eps_k - eps_a - eps_b - eps_c)
            E_T          = sum_{i<=j<=k} m_ijk e_ijk,     m = 6 (all different), 3 (two equal), 0 (i = j = k)

        The blocks ``X`` are products on the GEMM dispatcher (with the blocks laid out (k, j, i), the particle term of every
        (i, j) at a fixed k is ONE product and the hole term of every i at a fixed (j, k) one accumulating product);
        ``kernels.triples_energy`` turns them into ``e_ijk`` in one read.  Where all o^3 blocks fit
        ``kernels.TRIPLES_BYTES`` (tuning key ``triples_bytes``) there is one launch of it over all triples; otherwise
        passes over as many triples as their own blocks (six, or three where two indices are equal) fit, at least one,
        each block one particle and one hole product.  ``triples_passes`` keeps (triples, blocks, kernels) of every pass.

        The formula holds in canonical orbitals only: ``ValueError`` where an off-diagonal element of the Fock matrix
        exceeds ``canonical_tol * max|epsilon|`` (the orbitals of ``HartreeFock.scf`` at its default tolerance pass)."""
        if is_sharded(self.system.u):
            raise NotImplementedError("RCCD.triples does not take a sharded u: pass a system whose u lives on one device")
        with torch._C.DisableTorchFunctionSubclass():
            n, nv = self.n, self.l - self.n
            if t is None:
                t = self._t
            else:
                t = _plain(t)
                if tuple(t.shape) != (nv, nv, n, n):
                    raise ValueError(f"t must be (v, v, o, o) = {(nv, nv, n, n)}, got {tuple(t.shape)}")
                t = t.to(self._dt)
            self._require_canonical(canonical_tol)
            todo, e, _ = self._triples_energies(t)
            if not todo:                    # one occupied orbital: three like spins cannot share it
                return 0.0
            return float((self._triples_weights(todo, t.device) * e).sum().item())

    @staticmethod
    def _triples_weights(todo, dev):
        return torch.tensor([3.0 if (i == j or j == k) else 6.0 for i, j, k in todo], dtype=torch.float64, device=dev)

    def _triples_energies(self, t, t1=None):
        """The blocks and the pass loop of ``triples``: ``(todo, e, es)`` with ``todo`` the triples i <= j <= k (without
        i = j = k) and ``e`` their energies.  With ``t1`` (v, o) the passes go through ``kernels.triples_energy_singles``
        on ``A = 1/2 t1^T`` (o, v) and ``G[q o + r] = <bc|qr>`` (o^2, v, v), block ``X_pqr`` with the slot ``(p, q o + r)``,
        and ``es`` is the singles part of every triple; without it ``es`` is None."""
        n, nv = self.n, self.l - self.n
        self.triples_passes = []
        todo = [(i, j, k) for i in range(n) for j in range(i, n) for k in range(j, n) if not i == j == k]
        if not todo:
            return todo, None, None
        Vp, Hh = self._triples_integrals()
        dt, dev = self._dt, t.device
        tp = t.permute(3, 2, 0, 1).contiguous()                  # tp[j,i,a,d] = t[a,d,i,j]
        th = t.permute(2, 0, 1, 3).contiguous()                  # th[i,a,b,l] = t[a,b,i,l]
        eo, ev = self._eps[:n].tolist(), self._eps[n:].contiguous()
        v2, v3 = nv * nv, nv * nv * nv
        if t1 is not None:
            A = (0.5 * t1.transpose(0, 1)).contiguous()
            G = self._vvoo.permute(2, 3, 0, 1).contiguous().reshape(n * n, nv, nv)

        def orders(i, j, k):
            return ((i, j, k), (i, k, j), (j, i, k), (j, k, i), (k, i, j), (k, j, i))

        def energies(X, group, where):
            slots = torch.tensor([[where[pqr] for pqr in orders(*ijk)] for ijk in group], dtype=torch.int32, device=dev)
            eo3 = torch.tensor([eo[i] + eo[j] + eo[k] for i, j, k in group], dtype=torch.float64, device=dev)
            if t1 is None:
                e = kernels.triples_energy(X, slots, eo3, ev), None
            else:
                sslots = torch.tensor([[(p, q * n + r) for p, q, r in orders(*ijk)] for ijk in group], dtype=torch.int32,
                                      device=dev)
                e = kernels.triples_energy_singles(X, slots, eo3, ev, A, G, sslots)
            self.triples_passes.append((len(group), X.shape[0], kernels.last_dispatch()))
            return e

        fit = kernels.triples_budget() // (v3 * t.element_size())
        if fit >= n ** 3:
            # every block, X_pqr at (r, q, p): o particle products and o^2 hole products
            X = torch.empty((n ** 3, nv, nv, nv), dtype=dt, device=dev)
            for k in range(n):
                kernels.gemm_raw(dt, tp, Vp, X, n * n * nv, v2, nv, nv, v2, v2, b_off=k * v3, c_off=k * n * n * v3)
                for j in range(n):
                    kernels.gemm_raw(dt, th, Hh, X, n * v2, nv, n, n, nv, nv, accumulate=True,
                                     b_off=(j * n + k) * n * nv, c_off=(k * n + j) * n * v3)
            e, es = energies(X, todo, {(p, q, r): (r * n + q) * n + p for p in range(n) for q in range(n) for r in range(n)})
        else:
            # passes: triples share no block, so a group's blocks are the sum of its triples' own
            groups, count = [[]], 0
            for ijk in todo:
                own = len(set(orders(*ijk)))
                if groups[-1] and count + own > fit:
                    groups.append([])
                    count = 0
                groups[-1].append(ijk)
                count += own
            parts = []
            for group in groups:
                where = {}
                for ijk in group:
                    for pqr in orders(*ijk):
                        where.setdefault(pqr, len(where))
                X = torch.empty((len(where), nv, nv, nv), dtype=dt, device=dev)
                for (p, q, r), x in where.items():
                    kernels.gemm_raw(dt, tp, Vp, X, nv, v2, nv, nv, v2, v2, a_off=(q * n + p) * v2, b_off=r * v3, c_off=x * v3)
                    kernels.gemm_raw(dt, th, Hh, X, v2, nv, n, n, nv, nv, accumulate=True,
                                     a_off=p * v2 * n, b_off=(q * n + r) * n * nv, c_off=x * v3)
                parts.append(energies(X, group, where))
                del X
            e = torch.cat([part[0] for part in parts])
            es = None if t1 is None else torch.cat([part[1] for part in parts])
        return todo, e, es


class RCCSD(RCCD):
    """Closed-shell coupled-cluster singles and doubles on a ``SpatialOrbitalSystem``, with the perturbative triples
    (T): ``RCCD`` on the T1-dressed Hamiltonian.  Constructor, checks and conventions are those of
    ``RCCD``; amplitudes ``t1`` (v, o) and ``t`` (v, v, o, o).  With ``tau`` (l, l) zero except ``tau[virt, occ] = t1``,

        h~ = (1 - tau) h (1 + tau),      <pq|rs>~ = (1 - tau) (1 - tau) <..|..> (1 + tau) (1 + tau)

    (bras ``1 - tau``, kets ``1 + tau``; ``t1`` is never conjugated), ``f~ = h~ + 2 J~ - K~`` of the occupied orbitals and
    ``tt = 2 t - t.transpose(0, 1)``:

        R2       = the residual of RCCD on f~ and <..|..>~
        R1[a,i]  = f~[a,i] + sum_kc f~[k,c] tt[a,c,i,k] + sum_kcd <ak|cd>~ tt[c,d,i,k] - sum_klc <kl|ic>~ tt[a,c,k,l]
        E_corr   = 2 sum f[i,a] t1[a,i] + sum (2<ij|ab> - <ij|ba>) (t[a,b,i,j] + t1[a,i] t1[b,j])

    The dressing keeps the particle-exchange symmetry of ``u`` and gives up hermiticity, which the equations of RCCD
    never use.  Only two coefficient blocks change: the bra-virtual rows ``Xvh = Cv^H - t1 Co^H`` and the ket-occupied
    columns ``Yo = Co + Cv t1``.  One iteration is still ONE pass over half of ``u``:

        tau[k = (i <= j)] = Cv t[:, :, i, j] Cv^T + Yo[:, i] Yo[:, j]^T       (the driver <ab|ij>~ rides in the ladder)
        S = pair_contract_exchange(u, tau)
        B S[k] B^T,  B = [Co^H; Xvh]:   vv = <ab|ij>~ + sum_cd <ab|cd>~ t,   oo = <kl|ij>~ + sum_cd <kl|cd> t,
                                        vo and ov = <ak|ij>~ + sum_cd <ak|cd>~ t  at (i, j) and (j, i)

    and ``sum_k (2 vo_ik - vo_ki)[a,k]`` is the ``<ak|cd>~ tt`` term of ``R1`` TOGETHER WITH the mean-field part of
    ``f~[a,i]``, so ``R1`` starts from ``h~[a,i]``.  The small dressed blocks ovvo~, ovov~ and ooov~ come every iteration
    from ``transform_two_body_blocks`` with the dressed matrices (three more block passes over ``u`` per iteration);
    oovv is undressed and static; ``f~`` is ``kernels.mean_field(u, 2 Yo Co^H)`` between ``B`` and ``[Yo, Cv]``.  With
    ``C=None`` the same code runs on the unit matrix.

    ``solve`` iterates ``t1 += R1 / (e_i - e_a)``, ``t += R2 / D`` from ``f_ai / (e_i - e_a)`` and the first-order
    doubles until the norm of ``(R1, R2)`` together is below ``tol``.  ``triples()`` is E_(T): the connected part
    ``E_[T]`` of ``RCCD.triples`` and the singles part ``E_ST`` from one launch of ``kernels.triples_energy_singles``
    (``triples_parts``); canonical orbitals only."""

    def __init__(self, system, C=None, epsilon=None, ladder="exchange"):
        # RCCD's checks, Fock blocks, denominators and static blocks: vvoo (the start, and G of the triples), oovv and L are
        # used as they are; oooo, ovvo and ovov are dressed anew in every iteration and RCCD's copies stay unused
        super().__init__(system, C, epsilon, ladder)
        with torch._C.DisableTorchFunctionSubclass():
            n, l = self.n, self.l
            if self._Co is None:                       # the system is in the orbital basis: the unit matrix
                one = torch.eye(l, dtype=self._dt, device=self._u.device)
                self._Co, self._Cv = one[:, :n].contiguous(), one[:, n:].contiguous()
                self._Coh, self._Cvh = _dagger(self._Co).contiguous(), _dagger(self._Cv).contiguous()
            self._cj, self._ck = system._mean_field_weights()
            eo, ev = self._eps[:n], self._eps[n:]
            self._D1 = eo[None, :] - ev[:, None]
            self._t1 = self._fvo / self._D1
        self.t1 = _deliver(self._t1, system.np)
        self.triples_parts = None

    def _residuals(self, t1, t):
        ein = torch.einsum
        n, l = self.n, self.l
        u, dt = self._u, self._dt
        Co, Cv, Coh = self._Co, self._Cv, self._Coh
        Xvh = self._Cvh - t1 @ Coh                                        # bra-virtual rows
        Yo = Co + Cv @ t1                                                 # ket-occupied columns
        B = torch.cat([Coh, Xvh]).contiguous()                            # the bras (l, l): occupied undressed
        Kt = torch.cat([Yo, Cv], dim=1).contiguous()                      # the kets (l, l): virtual undressed
        # -- the pass over half of u
        tk = t[:, :, self._pi, self._pj].permute(2, 0, 1).contiguous()                # (K, v, v)
        tau = _sandwich(Cv, tk) + ein("pk,qk->kpq", Yo[:, self._pi], Yo[:, self._pj])
        tau = tau.contiguous()
        S = (kernels.pair_contract_exchange(u, tau) if self.ladder == "exchange" else kernels.pair_contract(u, tau)).to(dt)
        Q = _sandwich(B, S)                                               # (K, l, l): B S B^T
        nv = l - n
        driver = torch.empty((nv, nv, n, n), dtype=dt, device=t.device)
        W = torch.empty((n, n, n, n), dtype=dt, device=t.device)
        M = torch.empty((n, n, nv, n), dtype=dt, device=t.device)        # M[i,j,a,k] = <ak|ij>~ + sum_cd <ak|cd>~ t^{cd}_{ij}
        # the (j, i) results are the transposes
        driver[:, :, self._pj, self._pi] = Q[:, n:, n:].permute(2, 1, 0)
        driver[:, :, self._pi, self._pj] = Q[:, n:, n:].permute(1, 2, 0)
        W[:, :, self._pj, self._pi] = Q[:, :n, :n].permute(2, 1, 0)
        W[:, :, self._pi, self._pj] = Q[:, :n, :n].permute(1, 2, 0)
        M[self._pj, self._pi] = Q[:, :n, n:].transpose(1, 2)
        M[self._pi, self._pj] = Q[:, n:, :n]
        # -- the dressed one-body matrices and small blocks
        rho = (2.0 * (Yo @ Coh)).contiguous()
        hd = B @ self._h.to(dt) @ Kt
        fd = hd + B @ kernels.mean_field(u, rho, cj=self._cj, ck=self._ck).to(dt) @ Kt
        o, v = slice(0, n), slice(n, l)

        def block(b0, b1, k0, k1):
            return kernels.transform_two_body_blocks(u, b0.contiguous(), b1.contiguous(), k0.contiguous(), k1.contiguous()).to(dt)

        ovvo, ovov, ooov = block(Coh, Xvh, Cv, Yo), block(Coh, Xvh, Yo, Cv), block(Coh, Coh, Yo, Cv)
        R2 = _closed_shell_doubles(t, driver, W, fd[v, v], fd[o, o], self._oovv, self._L, ovvo, ovov)
        tt = 2.0 * t - t.transpose(0, 1)
        R1 = hd[v, o] + 2.0 * ein("ikak->ai", M) - ein("kiak->ai", M)    # f~[a,i] and the <ak|cd>~ tt term
        R1 = R1 + ein("kc,acik->ai", fd[o, v], tt) - ein("klic,ackl->ai", ooov, tt)
        return R1, R2

    def _amplitudes(self, t1, t):
        n, nv = self.n, self.l - self.n
        t1 = self._t1 if t1 is None else _plain(t1)
        t = self._t if t is None else _plain(t)
        if tuple(t1.shape) != (nv, n) or tuple(t.shape) != (nv, nv, n, n):
            raise ValueError(f"t1 must be (v, o) = {(nv, n)} and t (v, v, o, o) = {(nv, nv, n, n)}, "
                             f"got {tuple(t1.shape)} and {tuple(t.shape)}")
        return t1.to(self._dt), t.to(self._dt)

    def residual(self, t1=None, t=None):
        """``(R1, R2)`` of the amplitudes ``t1`` (v, o) and ``t`` (v, v, o, o) with ``t[a,b,i,j] = t[b,a,j,i]``, by
        default the current ones: device tensors."""
        with torch._C.DisableTorchFunctionSubclass():
            return self._residuals(*self._amplitudes(t1, t))

    def energy(self, t1=None, t=None):
        """``2 sum f_ia t1 + sum (2<ij|ab> - <ij|ba>) (t + t1 t1)`` of the amplitudes (a float)."""
        with torch._C.DisableTorchFunctionSubclass():
            t1, t = self._amplitudes(t1, t)
            pairs = t.permute(2, 3, 0, 1) + torch.einsum("ai,bj->ijab", t1, t1)
            e = 2.0 * (self._fov * t1.transpose(0, 1)).sum() + (self._L * pairs).sum()
            return float(e.real.item())

    def solve(self, tol=1e-8, max_iter=100, mixing=0.0):
        """Iterate ``t1 <- t1 + R1 / (e_i - e_a)``, ``t <- t + R2 / D`` (``mixing`` of the old amplitudes kept) until the
        2-norm of ``(R1, R2)`` together is below ``tol``.  Starts from ``f_ai / (e_i - e_a)`` and ``<ab|ij> / D``.
        Returns the correlation energy; keeps ``t1``, ``t``, ``residuals``, ``converged`` and ``iterations``."""
        if not 0.0 <= mixing < 1.0:
            raise ValueError(f"mixing must lie in [0, 1), got {mixing}")
        with torch._C.DisableTorchFunctionSubclass():
            t1, t = self._fvo / self._D1, self._vvoo / self._D
            self.residuals, self.converged, self.iterations = [], False, 0
            for it in range(1, max_iter + 1):
                R1, R2 = self._residuals(t1, t)
                norm = float(torch.hypot(torch.linalg.vector_norm(R1), torch.linalg.vector_norm(R2)).item())
                self.residuals.append(norm)
                if norm < tol:
                    self.converged = True
                    break
                self.iterations = it
                t1 = t1 + (1.0 - mixing) * (R1 / self._D1)
                t = t + (1.0 - mixing) * (R2 / self._D)
                t = 0.5 * (t + t.transpose(0, 1).transpose(2, 3))
            self._t1, self._t = t1, t
            self.t1 = _deliver(t1.contiguous(), self.system.np)
            self.t = _deliver(t.contiguous(), self.system.np)
        return self.energy()

    def triples(self, canonical_tol=1e-8):
        """E_(T) (a float) on the current amplitudes: ``E_[T] + E_ST``, kept as ``triples_parts``.  ``E_[T]`` is the
        correction of ``RCCD.triples`` on ``t``; with ``Y_ijk[a,b,c] = 1/2 t1[a,i] <bc|jk>`` and ``V'`` the six-fold
        permuted sum of ``Y`` that makes ``W`` from ``X``,

            E_ST = sum_{i<=j<=k} m_ijk sum_abc Re(conj(V'_abc) Z_abc) / D

        The blocks ``X`` come from ``t`` and the undressed integrals exactly as in ``RCCD.triples`` (the same budget and
        passes, ``triples_passes``); ``Y`` is never formed: ``kernels.triples_energy_singles`` reads ``A = 1/2 t1^T`` and
        ``G[q o + r] = <bc|qr>``.  Canonical orbitals only (``ValueError`` otherwise)."""
        if is_sharded(self.system.u):
            raise NotImplementedError("RCCSD.triples does not take a sharded u: pass a system whose u lives on one device")
        with torch._C.DisableTorchFunctionSubclass():
            self._require_canonical(canonical_tol)
            todo, e, es = self._triples_energies(self._t, self._t1)
            if not todo:
                self.triples_parts = (0.0, 0.0)
                return 0.0
            m = self._triples_weights(todo, self._t.device)
            self.triples_parts = (float((m * e).sum().item()), float((m * es).sum().item()))
            return self.triples_parts[0] + self.triples_parts[1]
