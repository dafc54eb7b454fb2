"""``QuantumSystem``: a ``BasisSet`` plus a particle number.

Thin forwarding layer with the interface of the reference's abstract base
(quantum_systems/system.py): it owns the basis set, tracks ``n``, ``l``,
``m = l - n`` and the occupied / virtual slices ``o`` / ``v``, and forwards the
basis-change and module-change calls.  The heavy work happens in
``BasisSet`` (HIP kernels)."""

import abc
import copy
from collections.abc import Iterable

from .basis_set import refuse_vectors_only, vectors_only


class QuantumSystem(metaclass=abc.ABCMeta):
    """``n`` occupied basis functions on top of ``basis_set`` (system.py:20-30)."""

    def __init__(self, n, basis_set):
        self._basis_set = basis_set
        assert n <= self._basis_set.l
        self.np = self._basis_set.np
        self.set_system_size(n, self._basis_set.l)
        self._time_evolution_operator = []
        self._add_h_0 = True
        self._add_u_0 = True

    def set_system_size(self, n, l):
        """Record sizes and the index ranges they imply (system.py:32-51)."""
        assert n <= l
        self.n, self.l = n, l
        self.m = l - n
        self.o = slice(0, n)
        self.v = slice(n, l)

    # -- to be provided by the concrete system kinds
    @abc.abstractmethod
    def construct_fock_matrix(self, h, u, f=None):
        pass

    @abc.abstractmethod
    def change_to_hf_basis(self, *args, **kwargs):
        pass

    @abc.abstractmethod
    def compute_reference_energy(self, h=None, u=None):
        pass

    # -- mean field of a general one-body density: ONE pass over u on the GPU (kernels.mean_field)
    def _mean_field_weights(self):
        """``(cj, ck)`` of  W[p,q] = cj u[p,r,q,s] rho[s,r] + ck u[p,r,s,q] rho[s,r]  for this kind of system."""
        raise NotImplementedError

    def construct_mean_field_from_density(self, rho_qp, u=None):
        """The two-body part ``W`` of the Fock matrix for the one-body density ``rho_qp`` (the convention of
        ``compute_particle_density``: the full, spin-summed density, trace(rho s) = n)."""
        from . import kernels, sharded_basis
        from .basis_set import _deliver, _stage
        from .sharded_module import is_sharded

        cj, ck = self._mean_field_weights()
        if u is None and vectors_only(self):
            return _deliver(self._basis_set.two_body.mean_field(_stage(rho_qp), cj=cj, ck=ck), self.np)
        u = self.u if u is None else u
        if is_sharded(u):
            return sharded_basis.mean_field(u, rho_qp, cj, ck, self.np)
        return _deliver(kernels.mean_field(_stage(u), _stage(rho_qp), cj=cj, ck=ck), self.np)

    def construct_mean_fields_from_densities(self, rhos, u=None):
        """``construct_mean_field_from_density`` for a stack of densities ``rhos`` (ND, l, l) from ONE read of ``u`` per
        group of them (``kernels.mean_field_batch``).  Returns (ND, l, l); every ``W[k]`` has the same bits whatever
        else is in the stack."""
        from . import kernels
        from .basis_set import _deliver, _stage
        from .sharded_module import is_sharded

        if u is None:
            refuse_vectors_only(self, "construct_mean_fields_from_densities")
        u = self.u if u is None else u
        if is_sharded(u):
            raise NotImplementedError("construct_mean_fields_from_densities does not take a sharded u: "
                                      "the batched mean-field contraction is not sharded")
        cj, ck = self._mean_field_weights()
        return _deliver(kernels.mean_field_batch(_stage(u), _stage(rhos), cj=cj, ck=ck), self.np)

    def contract_two_body_pairs(self, T, u=None, antisymmetric=False, exchange=False):
        """``S[k,p,q] = sum_rs u[p,q,r,s] T[k,r,s]`` for a stack of two-index amplitudes ``T`` (K, l, l), or one (l, l),
        from ONE read of ``u`` per group of them (``kernels.pair_contract``): the two-body part of the sigma vector of
        a two-particle state, the particle-particle ladder of coupled-cluster doubles.  No conjugation; a real ``u``
        with complex amplitudes stays real.  ``antisymmetric=True`` states that ``T[k] = -T[k]^T`` and needs the basis
        set's anti-symmetrised ``u``: ``kernels.pair_contract_antisym`` then reads a quarter of ``u``.
        ``exchange=True`` is the caller's word that ``u[p,q,r,s] = u[q,p,s,r]`` (the ``u`` of a spatial basis set; any
        amplitudes): ``kernels.pair_contract_exchange`` then reads half of ``u``."""
        from . import kernels
        from .basis_set import _deliver, _stage
        from .sharded_module import is_sharded

        if antisymmetric and exchange:
            raise ValueError("antisymmetric=True and exchange=True name two different kernels: set one of them")
        if antisymmetric and not (u is None and getattr(self._basis_set, "_anti_symmetrized_u", False)):
            raise ValueError("antisymmetric=True needs the basis set's own anti-symmetrised u "
                             "(a GeneralOrbitalSystem built with anti_symmetrize=True)")
        if u is None:
            refuse_vectors_only(self, "contract_two_body_pairs")
        u = self.u if u is None else u
        if is_sharded(u):
            raise NotImplementedError("contract_two_body_pairs does not take a sharded u: "
                                      "the pair contraction is not sharded")
        contract = (kernels.pair_contract_antisym if antisymmetric else
                    kernels.pair_contract_exchange if exchange else kernels.pair_contract)
        return _deliver(contract(_stage(u), _stage(T)), self.np)

    def construct_fock_matrix_from_density(self, rho_qp, h=None, u=None, f=None):
        """``f = h + W(rho)``: ``construct_fock_matrix`` for a general density instead of the reference determinant
        (with rho = that determinant the two agree).  ``f`` may supply the buffer, which is filled and returned."""
        h = self.h if h is None else h
        W = self.construct_mean_field_from_density(rho_qp, u)
        if f is None:
            return h + W
        f.fill(0)
        f += h
        f += W
        return f

    def compute_energy_from_density(self, rho_qp, h=None, u=None):
        """E = h_pq rho_qp + 1/2 W_pq rho_qp + E_nuc: ``compute_reference_energy`` for a general density."""
        np = self.np
        h = self.h if h is None else h
        W = self.construct_mean_field_from_density(rho_qp, u)
        rho = np.asarray(rho_qp)
        return (
            np.einsum("pq,qp->", h, rho) + 0.5 * np.einsum("pq,qp->", W, rho) + self.nuclear_repulsion_energy
        )

    # -- forwarding (system.py:57-71, :217-225)
    def change_module(self, np):
        self.np = np
        self._basis_set.change_module(np)

    def change_basis(self, C, C_tilde=None):
        self._basis_set.change_basis(C, C_tilde)
        self.set_system_size(self.n, self._basis_set.l)

    def change_basis_plan(self, C_tilde_given=False):
        """``change_basis`` with a square ``C`` captured as a HIP graph (``basis_set.ChangeBasisPlan``): ``plan(C)`` instead of
        ``system.change_basis(C)`` in loops over a small basis; ``n``, ``l``, ``o`` and ``v`` do not change."""
        return self._basis_set.change_basis_plan(C_tilde_given)

    def transform_one_body_elements(self, h, C, C_tilde=None):
        return self._basis_set.transform_one_body_elements(h, C, np=self.np, C_tilde=C_tilde)

    def transform_two_body_elements(self, u, C, C_tilde=None):
        return self._basis_set.transform_two_body_elements(u, C, np=self.np, C_tilde=C_tilde)

    def transform_two_body_blocks(self, bras, kets):
        return self._basis_set.transform_two_body_blocks(bras, kets)

    def compute_particle_density(self, rho_qp, C=None, C_tilde=None):
        return self._basis_set.compute_particle_density(rho_qp, C=C, C_tilde=C_tilde)

    # -- read-only views of the basis set (system.py:86-142)
    dim = property(lambda self: self._basis_set.dim)
    grid = property(lambda self: self._basis_set.grid)
    h = property(lambda self: self._basis_set.h, doc="one-body Hamiltonian")
    u = property(lambda self: self._basis_set.u, doc="two-body Hamiltonian")
    s = property(lambda self: self._basis_set.s, doc="overlap matrix")
    position = property(lambda self: self._basis_set.position)
    momentum = property(lambda self: self._basis_set.momentum)
    dipole_moment = property(lambda self: self._basis_set.dipole_moment)
    spf = property(lambda self: self._basis_set.spf)
    bra_spf = property(lambda self: self._basis_set.bra_spf)
    nuclear_repulsion_energy = property(lambda self: self._basis_set.nuclear_repulsion_energy)
    particle_charge = property(lambda self: self._basis_set.particle_charge)

    # -- time-dependent Hamiltonian assembly (system.py:144-215)
    def set_time_evolution_operator(self, time_evolution_operator, add_h_0=True, add_u_0=True):
        if not isinstance(time_evolution_operator, Iterable):
            time_evolution_operator = [time_evolution_operator]
        self._add_h_0 = add_h_0
        self._add_u_0 = add_u_0
        self._time_evolution_operator = [op.set_system(self) for op in time_evolution_operator]

    @property
    def has_one_body_time_evolution_operator(self):
        return any(op.is_one_body_operator for op in self._time_evolution_operator)

    @property
    def has_two_body_time_evolution_operator(self):
        return any(op.is_two_body_operator for op in self._time_evolution_operator)

    def h_t(self, current_time):
        h_0 = self._basis_set.h if self._add_h_0 else self.np.zeros_like(self._basis_set.h)
        if not self.has_one_body_time_evolution_operator:
            return h_0
        return h_0 + sum(op.h_t(current_time) for op in self._time_evolution_operator)

    def u_t(self, current_time):
        refuse_vectors_only(self, "u_t")
        u_0 = self._basis_set.u if self._add_u_0 else self.np.zeros_like(self._basis_set.u)
        if not self.has_two_body_time_evolution_operator:
            return u_0
        return u_0 + sum(op.u_t(current_time) for op in self._time_evolution_operator)

    def copy_system(self):
        """Independent deep copy (system.py:227-250); modules are detached
        during the copy because module objects cannot be deep-copied."""
        np = self.np
        self.np = None
        self._basis_set.np = None
        try:
            new = copy.deepcopy(self)
        finally:
            self.np = np
            self._basis_set.np = np
        new.np = np
        new._basis_set.np = np
        return new
