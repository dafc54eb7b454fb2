"""``SpatialOrbitalSystem``: closed-shell system over spatial orbitals
(reference: quantum_systems/spatial_orbital_system.py)."""

import copy

import torch

from . import sharded_basis
from .basis_set import refuse_vectors_only, vectors_only
from .general_orbital_system import GeneralOrbitalSystem
from .sharded_module import is_sharded
from .system import QuantumSystem


class SpatialOrbitalSystem(QuantumSystem):
    """``n`` particles in doubly occupied spatial orbitals; internally the
    number of occupied basis functions is ``n // 2``
    (spatial_orbital_system.py:40-50).

    >>> from quantum_systems_amd import SpatialOrbitalSystem, BasisSet
    >>> SpatialOrbitalSystem(4, BasisSet(20, 2)).n
    2
    """

    def __init__(self, n, basis_set, **kwargs):
        assert n % 2 == 0, "n must be divisable by 2 to be a closed-shell system"
        assert not basis_set.includes_spin, (
            f"{self.__class__.__name__} only supports basis sets without "
            + "spin-dependence."
        )
        super().__init__(n // 2, basis_set, **kwargs)

    def construct_general_orbital_system(self, a=[1, 0], b=[0, 1], anti_symmetrize=True):
        """Spin-doubled copy of this system: every spatial orbital yields an
        alpha and a beta spin orbital, ``2n`` occupied, two-body elements
        anti-symmetrised by default.  This system is left intact
        (spatial_orbital_system.py:52-104)."""
        # The reference deep-copies the whole basis set first (spatial_orbital_system.py:89-91,
        # basis_set.py:784-805) so that this system stays intact.  The spin doubling never modifies the
        # spatial ``u`` -- it reads it and writes the 16x larger spin tensor -- so the copy of ``u`` (34 GB at
        # l = 256, and the one thing that does not fit when ``u`` is sharded over the node) is elided: the
        # copy shares the tensor, everything O(l^2) is copied as upstream.
        refuse_vectors_only(self, "construct_general_orbital_system")
        bs = self._basis_set
        u = bs._u
        bs._u = None
        try:
            twin = bs.copy_basis()
        finally:
            bs._u = u
        twin._u = u
        gos = GeneralOrbitalSystem(self.n * 2, twin, a=a, b=b, anti_symmetrize=anti_symmetrize)
        if self._time_evolution_operator is not None:
            gos.set_time_evolution_operator(copy.deepcopy(self._time_evolution_operator))
        return gos

    def compute_reference_energy(self, h=None, u=None):
        """E0 = 2 h_ii + 2 u_ijij - u_ijji + E_nuc
        (spatial_orbital_system.py:106-150)."""
        o = self.o
        np = self.np
        h = self.h if h is None else h
        if u is None and vectors_only(self):
            # no u: E0 = tr((h + W / 2) rho) with the mean field W of the reference determinant's density
            W = self._reference_mean_field()
            return 2 * np.trace(h[o, o]) + np.trace(W[o, o]) + self.nuclear_repulsion_energy
        u = self.u if u is None else u
        if is_sharded(u):       # slab-local sums + one all-reduce of a single number
            return sharded_basis.compute_reference_energy(h, u, self.n, False, self.nuclear_repulsion_energy)
        return (
            2 * np.trace(h[o, o])
            + 2 * np.trace(np.trace(u[o, o, o, o], axis1=1, axis2=3))
            - np.trace(np.trace(u[o, o, o, o], axis1=1, axis2=2))
            + self.nuclear_repulsion_energy
        )

    def _reference_mean_field(self):
        """``2 u_piqi - u_piiq`` from the basis set's vectors: their mean field of the reference determinant's density,
        2 on the occupied diagonal."""
        from .basis_set import _deliver

        L = self._basis_set.two_body.L
        rho = torch.zeros((self.l, self.l), dtype=L.dtype, device=L.device)
        rho.diagonal()[: self.n] = 2.0
        cj, ck = self._mean_field_weights()
        return _deliver(self._basis_set.two_body.mean_field(rho, cj=cj, ck=ck), self.np)

    def construct_fock_matrix(self, h, u=None, f=None):
        """Restricted closed-shell Fock matrix
        f_pq = h_pq + 2 u_piqi - u_piiq (spatial_orbital_system.py:152-190).  ``u=None``: the basis set's ``u``, or its
        vectors where it holds no ``u``."""
        np = self.np
        o = self.o
        if u is None and vectors_only(self):
            W = self._reference_mean_field()
            if f is None:
                return h + W
            f.fill(0)
            f += h
            f += W
            return f
        u = self.u if u is None else u
        if is_sharded(u):       # slab-local rows / partial sums + l*l numbers over the node
            return sharded_basis.construct_fock_matrix(h, u, self.n, False, f=f)
        if f is None:
            f = np.zeros_like(h)
        f.fill(0)
        f += h
        f += 2 * np.einsum("piqi -> pq", u[:, o, :, o])
        f -= np.einsum("piiq -> pq", u[:, o, o, :])
        return f

    def _mean_field_weights(self):
        # closed shell, spin-summed density: f = h + J(rho) - K(rho) / 2
        return 1.0, -0.5

    def cholesky_two_body(self, tol, max_rank=None):
        """Cholesky vectors of this system's two-body tensor: ``cholesky.decompose(self, tol, max_rank)``."""
        from .cholesky import decompose

        return decompose(self, tol, max_rank=max_rank)

    def change_to_hf_basis(self, *args, **kwargs):
        raise NotImplementedError("There is currently no RHF implementation")
