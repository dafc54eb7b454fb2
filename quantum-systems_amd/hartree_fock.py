"""Self-consistent field on top of ``kernels.mean_field``: restricted Hartree-Fock for a ``SpatialOrbitalSystem``,
general Hartree-Fock for a ``GeneralOrbitalSystem``.

The reference names this step and leaves it out (``change_to_hf_basis`` raises, the ``tdhf`` call is commented out in
general_orbital_system.py:161-169).  Every iteration contracts the WHOLE two-body tensor with the current density --
one ``qs_mean_field`` launch, one read of ``u`` -- and everything else is O(l^3) plumbing on l x l matrices
(``torch.linalg.eigh``, a handful of products).

    hf = HartreeFock(system)
    C, epsilon, energies = hf.scf(tol=1e-10)
    e2 = hf.mp2()                       # second-order correlation energy on the converged orbitals
    omega, X = hf.cis().solve(4)        # lowest excited states (configuration interaction singles)
    hf.change_system_basis()            # system.change_basis(C): the Fock matrix is diagonal now

    chol = system.cholesky_two_body(tol)            # RHF on Cholesky vectors of u (cholesky.py): the mean field is a
    hf = HartreeFock(system, two_body=chol)         # few products on about 4 l matrices, u is not read again

A system whose basis set carries vectors and no ``u`` (the quantum dots' ``two_body="vectors"``) needs no
keyword: ``HartreeFock(system)`` picks ``system._basis_set.two_body`` up and ``scf()`` never touches ``system.u``.

``system.change_to_hf_basis()`` keeps raising ``NotImplementedError`` as in the reference.
"""

import numpy
import torch

from . import kernels, sharded_basis
from .basis_set import _deliver, _stage
from .cholesky import CholeskyTwoBody
from .general_orbital_system import GeneralOrbitalSystem
from .sharded_module import is_sharded
from .spatial_orbital_system import SpatialOrbitalSystem


def _dagger(A):
    return A.conj().transpose(0, 1)


class HartreeFock:
    """SCF driver: core-Hamiltonian guess, Loewdin orthogonalisation with the basis set's overlap ``s``, DIIS on
    ``F rho s - s rho F``.  ``system.n`` lowest orbitals are occupied (doubly for spatial orbitals)."""

    def __init__(self, system, two_body=None):
        if isinstance(system, SpatialOrbitalSystem):
            self.occupation = 2.0
        elif isinstance(system, GeneralOrbitalSystem):
            self.occupation = 1.0
        else:
            raise TypeError("HartreeFock needs a SpatialOrbitalSystem (RHF) or a GeneralOrbitalSystem (GHF)")
        if two_body is None and isinstance(system, SpatialOrbitalSystem):
            # a basis set that carries vectors (two_dim_ho's two_body="vectors": no u at all) brings its own
            two_body = getattr(system._basis_set, "two_body", None)
        if two_body is not None:
            # Cholesky vectors (cholesky.CholeskyTwoBody) of the system's plain u: the mean field is a few products on
            # them and u is never read.  RHF only: the vectors of a spin-expanded, anti-symmetrised tensor do not exist.
            if not isinstance(system, SpatialOrbitalSystem):
                raise TypeError("two_body= (Cholesky vectors) is supported for a SpatialOrbitalSystem (RHF) only")
            if not isinstance(two_body, CholeskyTwoBody):
                raise TypeError("two_body must be a cholesky.CholeskyTwoBody")
            if two_body.m != system.l:
                raise ValueError(f"two_body has {two_body.m} orbitals, the system {system.l}")
        self.two_body = two_body
        self.system = system
        self.C = self.epsilon = None
        self.energies = []
        self.converged = False
        self.iterations = 0
        self._basis_changed = False

    # -- the one O(l^4) step of an iteration
    def _mean_field(self, u, rho):
        cj, ck = self.system._mean_field_weights()
        if self.two_body is not None:
            return self.two_body.mean_field(rho, cj=cj, ck=ck)
        if is_sharded(u):
            return sharded_basis.mean_field(u, rho, cj, ck, self.system.np).as_subclass(torch.Tensor)
        return kernels.mean_field(u, rho, cj=cj, ck=ck)

    def _density(self, C):
        Co = C[:, : self.system.n]
        return (self.occupation * (Co @ _dagger(Co))).contiguous()

    def scf(self, tol=1e-10, max_iter=100, diis_vectors=8):
        """Iterate to ``max |X^H (F rho s - s rho F) X| < tol`` (X = s^-1/2).  Returns ``(C, epsilon, energies)``:
        the coefficients (columns = canonical orbitals, ``C^H s C = 1``) and orbital energies of the final Fock matrix
        in the system's array module, and the list of energies E[rho_k], one per iteration (the first is the
        core-guess determinant's)."""
        system = self.system
        with torch._C.DisableTorchFunctionSubclass():
            if self.two_body is not None:
                u = None                                                   # the vectors stand in: u is never touched
            else:
                u = system.u if is_sharded(system.u) else _stage(system.u).as_subclass(torch.Tensor)
            h = _stage(system.h).as_subclass(torch.Tensor)
            s = _stage(system.s).as_subclass(torch.Tensor)
            two_body_dtype = self.two_body.L.dtype if u is None else u.dtype
            dt = torch.complex128 if torch.complex128 in (h.dtype, s.dtype, two_body_dtype) else torch.float64
            h, s = h.to(dt), s.to(dt)
            e_nuc = system.nuclear_repulsion_energy

            sv, sU = torch.linalg.eigh(s)
            X = (sU * sv.rsqrt().to(dt)) @ _dagger(sU)                   # s^-1/2
            Xh = _dagger(X)

            def diagonalise(F):
                eps, Cp = torch.linalg.eigh(Xh @ F @ X)
                return eps, X @ Cp

            epsilon, C = diagonalise(h)                                   # core-Hamiltonian guess
            rho = self._density(C)
            self.energies, self.converged = [], False
            focks, errors = [], []
            for it in range(1, max_iter + 1):
                self.iterations = it
                W = self._mean_field(u, rho).to(dt)
                F = h + W
                rho_t = rho.transpose(0, 1)
                energy = ((h + 0.5 * W) * rho_t).sum() + e_nuc
                self.energies.append(float(energy.real.item()))
                err = Xh @ (F @ rho @ s - s @ rho @ F) @ X
                if float(err.abs().max().item()) < tol:
                    self.converged = True
                    break
                if diis_vectors and diis_vectors > 1:
                    focks.append(F)
                    errors.append(err)
                    del focks[:-diis_vectors], errors[:-diis_vectors]
                    F = self._extrapolate(focks, errors)
                epsilon, C = diagonalise(F)
                rho = self._density(C)
            # canonical orbitals of the last Fock matrix itself (not of an extrapolated one)
            epsilon, C = diagonalise(F if self.converged else h + self._mean_field(u, rho).to(dt))
            self.C, self.epsilon = _deliver(C.contiguous(), system.np), _deliver(epsilon, system.np)
        return self.C, self.epsilon, self.energies

    @staticmethod
    def _extrapolate(focks, errors):
        """Pulay's DIIS: the combination of the stored Fock matrices whose combined error is smallest."""
        m = len(focks)
        if m < 2:
            return focks[-1]
        B = numpy.zeros((m + 1, m + 1))
        for i in range(m):
            for j in range(i + 1):
                B[i, j] = B[j, i] = float((errors[i].conj() * errors[j]).sum().real.item())
        B[:m, m] = B[m, :m] = -1.0
        rhs = numpy.zeros(m + 1)
        rhs[m] = -1.0
        scale = max(B[:m, :m].diagonal().max(), 1e-300)
        B[:m, :m] /= scale
        c = numpy.linalg.lstsq(B, rhs, rcond=None)[0][:m]
        return sum(float(ci) * Fi for ci, Fi in zip(c, focks))

    def change_system_basis(self):
        """``system.change_basis(C)`` with the converged coefficients: the system's Fock matrix becomes diagonal."""
        if self.C is None:
            raise RuntimeError("run scf() first")
        self.system.change_basis(self.C)
        self._basis_changed = True
        return self.system

    def mp2(self):
        """Second-order Moller-Plesset correlation energy on the converged orbitals:
        ``moller_plesset.mp2_energy(system, C, epsilon)``."""
        from .moller_plesset import mp2_energy

        if self.C is None:
            raise RuntimeError("run scf() first")
        if self._basis_changed:
            raise RuntimeError(
                "the system is in its Hartree-Fock basis already (change_system_basis): C no longer refers to it -- "
                "call moller_plesset.mp2_energy(system)")
        return mp2_energy(self.system, self.C, self.epsilon)

    def cis(self, **kw):
        """Configuration interaction singles on the converged orbitals:
        ``configuration_interaction.CIS(system, C, epsilon, **kw)``."""
        from .configuration_interaction import CIS

        if self.C is None:
            raise RuntimeError("run scf() first")
        if self._basis_changed:
            raise RuntimeError(
                "the system is in its Hartree-Fock basis already (change_system_basis): C no longer refers to it -- "
                "call configuration_interaction.CIS(system)")
        return CIS(self.system, self.C, self.epsilon, **kw)

    def string_ci(self, **kw):
        """Exact states of a restricted (``SpatialOrbitalSystem``) solution in the converged orbitals:
        ``string_ci.StringCI(system, C, **kw)``."""
        from .string_ci import StringCI

        if self.C is None:
            raise RuntimeError("run scf() first")
        if self._basis_changed:
            raise RuntimeError(
                "the system is in its Hartree-Fock basis already (change_system_basis): C no longer refers to it -- "
                "call string_ci.StringCI(system)")
        return StringCI(self.system, self.C, **kw)

    def ccd(self, **kw):
        """Coupled-cluster doubles on the converged orbitals: ``coupled_cluster.RCCD(system, C, epsilon, **kw)`` for a
        closed shell (``SpatialOrbitalSystem``), ``coupled_cluster.CCD(system, C, epsilon, **kw)`` for a general
        (``GeneralOrbitalSystem``) solution."""
        from .coupled_cluster import CCD, RCCD
        from .spatial_orbital_system import SpatialOrbitalSystem

        cls = RCCD if isinstance(self.system, SpatialOrbitalSystem) else CCD
        if self.C is None:
            raise RuntimeError("run scf() first")
        if self._basis_changed:
            raise RuntimeError(
                "the system is in its Hartree-Fock basis already (change_system_basis): C no longer refers to it -- "
                f"call coupled_cluster.{cls.__name__}(system)")
        return cls(self.system, self.C, self.epsilon, **kw)

    def ccsd(self, **kw):
        """Closed-shell coupled-cluster singles and doubles on the converged orbitals:
        ``coupled_cluster.RCCSD(system, C, epsilon, **kw)``, whose ``triples()`` is (T).  Spatial systems only."""
        from .coupled_cluster import RCCSD
        from .spatial_orbital_system import SpatialOrbitalSystem

        if not isinstance(self.system, SpatialOrbitalSystem):
            raise TypeError("ccsd() needs a SpatialOrbitalSystem: coupled_cluster.RCCSD is the closed-shell method")
        if self.C is None:
            raise RuntimeError("run scf() first")
        if self._basis_changed:
            raise RuntimeError(
                "the system is in its Hartree-Fock basis already (change_system_basis): C no longer refers to it -- "
                "call coupled_cluster.RCCSD(system)")
        return RCCSD(self.system, self.C, self.epsilon, **kw)
