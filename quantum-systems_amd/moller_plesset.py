"""Second-order Moller-Plesset correlation energy on top of ``transform_two_body_blocks``.

What follows a converged ``HartreeFock.scf()``: the occupied-occupied-virtual-virtual block ``g_ijab = <ij|ab>`` of the
two-body tensor in the canonical orbitals, from ONE block transform (leading index first: one read of ``u``, never the
full l^4 result), and the energy denominators ``D_ijab = e_i + e_j - e_a - e_b``:

    SpatialOrbitalSystem (closed shell, n / 2 = system.n occupied):   E2 = Re sum g_ijab conj(2 g_ijab - g_jiab) / D_ijab
    GeneralOrbitalSystem (n occupied spin orbitals):       E2 = 1/4 sum |G_ijab|^2 / D_ijab,
        G = g for an anti-symmetrised u, else G_ijab = g_ijab - g_ijba

``u`` is taken to be Hermitian, ``<ab|ij> = conj(<ij|ab>)``, so the one block serves both factors of the MP2
numerator.  The reduction over the o^2 v^2 block is plain torch: under a thousandth of the pass over ``u``.
"""

import torch

from .basis_set import _stage, vectors_only
from .general_orbital_system import GeneralOrbitalSystem
from .sharded_module import is_sharded
from .spatial_orbital_system import SpatialOrbitalSystem


def _plain(arr):
    return _stage(arr).as_subclass(torch.Tensor)


def mp2_energy(system, C=None, epsilon=None):
    """MP2 correlation energy of ``system`` (a float).

    With ``C`` (l, l; columns = canonical orbitals, lowest first, ``C^H s C = 1`` as ``HartreeFock.scf`` returns them)
    and the orbital energies ``epsilon`` the system stays in its basis: occupied block ``C[:, :n_occ]``, virtual block
    the rest, bras their conjugate transposes.  With ``C=None`` the system is taken to BE in its canonical
    Hartree-Fock basis already (after ``HartreeFock.change_system_basis()``): the block is a slice of ``u`` and
    ``epsilon`` the diagonal of ``construct_fock_matrix``.  ``u`` is taken to be Hermitian."""
    if not isinstance(system, (SpatialOrbitalSystem, GeneralOrbitalSystem)):
        raise TypeError("mp2_energy needs a SpatialOrbitalSystem or a GeneralOrbitalSystem")
    # occupied orbitals: half the particle number for a closed shell (what a SpatialOrbitalSystem keeps as its n),
    # the particle number for spin orbitals
    n_occ = system.n
    if not 0 < n_occ < system.l:
        raise ValueError(f"{n_occ} occupied of {system.l} orbitals leave no occupied-virtual block")
    if (C is None) != (epsilon is None):
        raise ValueError("give both C and epsilon, or neither (system already in its canonical basis)")
    if is_sharded(system.u):
        raise NotImplementedError("mp2_energy does not take a sharded u: the block transform is not sharded")

    with torch._C.DisableTorchFunctionSubclass():
        if C is None:
            o, v = slice(0, n_occ), slice(n_occ, system.l)
            if vectors_only(system):
                g = system._basis_set.two_body.block(o, o, v, v)
            else:
                g = _plain(system.u)[o, o, v, v]
            f = _plain(system.construct_fock_matrix(system.h, system.u))
            eps = f.diagonal().real.to(torch.float64) if f.is_complex() else f.diagonal().to(torch.float64)
        else:
            C = _plain(C)
            Co, Cv = C[:, :n_occ], C[:, n_occ:]
            bra = Co.conj().transpose(0, 1)
            g = _plain(system.transform_two_body_blocks((bra, bra), (Cv, Cv)))
            eps = _plain(epsilon).real.to(torch.float64) if _plain(epsilon).is_complex() else _plain(epsilon).to(torch.float64)
        eo, ev = eps[:n_occ], eps[n_occ:]
        D = eo[:, None, None, None] + eo[None, :, None, None] - ev[None, None, :, None] - ev[None, None, None, :]
        if isinstance(system, SpatialOrbitalSystem):
            e2 = (g * (2.0 * g - g.transpose(0, 1)).conj() / D).sum()
        else:
            G = g if system._basis_set._anti_symmetrized_u else g - g.transpose(2, 3)
            e2 = 0.25 * ((G * G.conj()).real / D).sum()
        return float(e2.real.item())
