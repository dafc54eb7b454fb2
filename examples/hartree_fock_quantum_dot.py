"""Restricted Hartree-Fock for a 2-D quantum dot on one MI355X.

    python examples/hartree_fock_quantum_dot.py [shells] [n]

Builds the Fock-Darwin basis (Coulomb elements generated on the GPU), runs the SCF driver -- every iteration is ONE
pass over the two-body tensor (``kernels.mean_field``) -- and rotates the system into the Hartree-Fock basis, where
the Fock matrix is diagonal.  For omega = 1 the literature quotes RHF energies of about 3.16 (n = 2) and 20.72
(n = 6) Hartree in large bases; a small basis sits above them.
"""

import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch

import quantum_systems_amd as qs
from quantum_systems_amd import hip, kernels


def main():
    shells = int(sys.argv[1]) if len(sys.argv) > 1 else 7
    n = int(sys.argv[2]) if len(sys.argv) > 2 else 6
    l = shells * (shells + 1) // 2                       # 7 shells -> 28 orbitals

    basis = qs.TwoDimensionalHarmonicOscillator(l, 6.0, 61, omega=1.0, np=hip)
    system = qs.SpatialOrbitalSystem(n, basis)
    print(f"{n} electrons in {l} orbitals ({shells} shells); reference determinant: "
          f"{complex(system.compute_reference_energy().cpu()).real:.8f}")

    hf = qs.HartreeFock(system)
    C, epsilon, energies = hf.scf(tol=1e-10)
    print(f"RHF converged: {hf.converged} after {hf.iterations} iterations, kernels per iteration: {kernels.last_dispatch()}")
    for k, e in enumerate(energies):
        print(f"  iteration {k:2d}   E = {e:.10f}")

    hf.change_system_basis()                             # system.change_basis(C)
    f = torch.as_tensor(system.construct_fock_matrix(system.h, system.u))
    off = (f - torch.diag(torch.diagonal(f))).abs().max()
    print(f"Hartree-Fock basis: largest off-diagonal Fock element {float(off):.2e}")
    print(f"orbital energies: {[round(float(x), 6) for x in torch.as_tensor(epsilon)[:n + 2]]}")
    print(f"reference energy in the new basis: {complex(system.compute_reference_energy().cpu()).real:.10f}")


if __name__ == "__main__":
    main()
