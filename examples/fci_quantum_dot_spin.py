"""Which exact state of a 2-D quantum dot is a singlet and which a triplet: restricted Hartree-Fock, spin-free string CI
in the S_z = 0 sector, and <S^2> and the energy functional of every root from its densities.

    python examples/fci_quantum_dot_spin.py [shells] [roots] [n_pairs]

A spin-restricted solver in an S_z sector returns the multiplets interleaved.  ``StringCI.spin_squared`` applies
S^2 = S_z (S_z + 1) + N_beta - sum_pq E^alpha_qp E^beta_pq through the two replacement tables
(``kernels.string_ci_spin_squared``), and ``StringCI.energy_from_densities`` rebuilds the energy from the spin-summed
one- and two-body densities, sum ht rho + 1/2 sum ut Gamma, where Gamma is ONE Gram product of two expanded panels on
the GEMM dispatcher (``kernels.string_ci_density2``).  Default: 3 shells, 6 spatial orbitals, 2 + 2 electrons.
"""

import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch

import quantum_systems_amd as qs
from quantum_systems_amd import hip, kernels


def main():
    shells = int(sys.argv[1]) if len(sys.argv) > 1 else 3
    roots = int(sys.argv[2]) if len(sys.argv) > 2 else 4
    pairs = int(sys.argv[3]) if len(sys.argv) > 3 else 2
    l = shells * (shells + 1) // 2

    basis = qs.TwoDimensionalHarmonicOscillator(l, 6.0, 61, omega=1.0, np=hip)
    system = qs.SpatialOrbitalSystem(2 * pairs, basis)
    hf = qs.HartreeFock(system)
    hf.scf(tol=1e-10, max_iter=200)
    print(f"{2 * pairs} electrons in {l} spatial orbitals ({shells} shells), RHF converged: {hf.converged} after "
          f"{hf.iterations} iterations")

    ci = hf.string_ci()
    E, _ = ci.solve(n_roots=roots)
    E = torch.as_tensor(E).cpu().tolist()
    print(f"  {ci.na} x {ci.nb} = {ci.dim} determinants, converged: {ci.converged} after {ci.iterations} iterations")
    print("  root           energy        <S^2>   2S+1   energy_from_densities - E")
    for k in range(roots):
        print(f"  {k:4d}  {E[k]:15.10f}  {ci.spin_squared(k):11.8f}  {ci.spin_multiplicity(k):5.3f}   "
              f"{ci.energy_from_densities(k) - E[k]:+.2e}")
    ci.two_body_density(0)
    print(f"  two_body_density ran [{kernels.last_dispatch()}]")


if __name__ == "__main__":
    main()
