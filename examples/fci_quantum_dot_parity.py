"""The lowest singlets and the lowest triplets of a 2-D quantum dot as two solves: restricted Hartree-Fock, then spin-free
string CI restricted to one parity under the exchange of the two spins.

    python examples/fci_quantum_dot_parity.py [shells] [roots] [n_pairs]

With ``n_up == n_down`` the transposition ``(P c)[Ia, Ib] = c[Ib, Ia]`` commutes with ``H`` and ``S^2``, and a state of spin
``S`` has ``c = (-1)^S c^T``.  ``StringCI(..., spin_parity=+1)`` iterates inside the even subspace (singlets, and quintets
further up), ``spin_parity=-1`` inside the odd one (triplets): no guessing how many roots of the interleaved spectrum hold
four singlets.  Every ``H c`` runs on ``kernels.string_ci_sigma_sym``, which forms only the lower triangle of the expanded
intermediate: half of the product and half of the workspace.  Default: 3 shells, 6 spatial orbitals, 2 + 2 electrons.
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

    for parity, name in ((+1, "even S (singlets first)"), (-1, "odd S (triplets first)")):
        ci = hf.string_ci(spin_parity=parity)
        n = ci.na
        E, _ = ci.solve(n_roots=roots)
        E = torch.as_tensor(E).cpu().tolist()
        print(f"spin_parity = {parity:+d}, {name}: {n * (n + parity) // 2} of {ci.dim} dimensions, converged: {ci.converged} "
              f"after {ci.iterations} iterations")
        print("  root           energy        <S^2>   2S+1")
        for k in range(roots):
            print(f"  {k:4d}  {E[k]:15.10f}  {ci.spin_squared(k):11.8f}  {ci.spin_multiplicity(k):5.3f}")
    ci.sigma(ci._c)
    print(f"  sigma ran [{kernels.last_dispatch()}]")


if __name__ == "__main__":
    main()
