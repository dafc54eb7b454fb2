"""Three electrons in a 2-D quantum dot on one MI355X: what the exact states are good for beyond their energies.

    python examples/exact_quantum_dot_densities.py [shells] [roots] [n]

The quantum dot of ``exact_quantum_dot.py`` (Hartree-Fock spin orbitals, the full space of determinants), then for every
solved state the one- and two-body densities from ``kernels.det_ci_transition_density1`` and ``kernels.det_ci_density2``
(one workgroup per density element strides over the determinants; fixed-order sums) and what follows from them:

  * the energy functional ``sum ht rho + 1/4 sum ut G`` next to the Ritz value of the Davidson iteration: an independent
    check of the state that does not go through the sigma kernel;
  * ``<S^2>``: the Hamiltonian is spin-independent, so non-degenerate states show S (S + 1);
  * the transition dipoles from the ground state, and the natural occupations of the ground state.
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
    n = int(sys.argv[3]) if len(sys.argv) > 3 else 3
    l = shells * (shells + 1) // 2                       # 3 shells -> 6 orbitals -> 12 spin orbitals

    basis = qs.TwoDimensionalHarmonicOscillator(l, 6.0, 61, omega=1.0, np=hip)
    system = qs.GeneralOrbitalSystem(n, basis)
    hf = qs.HartreeFock(system)
    C, _, _ = hf.scf(tol=1e-10, max_iter=200)
    ci = qs.DeterminantCI(system, C)
    E, _ = ci.solve(roots)
    E = torch.as_tensor(E).cpu().tolist()
    print(f"{n} electrons in {2 * l} spin orbitals ({shells} shells): {ci.dim} determinants, {roots} roots, converged: "
          f"{ci.converged} after {ci.iterations} iterations")
    print("  state      Ritz value        E[rho, G]       difference       <S^2>")
    for k in range(roots):
        e = ci.energy_from_densities(k)
        print(f"  {k:5d}  {E[k]:16.10f}  {e:16.10f}  {e - E[k]:10.1e}  {ci.spin_squared(k):12.8f}")
    print(f"    the densities of one state ran [{kernels.last_dispatch()}]")
    print("  transition dipoles <0| r |k>:")
    for k in range(1, roots):
        mu = torch.as_tensor(ci.transition_dipole(0, k)).cpu()
        print(f"    k = {k}: " + "  ".join(f"{complex(x):.6f}" for x in mu.tolist()) + f"   |mu|^2 = {float((mu.abs() ** 2).sum()):.6e}")
    occ, _ = ci.natural_orbitals(0)
    occ = torch.as_tensor(occ).cpu().tolist()
    print("  natural occupations of the ground state: " + " ".join(f"{x:.4f}" for x in occ) + f"   (sum {sum(occ):.10f})")


if __name__ == "__main__":
    main()
