"""Two electrons in a 2-D quantum dot on one MI355X: Hartree-Fock, MP2 and the EXACT states in the same basis.

    python examples/two_electron_quantum_dot.py [shells] [roots]

Runs the SCF driver and ``hf.mp2()``, then ``TwoParticleCI`` on the Hartree-Fock orbitals: a block Davidson iteration
whose sigma vectors contract the untransformed two-body tensor with the trial amplitudes, all vectors of a step in ONE
``kernels.pair_contract`` call (one read of ``u`` per group of them).  With omega = 1 the ground state of the full
problem is E = 3 exactly; the basis reaches it from above.
"""

import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch

import quantum_systems_amd as qs
from quantum_systems_amd import hip, kernels


def main():
    shells = int(sys.argv[1]) if len(sys.argv) > 1 else 6
    roots = int(sys.argv[2]) if len(sys.argv) > 2 else 4
    l = shells * (shells + 1) // 2                       # 6 shells -> 21 orbitals

    basis = qs.TwoDimensionalHarmonicOscillator(l, 6.0, 61, omega=1.0, np=hip)
    system = qs.SpatialOrbitalSystem(2, basis)
    hf = qs.HartreeFock(system)
    C, epsilon, energies = hf.scf(tol=1e-10)
    e2 = hf.mp2()
    print(f"2 electrons in {l} orbitals ({shells} shells), RHF converged: {hf.converged} after {hf.iterations} iterations")
    print(f"  E_HF          = {energies[-1]:.10f}")
    print(f"  E_HF + E_MP2  = {energies[-1] + e2:.10f}")

    ci = qs.TwoParticleCI(system, C)
    for spin in ("singlet", "triplet"):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        E, _ = ci.solve(roots, spin=spin)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        E = torch.as_tensor(E).cpu().tolist()
        print(f"  exact {spin}s  = " + "  ".join(f"{e:.10f}" for e in E))
        print(f"    converged: {ci.converged} after {ci.iterations} iterations in {dt:.2f} s, vectors per step "
              f"{ci.sigma_history}, largest residual {max(ci.residuals):.1e}; last step ran [{kernels.last_dispatch()}]")


if __name__ == "__main__":
    main()
