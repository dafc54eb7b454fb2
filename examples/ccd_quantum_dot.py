"""Coupled-cluster doubles for a 2-D quantum dot on one MI355X: RHF, then CCD in spin orbitals.

    python examples/ccd_quantum_dot.py [shells] [n] [omega]

Runs the restricted SCF on the spatial orbitals, doubles the basis to spin orbitals with an anti-symmetrised ``u``
(``construct_general_orbital_system``), and solves the CCD equations on the RHF determinant with
``coupled_cluster.CCD``: every iteration is ONE pass of ``kernels.pair_contract_antisym`` over the quarter of the
untransformed ``u`` that its symmetries do not repeat, plus small products on the occupied-virtual blocks.  Prints the
MP2 energy (the start of the iteration), the CCD energy and -- for two particles, where CCD on the doubles is exact up
to the singles -- the exact energy of ``TwoParticleCI``."""

import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch

import quantum_systems_amd as qs
from quantum_systems_amd import hip


def main():
    shells = int(sys.argv[1]) if len(sys.argv) > 1 else 5
    n = int(sys.argv[2]) if len(sys.argv) > 2 else 2
    omega = float(sys.argv[3]) if len(sys.argv) > 3 else 1.0
    l = shells * (shells + 1) // 2                       # 5 shells -> 15 orbitals, 30 spin orbitals

    spatial = qs.SpatialOrbitalSystem(n, qs.TwoDimensionalHarmonicOscillator(l, 6.0, 61, omega=omega, np=hip))
    hf = qs.HartreeFock(spatial)
    C, epsilon, energies = hf.scf(tol=1e-10)
    print(f"{n} electrons in {l} orbitals ({shells} shells), omega = {omega}: RHF converged {hf.converged} "
          f"after {hf.iterations} iterations")
    print(f"  E_RHF  = {energies[-1]:.10f}")

    system = spatial.construct_general_orbital_system(anti_symmetrize=True)
    # spin orbital 2 p + sigma: the RHF orbitals for either spin, the n lowest occupied
    two = torch.eye(2, dtype=torch.float64, device="cuda")
    C2 = torch.kron(torch.as_tensor(C).as_subclass(torch.Tensor), two.to(torch.as_tensor(C).dtype))
    eps2 = torch.as_tensor(epsilon).as_subclass(torch.Tensor).repeat_interleave(2)
    ccd = qs.CCD(system, hip.asarray(C2.contiguous()), hip.asarray(eps2.contiguous()))
    e_mp2 = ccd.energy()
    e_ccd = ccd.solve(tol=1e-8, max_iter=200)
    print(f"  E_MP2  = {energies[-1] + e_mp2:.10f}   (correlation {e_mp2:.10f})")
    print(f"  E_CCD  = {energies[-1] + e_ccd:.10f}   (correlation {e_ccd:.10f}; converged {ccd.converged} "
          f"after {ccd.iterations} iterations, residual {ccd.residuals[-1]:.1e})")
    if n == 2:
        exact = qs.TwoParticleCI(spatial, C)
        e, _ = exact.solve(1, tol=1e-9)
        e = float(torch.as_tensor(e).cpu()[0])
        print(f"  E_exact = {e:.10f}   (singlet ground state; CCD leaves {e_ccd + energies[-1] - e:.2e} to the singles)")


if __name__ == "__main__":
    main()
