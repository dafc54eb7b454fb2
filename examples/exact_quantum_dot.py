"""Three electrons in a 2-D quantum dot on one MI355X: Hartree-Fock, MP2 and the EXACT states in the same basis.

    python examples/exact_quantum_dot.py [shells] [roots] [n]

Spin-doubles the harmonic-oscillator basis, runs the general Hartree-Fock driver and ``hf.mp2()``, then
``DeterminantCI`` on the Hartree-Fock spin orbitals: the full space of C(m, n) Slater determinants, a block Davidson
iteration whose sigma vectors come from ONE ``kernels.det_ci_sigma`` call per step (every determinant's single and
double excitations walked once per group of trial vectors; H is never stored).  The default, 4 shells (m = 20 spin
orbitals) and 3 electrons, is a space of 1140 determinants.
"""

import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch

import quantum_systems_amd as qs
from quantum_systems_amd import hip, kernels


def main():
    shells = int(sys.argv[1]) if len(sys.argv) > 1 else 4
    roots = int(sys.argv[2]) if len(sys.argv) > 2 else 3
    n = int(sys.argv[3]) if len(sys.argv) > 3 else 3
    l = shells * (shells + 1) // 2                       # 4 shells -> 10 orbitals -> 20 spin orbitals

    basis = qs.TwoDimensionalHarmonicOscillator(l, 6.0, 61, omega=1.0, np=hip)
    system = qs.GeneralOrbitalSystem(n, basis)
    hf = qs.HartreeFock(system)
    C, epsilon, energies = hf.scf(tol=1e-10, max_iter=200)
    e2 = hf.mp2()
    print(f"{n} electrons in {2 * l} spin orbitals ({shells} shells), GHF converged: {hf.converged} after "
          f"{hf.iterations} iterations")
    print(f"  E_HF    = {float(torch.as_tensor(energies[-1]).real):.10f}")
    print(f"  E_MP2   = {float(torch.as_tensor(energies[-1] + e2).real):.10f}")

    ci = qs.DeterminantCI(system, C)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    E, _ = ci.solve(roots)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    E = torch.as_tensor(E).cpu().tolist()
    print(f"  E_exact = {E[0]:.10f}   (full space of {ci.dim} determinants)")
    print("  lowest states: " + "  ".join(f"{e:.10f}" for e in E))
    print(f"    converged: {ci.converged} after {ci.iterations} iterations in {dt:.2f} s, vectors per step "
          f"{ci.sigma_history}, largest residual {max(ci.residuals):.1e}; last step ran [{kernels.last_dispatch()}]")
    rho = torch.as_tensor(ci.one_body_density(0))
    print(f"  trace of the ground state's one-body density: {float(rho.diagonal().sum().real):.12f}")


if __name__ == "__main__":
    main()
