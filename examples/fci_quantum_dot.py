"""Electrons in a 2-D quantum dot on one MI355X, in SPATIAL orbitals: restricted Hartree-Fock, MP2 and the EXACT states
by spin-free string CI, without spin-doubling the two-body tensor.

    python examples/fci_quantum_dot.py [shells] [roots] [n_pairs]

``StringCI`` works on the RHF orbitals of the ``SpatialOrbitalSystem``: a state is ``c[Ia, Ib]`` over alpha and beta
occupation strings, and every sigma vector of the block Davidson iteration is one expand, ONE dense product
``W . D`` (m^2 x m^2 by m^2 x dim) on the GEMM dispatcher and one fold (``kernels.string_ci_sigma``).  At the default
size -- 3 shells, 6 spatial orbitals, 2 + 2 electrons, 225 determinants -- the same energies are computed a second time
by ``DeterminantCI`` on the S_z = 0 sector of the spin-doubled system.
"""

import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch

import quantum_systems_amd as qs
from quantum_systems_amd import hip, kernels


def main():
    shells = int(sys.argv[1]) if len(sys.argv) > 1 else 3
    roots = int(sys.argv[2]) if len(sys.argv) > 2 else 3
    pairs = int(sys.argv[3]) if len(sys.argv) > 3 else 2
    l = shells * (shells + 1) // 2

    basis = qs.TwoDimensionalHarmonicOscillator(l, 6.0, 61, omega=1.0, np=hip)
    system = qs.SpatialOrbitalSystem(2 * pairs, basis)
    hf = qs.HartreeFock(system)
    C, epsilon, energies = hf.scf(tol=1e-10, max_iter=200)
    e2 = hf.mp2()
    print(f"{2 * pairs} electrons in {l} spatial orbitals ({shells} shells), RHF converged: {hf.converged} after "
          f"{hf.iterations} iterations")
    print(f"  E_HF    = {float(torch.as_tensor(energies[-1]).real):.10f}")
    print(f"  E_MP2   = {float(torch.as_tensor(energies[-1] + e2).real):.10f}")

    ci = hf.string_ci()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    E, _ = ci.solve(roots)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    E = torch.as_tensor(E).cpu().tolist()
    print(f"  E_exact = {E[0]:.10f}   ({ci.na} x {ci.nb} = {ci.dim} determinants)")
    print("  lowest states: " + "  ".join(f"{e:.10f}" for e in E))
    print(f"    converged: {ci.converged} after {ci.iterations} iterations in {dt:.2f} s, vectors per step "
          f"{ci.sigma_history}; last step ran [{kernels.last_dispatch()}]")
    occ, _ = ci.natural_orbitals(0)
    print("  natural occupations: " + " ".join(f"{x:.6f}" for x in torch.as_tensor(occ).cpu().tolist()))

    if 2 * l <= 24:                                       # a size where the spin-orbital route runs as well
        general = system.construct_general_orbital_system()
        C2 = torch.kron(torch.as_tensor(C).as_subclass(torch.Tensor), torch.eye(2, dtype=torch.float64, device="cuda"))
        det = qs.DeterminantCI(general, hip.asarray(C2), dets=qs.sz_sector(2 * l, 2 * pairs, 0))
        Ed, _ = det.solve(roots)
        Ed = torch.as_tensor(Ed).cpu().tolist()
        print(f"  DeterminantCI on {2 * l} spin orbitals, S_z = 0: " + "  ".join(f"{e:.10f}" for e in Ed))
        print(f"    largest difference of the two routes: {max(abs(a - b) for a, b in zip(E, Ed)):.2e}")


if __name__ == "__main__":
    main()
