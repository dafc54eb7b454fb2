"""Restricted Hartree-Fock and MP2 for a closed-shell quantum dot at 32 shells (528 orbitals) on one MI355X, without the
two-body tensor.

    python examples/rhf_mp2_32_shell_quantum_dot.py [shells] [electrons] [omega]

At 32 shells ``u`` would be 622 GB.  ``two_body="vectors"`` builds no ``u``: the basis set carries the
factors of the quadrature form, ``u[p,q,r,s] = sum_x L_x[r,p] L_x[q,s]`` with 4000 exact vectors (8.9 GB), and the
mean field of every SCF iteration, the block ``<ij|ab>`` of MP2 and the change to the Hartree-Fock basis run on them.
Printed: the energies, the rank, the bytes held and the time of each step; the basis set's host loops (single-particle
functions, position integrals) are timed with the construction and dominate it."""

import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch

import quantum_systems_amd as qs
from quantum_systems_amd import hip, moller_plesset, two_dim_ho


def clock(t0):
    torch.cuda.synchronize()
    return time.time() - t0


def main():
    shells = int(sys.argv[1]) if len(sys.argv) > 1 else 32
    n = int(sys.argv[2]) if len(sys.argv) > 2 else 12
    omega = float(sys.argv[3]) if len(sys.argv) > 3 else 1.0
    l = shells * (shells + 1) // 2

    t0 = time.time()
    chol = two_dim_ho.coulomb_vectors(l, omega=omega)
    print(f"{n} electrons in {l} orbitals ({shells} shells), omega = {omega}")
    print(f"  Coulomb vectors alone: rank {chol.rank}, {chol.L.numel() * 8 / 1e9:.3f} GB in {clock(t0):.3f} s "
          f"(u would be {8 * l**4 / 1e9:.1f} GB)")
    del chol

    t0 = time.time()
    dot = qs.TwoDimensionalHarmonicOscillator(l, 8.0, 11, omega=omega, coulomb="quadrature", two_body="vectors", np=hip)
    print(f"  basis set (host loops included) in {clock(t0):.2f} s; u is {dot.u}, two_body holds "
          f"{dot.two_body.L.numel() * 8 / 1e9:.3f} GB")

    system = qs.SpatialOrbitalSystem(n, dot)
    hf = qs.HartreeFock(system)
    t0 = time.time()
    _, _, energies = hf.scf(tol=1e-9)
    t_scf = clock(t0)
    print(f"  E_RHF = {energies[-1]:.10f}   (converged {hf.converged} after {hf.iterations} iterations, "
          f"{t_scf:.2f} s, {t_scf / hf.iterations:.3f} s each)")
    t0 = time.time()
    e_mp2 = hf.mp2()
    print(f"  E_MP2 = {energies[-1] + e_mp2:.10f}   (correlation {e_mp2:.10f}, {clock(t0):.3f} s)")
    t0 = time.time()
    hf.change_system_basis()
    print(f"  Hartree-Fock basis: vectors transformed in {clock(t0):.2f} s, "
          f"reference energy {float(qs.array_module.to_host(system.compute_reference_energy()).real):.10f}, "
          f"MP2 there {moller_plesset.mp2_energy(system):.10f}")
    print(f"  peak device memory {torch.cuda.max_memory_allocated() / 1e9:.1f} GB")


if __name__ == "__main__":
    main()
