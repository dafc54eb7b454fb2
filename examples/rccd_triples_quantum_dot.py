"""Perturbative triples on closed-shell coupled-cluster doubles for a 2-D quantum dot on one MI355X: RHF, RCCD, +T.

    python examples/rccd_triples_quantum_dot.py [shells] [omega]

For 2 and for 6 electrons: the restricted SCF, ``HartreeFock.ccd()`` (``coupled_cluster.RCCD``), its ``solve()`` and
then ``triples()``: the correction ``E_T = sum |<mu| H T2 |0>|^2 / D_mu`` over the triply excited determinants, formed
from products on the GEMM dispatcher and ONE read of them by ``kernels.triples_energy``.  Beside the three energies
the exact one of the same basis (``StringCI``: all determinants).  Two electrons have no triple excitation: E_T = 0."""

import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch

import quantum_systems_amd as qs
from quantum_systems_amd import hip


def run(n, l, shells, omega):
    spatial = qs.SpatialOrbitalSystem(n, qs.TwoDimensionalHarmonicOscillator(l, 6.0, 61, omega=omega, np=hip))
    hf = qs.HartreeFock(spatial)
    _, _, energies = hf.scf(tol=1e-10)
    print(f"{n} electrons in {l} orbitals ({shells} shells), omega = {omega}: RHF converged {hf.converged} "
          f"after {hf.iterations} iterations")
    rccd = hf.ccd()
    e_rccd = rccd.solve(tol=1e-8, max_iter=200)
    e_t = rccd.triples()
    exact = hf.string_ci()
    e, _ = exact.solve(1, tol=1e-9)
    e = float(torch.as_tensor(e).cpu()[0])
    print(f"  E_RHF      = {energies[-1]:.10f}")
    print(f"  E_RCCD     = {energies[-1] + e_rccd:.10f}   (correlation {e_rccd:.10f}, converged {rccd.converged} after "
          f"{rccd.iterations} iterations; off the exact energy by {energies[-1] + e_rccd - e:+.2e})")
    print(f"  E_RCCD+T   = {energies[-1] + e_rccd + e_t:.10f}   (E_T {e_t:.10f}, {len(rccd.triples_passes)} pass(es); "
          f"off the exact energy by {energies[-1] + e_rccd + e_t - e:+.2e})")
    print(f"  E_exact    = {e:.10f}   (all determinants)")


def main():
    shells = int(sys.argv[1]) if len(sys.argv) > 1 else 4
    omega = float(sys.argv[2]) if len(sys.argv) > 2 else 1.0
    l = shells * (shells + 1) // 2                       # 4 shells -> 10 orbitals
    for n in (2, 6):
        run(n, l, shells, omega)


if __name__ == "__main__":
    main()
