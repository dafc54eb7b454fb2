"""Closed-shell coupled-cluster doubles for a 2-D quantum dot on one MI355X, on the SPATIAL orbitals: RHF, then RCCD.

    python examples/rccd_quantum_dot.py [shells] [omega]

For 2 and for 6 electrons: the restricted SCF, then ``HartreeFock.ccd()``, which for a ``SpatialOrbitalSystem`` is
``coupled_cluster.RCCD``: every iteration is ONE pass of ``kernels.pair_contract_exchange`` over the half of the
untransformed spatial ``u`` that its particle-exchange symmetry does not repeat, plus small products on the
occupied-virtual blocks.  Beside it the route through spin orbitals -- the basis doubled with an anti-symmetrised ``u``
16 times the size (``construct_general_orbital_system``), GHF, ``coupled_cluster.CCD`` -- which reaches the same energy,
and the exact energy of the same basis (``StringCI``: all determinants)."""

import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch

import quantum_systems_amd as qs
from quantum_systems_amd import hip


def run(n, l, shells, omega):
    spatial = qs.SpatialOrbitalSystem(n, qs.TwoDimensionalHarmonicOscillator(l, 6.0, 61, omega=omega, np=hip))
    hf = qs.HartreeFock(spatial)
    C, epsilon, energies = hf.scf(tol=1e-10)
    print(f"{n} electrons in {l} orbitals ({shells} shells), omega = {omega}: RHF converged {hf.converged} "
          f"after {hf.iterations} iterations")
    print(f"  E_RHF   = {energies[-1]:.10f}")
    rccd = hf.ccd()
    e_mp2 = rccd.energy()
    e_rccd = rccd.solve(tol=1e-8, max_iter=200)
    print(f"  E_MP2   = {energies[-1] + e_mp2:.10f}   (correlation {e_mp2:.10f})")
    print(f"  E_RCCD  = {energies[-1] + e_rccd:.10f}   (correlation {e_rccd:.10f}; {type(rccd).__name__} converged "
          f"{rccd.converged} after {rccd.iterations} iterations, residual {rccd.residuals[-1]:.1e})")

    general = spatial.construct_general_orbital_system(anti_symmetrize=True)
    ghf = qs.HartreeFock(general)
    _, _, g_energies = ghf.scf(tol=1e-10)
    ccd = ghf.ccd()
    e_ccd = ccd.solve(tol=1e-8, max_iter=200)
    print(f"  E_CCD   = {g_energies[-1] + e_ccd:.10f}   (GHF {g_energies[-1]:.10f} + {type(ccd).__name__} on {general.l} "
          f"spin orbitals, correlation {e_ccd:.10f}; differs by {g_energies[-1] + e_ccd - energies[-1] - e_rccd:.1e})")

    exact = hf.string_ci()
    e, _ = exact.solve(1, tol=1e-9)
    e = float(torch.as_tensor(e).cpu()[0])
    print(f"  E_exact = {e:.10f}   (all determinants; RCCD leaves {energies[-1] + e_rccd - e:.2e})")


def main():
    shells = int(sys.argv[1]) if len(sys.argv) > 1 else 4
    omega = float(sys.argv[2]) if len(sys.argv) > 2 else 1.0
    l = shells * (shells + 1) // 2                       # 4 shells -> 10 orbitals
    for n in (2, 6):
        run(n, l, shells, omega)


if __name__ == "__main__":
    main()
