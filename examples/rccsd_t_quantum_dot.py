"""Closed-shell CCSD(T) for a 2-D quantum dot on one MI355X: singles make the method independent of Hartree-Fock
orbitals and exact for two electrons; (T) adds the perturbative triples with their singles term.

    python examples/rccsd_t_quantum_dot.py [shells] [omega]

1. Two electrons in the dot's OWN oscillator basis (no Hartree-Fock, ``C=None``): ``coupled_cluster.RCCD`` misses the
   exact energy by the orbital relaxation it cannot describe, ``coupled_cluster.RCCSD`` reproduces ``TwoParticleCI``.
2. Six electrons: RHF -> ``HartreeFock.ccsd()`` -> ``solve()`` -> ``triples()``: E_(T) = E_[T] + E_ST from ONE read of the
   blocks by ``kernels.triples_energy_singles``, beside RCCD, RCCD+T and the exact energy of the basis (``StringCI``)."""

import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch

import quantum_systems_amd as qs
from quantum_systems_amd import hip


def number(x):
    return float(torch.as_tensor(x).real.cpu().reshape(-1)[0])


def own_basis(l, shells, omega):
    spatial = qs.SpatialOrbitalSystem(2, qs.TwoDimensionalHarmonicOscillator(l, 6.0, 61, omega=omega, np=hip))
    e_ref = number(spatial.compute_reference_energy())
    rccd, rccsd = qs.RCCD(spatial), qs.RCCSD(spatial)
    e_d = rccd.solve(tol=1e-9, max_iter=300)
    e_sd = rccsd.solve(tol=1e-9, max_iter=300)
    exact, _ = qs.TwoParticleCI(spatial).solve(1, tol=1e-10)
    exact = number(exact)
    print(f"2 electrons in {l} oscillator orbitals ({shells} shells), omega = {omega}, no Hartree-Fock step:")
    print(f"  E_ref      = {e_ref:.10f}   (both electrons in the lowest oscillator orbital)")
    print(f"  E_RCCD     = {e_ref + e_d:.10f}   (converged {rccd.converged} after {rccd.iterations} iterations; off the "
          f"exact energy by {e_ref + e_d - exact:+.2e})")
    print(f"  E_RCCSD    = {e_ref + e_sd:.10f}   (converged {rccsd.converged} after {rccsd.iterations} iterations; off the "
          f"exact energy by {e_ref + e_sd - exact:+.2e}; largest |t1| {number(torch.as_tensor(rccsd.t1).abs().max()):.3f})")
    print(f"  E_exact    = {exact:.10f}   (TwoParticleCI)")


def hartree_fock_basis(n, l, shells, omega):
    spatial = qs.SpatialOrbitalSystem(n, qs.TwoDimensionalHarmonicOscillator(l, 6.0, 61, omega=omega, np=hip))
    hf = qs.HartreeFock(spatial)
    _, _, energies = hf.scf(tol=1e-10)
    e_hf = energies[-1]
    print(f"{n} electrons in {l} orbitals ({shells} shells), omega = {omega}: RHF converged {hf.converged} after "
          f"{hf.iterations} iterations")
    rccd = hf.ccd()
    e_d = rccd.solve(tol=1e-8, max_iter=200)
    e_dt = rccd.triples()
    rccsd = hf.ccsd()
    e_sd = rccsd.solve(tol=1e-8, max_iter=200)
    e_t = rccsd.triples()
    connected, singles = rccsd.triples_parts
    e, _ = hf.string_ci().solve(1, tol=1e-9)
    e = number(e)
    print(f"  E_RHF      = {e_hf:.10f}")
    print(f"  E_RCCD     = {e_hf + e_d:.10f}   (off the exact energy by {e_hf + e_d - e:+.2e})")
    print(f"  E_RCCD+T   = {e_hf + e_d + e_dt:.10f}   (off the exact energy by {e_hf + e_d + e_dt - e:+.2e})")
    print(f"  E_RCCSD    = {e_hf + e_sd:.10f}   (converged {rccsd.converged} after {rccsd.iterations} iterations; off the "
          f"exact energy by {e_hf + e_sd - e:+.2e})")
    print(f"  E_RCCSD(T) = {e_hf + e_sd + e_t:.10f}   (E_[T] {connected:.10f}, E_ST {singles:+.3e}, "
          f"{len(rccsd.triples_passes)} pass(es); off the exact energy by {e_hf + e_sd + e_t - e:+.2e})")
    print(f"  E_exact    = {e:.10f}   (all determinants)")


def main():
    shells = int(sys.argv[1]) if len(sys.argv) > 1 else 4
    omega = float(sys.argv[2]) if len(sys.argv) > 2 else 1.0
    l = shells * (shells + 1) // 2                       # 4 shells -> 10 orbitals
    own_basis(l, shells, omega)
    hartree_fock_basis(6, l, shells, omega)


if __name__ == "__main__":
    main()
