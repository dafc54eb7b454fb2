"""Hartree-Fock and second-order Moller-Plesset energy of a 2-D quantum dot on one MI355X.

    python examples/mp2_quantum_dot.py [shells] [n]

Runs the SCF driver, then ``hf.mp2()``: the occupied-occupied-virtual-virtual block <ij|ab> of the two-body tensor in
the canonical orbitals from ONE block transform (``kernels.transform_two_body_blocks``: the occupied rows are
contracted with the leading index first, one read of ``u``) instead of the full four-index transform, and times the
two routes to the block next to each other.
"""

import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch

import quantum_systems_amd as qs
from quantum_systems_amd import hip, kernels


def timed(fn, reps=5):
    fn()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / reps


def main():
    shells = int(sys.argv[1]) if len(sys.argv) > 1 else 8
    n = int(sys.argv[2]) if len(sys.argv) > 2 else 6
    l = shells * (shells + 1) // 2                       # 8 shells -> 36 orbitals

    basis = qs.TwoDimensionalHarmonicOscillator(l, 6.0, 61, omega=1.0, np=hip)
    system = qs.SpatialOrbitalSystem(n, basis)
    hf = qs.HartreeFock(system)
    C, epsilon, energies = hf.scf(tol=1e-10)
    e2 = hf.mp2()
    print(f"{n} electrons in {l} orbitals ({shells} shells), RHF converged: {hf.converged} after {hf.iterations} iterations")
    print(f"  E_HF  = {energies[-1]:.10f}")
    print(f"  E2    = {e2:.10f}")
    print(f"  E_MP2 = {energies[-1] + e2:.10f}")

    o = system.n
    u, C = torch.as_tensor(system.u), torch.as_tensor(C)
    bra, ket = kernels.default_bra(C)[:o].contiguous(), C[:, o:].contiguous()
    t_block = timed(lambda: kernels.transform_two_body_blocks(u, bra, bra, ket, ket))
    ran = kernels.last_dispatch()
    t_full = timed(lambda: kernels.transform_two_body(u, C)[:o, :o, o:, o:])
    print(f"<ij|ab>: block transform {t_block * 1e3:.1f} us ({ran}); full transform + slice {t_full * 1e3:.1f} us")


if __name__ == "__main__":
    main()
