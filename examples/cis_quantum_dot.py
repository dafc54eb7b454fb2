"""Lowest excited states of a 2-D quantum dot on one MI355X: RHF, then configuration interaction singles.

    python examples/cis_quantum_dot.py [shells] [n] [roots]

Runs the SCF driver, then ``hf.cis()``: a block Davidson iteration whose sigma vectors are mean-field contractions of
the two-body tensor with transition densities.  All trial vectors of a step go through ``kernels.mean_field_batch``
together -- one read of ``u`` per group of them -- and the same solve is timed with the vectors sent one by one.
``n`` is the number of doubly occupied orbitals.
"""

import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch

import quantum_systems_amd as qs
from quantum_systems_amd import hip, kernels


def launches(entry):
    """Streaming launches in one dispatch-log entry (repeats of a kernel name are logged as ``name xN``)."""
    total = 0
    for part in entry.split(";"):
        if "qs::mean_field_batch_kernel<" in part:
            tail = part.strip().rsplit(" x", 1)
            total += int(tail[1]) if len(tail) == 2 and tail[1].isdigit() else 1
    return total


def solve(hf, roots, spin, batched):
    cis = hf.cis(batched=batched)
    kernels.dispatch_log = []
    try:
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        omega, _ = cis.solve(roots, tol=1e-8, spin=spin)
        torch.cuda.synchronize()
        wall = time.perf_counter() - t0
        passes = sum(launches(entry) for entry in kernels.dispatch_log)
    finally:
        kernels.dispatch_log = None
    return cis, torch.as_tensor(omega).cpu().numpy(), wall, passes


def main():
    shells = int(sys.argv[1]) if len(sys.argv) > 1 else 10
    n = int(sys.argv[2]) if len(sys.argv) > 2 else 3
    roots = int(sys.argv[3]) if len(sys.argv) > 3 else 6
    l = shells * (shells + 1) // 2                       # 10 shells -> 55 orbitals

    basis = qs.TwoDimensionalHarmonicOscillator(l, 6.0, 61, omega=1.0, np=hip)
    system = qs.SpatialOrbitalSystem(2 * n, basis)
    hf = qs.HartreeFock(system)
    _, _, energies = hf.scf(tol=1e-10)
    print(f"{2 * n} electrons in {l} orbitals ({shells} shells), RHF converged: {hf.converged} after {hf.iterations} "
          f"iterations, E_HF = {energies[-1]:.10f}")
    solve(hf, roots, "singlet", True)                    # warm-up (workspace, code objects)
    for spin in ("singlet", "triplet"):
        cis, omega, wall, passes = solve(hf, roots, spin, True)
        _, omega_1, wall_1, passes_1 = solve(hf, roots, spin, False)
        print(f"{spin}s: {omega}")
        print(f"  converged {cis.converged} after {cis.iterations} iterations, {sum(cis.sigma_history)} sigma vectors "
              f"(per step {cis.sigma_history})")
        print(f"  batched: {wall * 1e3:8.2f} ms, {passes} passes over u;  one by one: {wall_1 * 1e3:8.2f} ms, {passes_1} "
              f"passes;  max |difference| {abs(omega - omega_1).max():.1e}")
        if spin == "singlet":
            mu = torch.as_tensor(cis.transition_dipole_moments()).abs().cpu().numpy()
            print("  |transition dipole| (x, y):", mu.round(6).tolist())


if __name__ == "__main__":
    main()
