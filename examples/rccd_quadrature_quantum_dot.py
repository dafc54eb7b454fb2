"""Closed-shell coupled-cluster doubles for 6 electrons in the real 12-shell quantum dot (78 orbitals) on one MI355X.

    python examples/rccd_quadrature_quantum_dot.py [shells] [omega]

The Coulomb elements come from the quadrature generator (``coulomb="quadrature"``), which is exact at
every shell; the closed form of the reference loses digits from about 9 shells on.  The tensor has particle-exchange
symmetry bit for bit, so ``HartreeFock.ccd()`` -- ``coupled_cluster.RCCD`` for a ``SpatialOrbitalSystem`` -- takes its
ladder from half of ``u`` without a second look.  Beside the energies: the largest difference to the closed-form
tensor of the same dot, which is the closed form's error."""

import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch

import quantum_systems_amd as qs
from quantum_systems_amd import hip, kernels, two_dim_ho


def main():
    shells = int(sys.argv[1]) if len(sys.argv) > 1 else 12
    omega = float(sys.argv[2]) if len(sys.argv) > 2 else 1.0
    n, l = 6, shells * (shells + 1) // 2                 # 12 shells -> 78 orbitals

    t0 = time.time()
    dot = qs.TwoDimensionalHarmonicOscillator(l, 6.0, 61, omega=omega, coulomb="quadrature", np=hip)
    torch.cuda.synchronize()
    print(f"{n} electrons in {l} orbitals ({shells} shells), omega = {omega}: basis with quadrature u in {time.time() - t0:.2f} s, "
          f"exchange-symmetric bit for bit: {kernels.two_body_exchange_symmetric(dot.u)}")

    hf = qs.HartreeFock(qs.SpatialOrbitalSystem(n, dot))
    _, _, energies = hf.scf(tol=1e-10)
    print(f"  E_RHF   = {energies[-1]:.10f}   (converged {hf.converged} after {hf.iterations} iterations)")
    rccd = hf.ccd()
    e_mp2 = rccd.energy()
    e_rccd = rccd.solve(tol=1e-8, max_iter=200)
    print(f"  E_MP2   = {energies[-1] + e_mp2:.10f}   (correlation {e_mp2:.10f})")
    print(f"  E_RCCD  = {energies[-1] + e_rccd:.10f}   (correlation {e_rccd:.10f}; converged {rccd.converged} after "
          f"{rccd.iterations} iterations, residual {rccd.residuals[-1]:.1e})")

    t0 = time.time()
    quadrature = two_dim_ho.get_coulomb_elements(l, method="quadrature")
    torch.cuda.synchronize()
    t_quad = time.time() - t0
    t0 = time.time()
    closed = two_dim_ho.get_coulomb_elements(l)
    torch.cuda.synchronize()
    t_closed = time.time() - t0
    print(f"  largest |closed form - quadrature| over all {l}^4 elements: {float((closed - quadrature).abs().max()):.2e}   "
          f"(generated in {t_closed:.2f} s and {t_quad:.4f} s)")


if __name__ == "__main__":
    main()
