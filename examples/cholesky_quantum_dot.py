"""Cholesky vectors of the two-body integrals of a 2-D quantum dot on one MI355X.

    python examples/cholesky_quantum_dot.py [shells] [n]

Decomposes the Coulomb tensor of the Fock-Darwin basis (``cholesky.decompose``: a pivoted Cholesky decomposition of
G[(r,p),(q,s)] = u[p,q,r,s], read from ``u`` in place) and prints the rank against l^2 -- for R closed shells it is
(2R - 1) 2R / 2, about 4 l, exact to rounding.  Then runs restricted Hartree-Fock twice, on ``u`` (one pass over the
tensor per iteration) and on the vectors (a few products on about 4 l matrices), and takes the MP2 energy from the
block <ij|ab> of the vectors in the Hartree-Fock orbitals (``transform`` + ``block``) next to ``hf.mp2()`` on ``u``.
"""

import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch

import quantum_systems_amd as qs
from quantum_systems_amd import hip


def main():
    shells = int(sys.argv[1]) if len(sys.argv) > 1 else 7
    n = int(sys.argv[2]) if len(sys.argv) > 2 else 6
    l = shells * (shells + 1) // 2                       # 7 shells -> 28 orbitals

    basis = qs.TwoDimensionalHarmonicOscillator(l, 6.0, 61, omega=1.0, np=hip)
    system = qs.SpatialOrbitalSystem(n, basis)
    u = torch.as_tensor(system.u)
    tol = 1e-8 * float(u.abs().max())         # (above the error of the generated elements: DESIGN.md section 7)

    chol = system.cholesky_two_body(tol)
    err = float((chol.reconstruct() - u).abs().max())
    print(f"{l} orbitals ({shells} shells): rank {chol.rank} of l^2 = {l * l} ((2R - 1) 2R / 2 = {(2 * shells - 1) * shells}), "
          f"converged {chol.converged}")
    print(f"  residual diagonal: largest {chol.residual[0]:.2e}, smallest {chol.residual[1]:.2e} (tol {tol:.2e}); "
          f"max |u - reconstruct()| = {err:.2e}")
    print(f"  storage: {chol.L.numel() * 8 / 1e6:.3f} MB of vectors for {u.numel() * 8 / 1e6:.3f} MB of u")

    on_u = qs.HartreeFock(system)
    C, epsilon, e_u = on_u.scf(tol=1e-10)
    on_vectors = qs.HartreeFock(system, two_body=chol)
    _, _, e_v = on_vectors.scf(tol=1e-10)
    print(f"RHF, {n} electrons: on u {e_u[-1]:.10f} ({on_u.iterations} iterations), on the vectors {e_v[-1]:.10f} "
          f"({on_vectors.iterations} iterations), largest difference per iteration "
          f"{max(abs(a - b) for a, b in zip(e_u, e_v)):.2e}")

    # MP2 from the vectors: <ij|ab> in the canonical orbitals is one block of the transformed vectors
    o, v = slice(0, system.n), slice(system.n, l)
    g = chol.transform(C).block(o, o, v, v)
    eps = torch.as_tensor(epsilon).real.to(torch.float64)
    D = eps[o, None, None, None] + eps[None, o, None, None] - eps[None, None, v, None] - eps[None, None, None, v]
    e2 = float((g * (2.0 * g - g.transpose(0, 1)).conj() / D).sum().real)
    print(f"MP2: E2 from the vectors' block {e2:.10f}, from the block transform of u {on_u.mp2():.10f}")


if __name__ == "__main__":
    main()
