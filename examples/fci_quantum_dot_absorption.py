"""The dipole absorption spectrum and the polarizability of the exact ground state of a 2-D parabolic quantum dot:
restricted Hartree-Fock, spin-free string CI, and a Lanczos recurrence on H from (x - <x>)|Psi_0>.

    python examples/fci_quantum_dot_absorption.py [shells] [n_pairs] [n_steps] [omega]

``StringCI.apply_one_body`` applies the dipole operator as one gather through the replacement tables
(``kernels.string_ci_one_body``, no intermediate); ``StringCI.dipole_spectrum`` then runs ``response.lanczos`` on
``kernels.string_ci_sigma`` -- three vectors of memory, n_steps applications of H -- and returns per spatial dimension the
poles omega_j = E_j - E_0 and weights |<j|x|0>|^2 that reproduce the first 2 n_steps moments of the spectrum.  No excited
state is solved for.

In a parabolic confinement the dipole couples to the centre of mass alone, whose excitation energy is the confinement
frequency whatever the interaction (Kohn's theorem): the strongest line should lie at omega, and alpha(0) near N / omega^2.
The basis is finite, so both are printed, not asserted.  Default: 3 shells, 6 spatial orbitals, 2 + 2 electrons.
"""

import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch

import quantum_systems_amd as qs
from quantum_systems_amd import hip, kernels


def main():
    shells = int(sys.argv[1]) if len(sys.argv) > 1 else 3
    pairs = int(sys.argv[2]) if len(sys.argv) > 2 else 2
    steps = int(sys.argv[3]) if len(sys.argv) > 3 else 40
    omega = float(sys.argv[4]) if len(sys.argv) > 4 else 1.0
    l = shells * (shells + 1) // 2

    basis = qs.TwoDimensionalHarmonicOscillator(l, 6.0, 61, omega=omega, np=hip)
    system = qs.SpatialOrbitalSystem(2 * pairs, basis)
    hf = qs.HartreeFock(system)
    hf.scf(tol=1e-10, max_iter=200)
    print(f"{2 * pairs} electrons in {l} spatial orbitals ({shells} shells), omega = {omega}, RHF converged: {hf.converged} "
          f"after {hf.iterations} iterations")

    ci = hf.string_ci()
    E, _ = ci.solve(n_roots=1, tol=1e-10)
    print(f"  {ci.na} x {ci.nb} = {ci.dim} determinants, E_0 = {float(torch.as_tensor(E).cpu()[0]):.10f}, converged: {ci.converged}")

    spectra = ci.dipole_spectrum(0, n_steps=min(steps, ci.dim))
    ci.apply_one_body(system.dipole_moment, ci.c[0])
    print(f"  apply_one_body on the dipole operator ran [{kernels.last_dispatch()}]")
    for axis, S in zip("xyz", spectra):
        order = S.weights.argsort()[::-1][:5]
        f = S.oscillator_strengths()
        print(f"  dipole along {axis}: {len(S.poles)} poles, total weight {S.moment(0):.6f}, sum of oscillator strengths "
              f"{f.sum():.6f} (N = {2 * pairs} in a complete basis)")
        print("      omega_j       weight    oscillator strength")
        for j in sorted(order):
            print(f"    {S.poles[j]:10.6f}  {S.weights[j]:10.6f}  {f[j]:10.6f}")
        top = order[0]
        print(f"    strongest line at {S.poles[top]:.6f}: {S.poles[top] - omega:+.2e} from the confinement frequency, "
              f"{100 * f[top] / f.sum():.2f} % of the oscillator strength (Kohn's theorem: all of it at omega)")
    alpha0 = torch.as_tensor(ci.polarizability(0.0, n_steps=min(steps, ci.dim))).cpu().tolist()
    print(f"  static polarizability alpha_xx(0) per dimension: {', '.join(f'{a:.6f}' for a in alpha0)} "
          f"(N / omega^2 = {2 * pairs / omega ** 2:.6f} for the centre-of-mass mode alone)")


if __name__ == "__main__":
    main()
