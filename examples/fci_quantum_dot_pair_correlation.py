"""Where the up and the down electrons of a polarised quantum-dot state are, and how they avoid one another: restricted
Hartree-Fock orbitals, spin-free string CI with n_up != n_down, and the spin-resolved densities of the ground state.

    python examples/fci_quantum_dot_pair_correlation.py [shells] [n_up] [n_down]

``StringCI.spin_density`` is rho_alpha - rho_beta, and ``StringCI.pair_density_matrix(phi0, spins=...)`` contracts a
spin block of the two-body density with the orbital values ``phi0`` at a reference point: through
``system.compute_particle_density`` it becomes the density of up electrons given an up electron ("aa") or a down electron
("ab") at that point.  The same-spin one vanishes at the reference point (the Fermi hole); the opposite-spin one is only
lowered there (the Coulomb hole).  All of it comes from ONE ``kernels.string_ci_density2_spin`` call per quantity: two Gram
products of panels that keep the alpha and the beta replacement apart.  Default: 3 shells, 6 spatial orbitals, 3 up and 1
down electron.
"""

import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch

import quantum_systems_amd as qs
from quantum_systems_amd import hip, kernels


def plain(x):
    return torch.as_tensor(x).as_subclass(torch.Tensor)


def main():
    shells = int(sys.argv[1]) if len(sys.argv) > 1 else 3
    n_up = int(sys.argv[2]) if len(sys.argv) > 2 else 3
    n_down = int(sys.argv[3]) if len(sys.argv) > 3 else 1
    l = shells * (shells + 1) // 2

    basis = qs.TwoDimensionalHarmonicOscillator(l, 6.0, 61, omega=1.0, np=hip)
    system = qs.SpatialOrbitalSystem(2 * ((n_up + n_down + 1) // 2), basis)
    hf = qs.HartreeFock(system)
    C, _, _ = hf.scf(tol=1e-10, max_iter=200)
    ci = hf.string_ci(n_up=n_up, n_down=n_down)
    E, _ = ci.solve(n_roots=1)
    print(f"{n_up} up and {n_down} down electrons in {l} spatial orbitals ({shells} shells): {ci.na} x {ci.nb} = {ci.dim} "
          f"determinants, E = {float(plain(E)[0]):.10f}, converged: {ci.converged}")
    print(f"  <S^2> = {ci.spin_squared(0):.8f}, from the opposite-spin pair density {ci.spin_squared_from_densities(0):.8f}")
    n_a, _, n_b, _ = ci.natural_spin_orbitals(0)
    print("  natural up occupations:   " + " ".join(f"{x:.6f}" for x in plain(n_a).cpu().tolist()))
    print("  natural down occupations: " + " ".join(f"{x:.6f}" for x in plain(n_b).cpu().tolist()))

    rho_a, rho_b = ci.one_body_density_spin(0)
    ran = kernels.last_dispatch()
    up = plain(system.compute_particle_density(rho_a, C=C)).real
    down = plain(system.compute_particle_density(rho_b, C=C)).real
    spin = plain(system.compute_particle_density(ci.spin_density(0), C=C)).real
    print(f"  spin density: largest |up - down - spin_density| on the grid {float((up - down - spin).abs().max()):.1e}, "
          f"largest spin density {float(spin.max()):.6f}")

    # the reference point: where the down density is largest; phi0[p] = psi_p(r0) = sum_a chi_a(r0) C[a, p]
    at = int(down.reshape(-1).argmax())
    spf = plain(system.spf)
    dt = torch.promote_types(spf.dtype, plain(C).dtype)
    phi0 = spf.reshape(l, -1)[:, at].to(dt) @ plain(C).to(dt)
    print(f"  reference point: grid index {at}, down density there {float(down.reshape(-1)[at]):.6f}, up density "
          f"{float(up.reshape(-1)[at]):.6f}")
    for spins, who in (("aa", "an up electron"), ("ab", "a down electron")):
        M = ci.pair_density_matrix(phi0, 0, spins=spins)
        cond = plain(system.compute_particle_density(M, C=C)).real.reshape(-1)
        ref = up.reshape(-1)[at] if spins == "aa" else down.reshape(-1)[at]
        print(f"  up density given {who} at the point: at the point {float(cond[at] / ref):+.6f}, largest "
              f"{float(cond.max() / ref):.6f} at grid index {int(cond.argmax())}   (uncorrelated: {float(up.reshape(-1)[at]):.6f} at "
              f"the point)")
    print(f"  one_body_density_spin ran [{ran}]")


if __name__ == "__main__":
    main()
