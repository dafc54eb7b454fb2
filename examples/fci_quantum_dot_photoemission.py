"""Removing an electron from, and adding one to, the exact ground state of a 2-D parabolic quantum dot: restricted
Hartree-Fock, spin-free string CI, and Lanczos recurrences in the sectors with one electron less and one more.

    python examples/fci_quantum_dot_photoemission.py [shells] [n_pairs] [n_steps] [omega]

``StringCI.neighbour`` gives the ``StringCI`` of the neighbouring sector on the SAME transformed integrals;
``StringCI.annihilate`` / ``create`` carry a state there as one gather through a ladder table (``kernels.string_ci_ladder``,
no intermediate); ``removal_spectrum`` / ``addition_spectrum`` run ``response.lanczos`` on ``kernels.string_ci_sigma`` of that
sector from ``a(v)|Psi_0>`` and ``a+(v)|Psi_0>`` and return poles ``E_j(N -+ 1) - E_0(N)`` and weights -- the tunnelling
(photoemission and inverse photoemission) lines of the orbital ``v`` -- and ``green_function`` adds them up to the retarded
``G_vv(omega)``.  ``dyson_orbitals`` gives the amplitudes ``<Psi_j(N - 1)| a_p |Psi_0>`` against solved states of the ion.

Printed, not asserted: the first ionisation energy and the affinity from two ``solve()`` calls next to the lowest poles of the
two spectra, the pole strength of the first Dyson orbital, and the two sum rules ``sum_j w-_j = v^+ rho v`` and
``sum_j w+_j = v^+ (1 - rho) v``.  Default: 3 shells, 6 spatial orbitals, 2 + 2 electrons, v = the highest occupied
Hartree-Fock orbital for removal and the lowest empty one for addition.
"""

import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy
import torch

import quantum_systems_amd as qs
from quantum_systems_amd import hip, kernels


def host(x):
    return torch.as_tensor(x).cpu().numpy()


def lowest(S):
    """The lowest pole that carries weight, and that weight."""
    j = numpy.nonzero(S.weights > 1e-10 * S.weights.sum())[0][0]
    return S.poles[j], S.weights[j]


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
    E0 = float(host(E)[0])
    print(f"  N     : {ci.na} x {ci.nb} = {ci.dim} determinants, E_0 = {E0:.10f}, converged: {ci.converged}")
    ion, anion = ci.neighbour(d_up=-1), ci.neighbour(d_up=+1)
    Ei, _ = ion.solve(n_roots=min(4, ion.dim), tol=1e-10)
    Ea, _ = anion.solve(n_roots=1, tol=1e-10)
    Ei, Ea = host(Ei), host(Ea)
    print(f"  N - 1 : {ion.na} x {ion.nb} = {ion.dim} determinants, E_0 = {Ei[0]:.10f}; shares the transformed integrals: {ion._ut is ci._ut}")
    print(f"  N + 1 : {anion.na} x {anion.nb} = {anion.dim} determinants, E_0 = {Ea[0]:.10f}")

    homo, lumo = numpy.eye(l)[pairs - 1], numpy.eye(l)[pairs]
    Sm = ci.removal_spectrum(homo, n_steps=min(steps, ion.dim))
    Sp = ci.addition_spectrum(lumo, n_steps=min(steps, anion.dim))
    ci.annihilate(homo, ci.c[0])
    print(f"  annihilate ran [{kernels.last_dispatch()}]")
    pm, wm = lowest(Sm)
    pp, wp = lowest(Sp)
    print(f"  first ionisation energy E_0(N-1) - E_0(N) = {Ei[0] - E0:.8f}; lowest removal pole of the highest occupied orbital "
          f"{pm:.8f} with weight {wm:.6f}")
    print(f"  electron affinity       E_0(N) - E_0(N+1) = {E0 - Ea[0]:.8f}; minus the lowest addition pole of the lowest empty orbital "
          f"{-pp:.8f} with weight {wp:.6f}")
    print(f"  fundamental gap I - A = {(Ei[0] - E0) - (E0 - Ea[0]):.8f}; from the two spectra {pm + pp:.8f}")

    g, _ = ci.dyson_orbitals(ion)
    g = host(g)
    strength = (numpy.abs(g) ** 2).sum(axis=1)
    print("  Dyson orbitals against the solved states of N - 1: pole strengths " + ", ".join(f"{x:.6f}" for x in strength)
          + f"; the first one is {100 * abs(g[0, pairs - 1]) ** 2 / strength[0]:.2f} % the highest occupied orbital")

    rho_a, _ = (host(x) for x in ci.one_body_density_spin(0))
    for name, v, S, want in (("removal ", homo, Sm, numpy.einsum("p,q,qp->", homo, homo, rho_a).real),
                             ("addition", lumo, Sp, numpy.einsum("p,q,pq->", lumo, lumo, numpy.eye(l) - rho_a).real)):
        print(f"  sum rule, {name}: sum of the weights {S.moment(0):.12f}, from the up density {want:.12f}")

    grid = numpy.linspace(-pm - 1.0, pp + 1.0, 9)
    G = host(ci.green_function(grid, homo, eta=0.05, n_steps=min(steps, ion.dim, anion.dim)))
    print("  retarded G of the highest occupied orbital, eta = 0.05:")
    for w, z in zip(grid, G):
        print(f"    omega = {w:9.5f}   G = {z.real:12.6f} {z.imag:+12.6f} i   spectral density -Im G / pi = {-z.imag / numpy.pi:10.6f}")


if __name__ == "__main__":
    main()
