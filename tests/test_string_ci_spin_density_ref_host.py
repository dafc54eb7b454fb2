"""The host oracle of tests/_string_ci_spin_density_ref.py against independent statements of the same quantities (no GPU):
the spin blocks of ``_det_ci_density_ref``'s Jordan-Wigner spin-orbital densities (spin orbital 2 p + sigma, alpha = 0),
the spin-summed oracle of ``_string_ci_density_ref``, the dense S^2 built from Jordan-Wigner matrices, the
Jordan-Wigner Hamiltonian of ``_string_ci_ref``, and the two trace rules."""

import numpy as np
import pytest

import _det_ci_density_ref as ddref
import _string_ci_density_ref as sref
import _string_ci_ref as ref
import _string_ci_spin_density_ref as spref

# slices of the spin-orbital density G[p,q,r,s] = <a+_p a+_q a_s a_r> that hold one spin block
SLICES = {"aa": (0, 0), "ab": (0, 1), "bb": (1, 1), "ba": (1, 0)}


def vectors(m, Na, Nb, cplx, seed):
    na, nb = len(ref.strings(m, Na)), len(ref.strings(m, Nb))
    rng = np.random.default_rng(seed)
    c = rng.standard_normal((2, na, nb))
    if cplx:
        c = c + 1j * rng.standard_normal((2, na, nb))
    return c[0] / np.linalg.norm(c[0]), c[1] / np.linalg.norm(c[1])


def block(G_so, st):
    a, b = SLICES[st]
    return G_so[a::2, b::2, a::2, b::2]


@pytest.mark.parametrize("cplx", [False, True])
@pytest.mark.parametrize("m,Na,Nb", ref.SHAPES)
def test_blocks_are_the_spin_blocks_of_the_spin_orbital_densities(m, Na, Nb, cplx):
    Ea, Eb = ref.list_E(ref.strings(m, Na), m), ref.list_E(ref.strings(m, Nb), m)
    bra, ket = vectors(m, Na, Nb, cplx, 17 * m + Na)
    pos, phase = ref.sector_map(m, Na, Nb)
    count = {"a": Na, "b": Nb}
    for b, k in ((bra, bra), (bra, ket)):
        G, (rho_a, rho_b) = spref.spin_gamma(Ea, Eb, b, k)
        rho_so, G_so = ddref.jw_densities(phase * b.reshape(-1), phase * k.reshape(-1), 2 * m, Na + Nb, keep=pos)
        for st in spref.BLOCKS:
            assert np.abs(G[st] - block(G_so, st)).max() <= 1e-15, st
        assert np.abs(spref.transposed(G["ab"]) - block(G_so, "ba")).max() <= 1e-15
        assert np.abs(rho_a - rho_so[0::2, 0::2]).max() <= 1e-15 and np.abs(rho_b - rho_so[1::2, 1::2]).max() <= 1e-15
        # the spin sum is the spin-summed oracle
        Gs, rhos = sref.dense_gamma((Ea, Eb), b, k)
        assert np.abs(spref.spin_sum(G) - Gs).max() <= 1e-15 and np.abs(rho_a + rho_b - rhos).max() <= 1e-15
        # the two trace rules
        overlap = np.vdot(b, k)
        rho = {"a": rho_a, "b": rho_b}
        for st in spref.BLOCKS:
            s, t = st
            same = 1 if s == t else 0
            assert abs(np.einsum("pqpq->", G[st]) - count[s] * (count[t] - same) * overlap) <= 1e-14, st
            assert np.abs(np.einsum("pqrq->pr", G[st]) - (count[t] - same) * rho[s].T).max() <= 1e-14, st
        # exchange antisymmetry of the equal-spin blocks
        for st in ("aa", "bb"):
            assert np.abs(G[st] + G[st].transpose(1, 0, 2, 3)).max() <= 1e-15
            assert np.abs(G[st] + G[st].transpose(0, 1, 3, 2)).max() <= 1e-15
    G, _ = spref.spin_gamma(Ea, Eb, bra, bra)
    for st in spref.BLOCKS:
        assert np.abs(G[st] - G[st].transpose(2, 3, 0, 1).conj()).max() <= 1e-15


@pytest.mark.parametrize("cplx", [False, True])
@pytest.mark.parametrize("m,Na,Nb", ref.SHAPES)
def test_spin_squared_read_off_the_opposite_spin_block(m, Na, Nb, cplx):
    Ea, Eb = ref.list_E(ref.strings(m, Na), m), ref.list_E(ref.strings(m, Nb), m)
    S = sref.dense_spin_squared(m, Na, Nb)
    bra, _ = vectors(m, Na, Nb, cplx, 3 * m + Nb)
    G, _ = spref.spin_gamma(Ea, Eb, bra, bra)
    v = ref._wide(bra).reshape(-1)
    want = v.conj() @ (ref._wide(S) @ v)
    assert abs(spref.spin_squared(G, Na, Nb) - want) <= 1e-14


@pytest.mark.parametrize("cplx", [False, True])
@pytest.mark.parametrize("m,Na,Nb", ref.SHAPES)
def test_energy_from_the_spin_blocks_is_the_rayleigh_quotient(m, Na, Nb, cplx):
    ht, ut = ref.random_hamiltonian(m, 9 + m + Na, cplx)
    Hx = ref.dense_hamiltonian(ht, ut, Na, Nb, extended=True)
    Ea, Eb = ref.list_E(ref.strings(m, Na), m), ref.list_E(ref.strings(m, Nb), m)
    bra, ket = vectors(m, Na, Nb, cplx, 6)
    for b, k in ((bra, bra), (bra, ket)):
        G, rho = spref.spin_gamma(Ea, Eb, b, k)
        want = ref._wide(b).reshape(-1).conj() @ (Hx @ ref._wide(k).reshape(-1))
        assert abs(spref.energy(ht, ut, G, rho) - want) <= 1e-13 * max(1.0, float(np.abs(Hx).max()))
