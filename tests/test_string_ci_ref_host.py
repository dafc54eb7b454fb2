"""Host checks of the spin-free string formulation before any kernel runs: the Knowles-Handy path built from the
oracle's dense ``E_pq`` equals the Jordan-Wigner Hamiltonian (which pins the phase between the two creator orders and the
definitions of ``k`` and ``W``), and the host helpers of ``quantum_systems_amd.string_ci`` -- ``full_strings``, the list
checks, ``determinant_order`` behind ``to_determinants`` -- agree with the oracle."""

import numpy as np
import pytest

import _det_ci_ref as dref
import _string_ci_ref as ref


@pytest.mark.parametrize("complex_", [False, True], ids=["real", "complex"])
@pytest.mark.parametrize("m,Na,Nb", ref.SHAPES)
def test_knowles_handy_path_is_the_jordan_wigner_hamiltonian(m, Na, Nb, complex_):
    ht, ut = ref.random_hamiltonian(m, 100 + 10 * m + 3 * Na + Nb, complex_)
    H = ref.dense_hamiltonian(ht, ut, Na, Nb)
    k, W = ref.kh_operands(ht, ut)
    Hkh = ref.kh_hamiltonian(k, W, ref.dense_E(m, Na, Nb))
    assert H.shape == Hkh.shape == (len(ref.strings(m, Na)) * len(ref.strings(m, Nb)),) * 2
    err, bound = np.abs(H - Hkh).max(), 1e-12 * np.linalg.norm(H)
    print(f"({m},{Na},{Nb}) {'c128' if complex_ else 'f64'}: |H_KH - H_JW| / bound = {err / bound:.3e}")
    assert err <= bound
    assert np.abs(H - H.conj().T).max() <= bound


@pytest.mark.parametrize("m,Na,Nb", ref.SHAPES)
def test_dense_E_is_the_sum_of_the_one_spin_operators(m, Na, Nb):
    """E_pq on the sector is E^alpha_pq x 1 + 1 x E^beta_pq with the ONE-spin operators of the ladder oracle: the
    determinant "all alpha first" lets E act on one string at a time with that string's own sign."""
    E = ref.dense_E(m, Na, Nb)
    Ea, Eb = ref.list_E(ref.strings(m, Na), m), ref.list_E(ref.strings(m, Nb), m)
    na, nb = Ea.shape[2], Eb.shape[2]
    want = np.einsum("pqij,ab->pqiajb", Ea, np.eye(nb)) + np.einsum("ij,pqab->pqiajb", np.eye(na), Eb)
    assert np.array_equal(E, want.reshape(m, m, na * nb, na * nb))


def test_full_strings_and_list_checks():
    from quantum_systems_amd.string_ci import checked_strings, full_strings

    for m, N in [(1, 0), (1, 1), (5, 0), (5, 2), (6, 6), (9, 4)]:
        assert np.array_equal(full_strings(m, N), ref.strings(m, N))
        assert full_strings(m, N).dtype == np.int64
    assert np.array_equal(full_strings(63, 0), [0])
    assert len(full_strings(63, 1)) == 63 and int(full_strings(63, 1)[-1]) == 1 << 62
    for bad in [(0, 0), (64, 1), (5, -1), (5, 6)]:
        with pytest.raises(ValueError):
            full_strings(*bad)
    assert np.array_equal(checked_strings(None, 5, 2), ref.strings(5, 2))
    assert np.array_equal(checked_strings([3, 5, 24], 5, 2), [3, 5, 24])
    assert np.array_equal(checked_strings(np.array([0], dtype=np.uint64), 5, 0), [0])
    for bad, N in [([5, 3], 2), ([3, 3], 2), ([3, 7], 2), ([3, 33], 2), ([], 2), ([[3]], 2), ([3.0], 2), ([-1], 2), ([0], 1)]:
        with pytest.raises(ValueError):
            checked_strings(np.array(bad), 5, N)


@pytest.mark.parametrize("m,Na,Nb", ref.SHAPES + [(5, 2, 3)])
def test_determinant_order_is_the_oracles_sector_map(m, Na, Nb):
    from quantum_systems_amd.string_ci import determinant_order

    masks, perm, phase = determinant_order(ref.strings(m, Na), ref.strings(m, Nb))
    sec = np.array([x for x in dref.sector(2 * m, Na + Nb) if dref.popcount(int(x) & 0x5555555555555555) == Na]) \
        if 2 * m <= 10 else None
    assert (np.diff(masks) > 0).all()
    if sec is not None:
        assert np.array_equal(masks, sec)
    # the oracle's position and sign of every (Ia, Ib)
    want_mask, want_phase = [], []
    for a in ref.strings(m, Na):
        for b in ref.strings(m, Nb):
            want_mask.append(ref._interleaved(int(a), int(b), m))
            want_phase.append(ref._parity(int(a), int(b), m))
    assert np.array_equal(masks, np.array(want_mask)[perm])
    assert np.array_equal(phase, want_phase)
    with pytest.raises(ValueError):
        determinant_order(np.array([1 << 31]), np.array([1]))


def test_to_determinants_carries_the_hamiltonian():
    """H in (Ia, Ib) order, taken through ``determinant_order``, is the Jordan-Wigner H on the interleaved sector."""
    from quantum_systems_amd.string_ci import determinant_order

    m, Na, Nb = 4, 2, 1
    ht, ut = ref.random_hamiltonian(m, 7, True)
    H = ref.dense_hamiltonian(ht, ut, Na, Nb)
    masks, perm, phase = determinant_order(ref.strings(m, Na), ref.strings(m, Nb))
    h2, u2 = ref.spin_orbital_inputs(ht, ut)
    full = dref.dense_hamiltonian(h2, u2, Na + Nb)
    sec = {int(x): i for i, x in enumerate(dref.sector(2 * m, Na + Nb))}
    idx = np.array([sec[int(x)] for x in masks])
    Hd = (H * phase[:, None] * phase[None, :])[np.ix_(perm, perm)]
    assert np.abs(Hd - full[np.ix_(idx, idx)]).max() <= 1e-12 * np.linalg.norm(H)
