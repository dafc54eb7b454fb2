"""The NumPy reference of tests/_ccsd_ref.py against its own definitions, on the CPU: the T1-dressed working form of CCSD
equals ``<mu| e^{-T} H e^{T} |0>`` by Fock-space matrices, (T) with singles in the working form with ``Y`` equals the
determinant sum with ``B_mu``, and CCSD for two electrons is exact."""

import numpy as np
import pytest

import _ccsd_ref as cs
import _rccd_ref as rc
import _triples_ref as tr


def amplitudes(seed, nv, ns, complex_, scale=0.1):
    rng = np.random.default_rng(seed)
    t2 = rc.closed_shell_amplitudes(rng, nv, ns, complex_=complex_, scale=scale)
    t1 = scale * rng.standard_normal((nv, ns))
    if complex_:
        t1 = t1 + 1j * scale * rng.standard_normal((nv, ns))
    return t1, t2


@pytest.mark.parametrize("complex_", [False, True], ids=["real", "complex"])
def test_working_forms_equal_the_projections(complex_):
    l, ns = 4, 2
    h, u, _ = rc.closed_shell_problem(l, 11, complex_=complex_, scale=0.2)
    t1, t2 = amplitudes(12, l - ns, ns, complex_, scale=0.3)
    E, R1, R2 = cs.projections(h, u, ns, t1, t2)
    W1, W2 = cs.residuals(h, u, ns, t1, t2)
    Ew = cs.total_energy(h, u, ns, t1, t2)
    Ec = cs.conventional_energy(h, u, ns, t1, t2)
    for name, got, want in (("R1", W1, R1), ("R2", W2, R2), ("E dressed", Ew, E), ("E conventional", Ec, E)):
        err = float(np.abs(np.asarray(got) - np.asarray(want)).max() / np.abs(np.asarray(want)).max())
        print(f"{name}: relative deviation {err:.3e}")
        assert err <= 1e-12, name
    assert np.abs(R1).max() > 1e-2 and np.abs(R2).max() > 1e-2
    if complex_:
        assert np.abs(np.imag(R1)).max() > 1e-3                              # conjugating t1 anywhere would show
    # the dressing keeps the particle-exchange symmetry and gives up hermiticity
    _, ud, _ = cs.dressed(h, u, ns, t1)
    assert np.abs(ud - ud.transpose(1, 0, 3, 2)).max() <= 1e-14 * np.abs(ud).max()
    assert np.abs(ud - ud.conj().transpose(2, 3, 0, 1)).max() > 1e-3


@pytest.mark.parametrize("l, ns", [(5, 2), (5, 3)])
def test_triples_with_singles_equal_the_determinant_sum(l, ns):
    h, u, eps = tr.canonical_problem(l, ns, 20 + ns, complex_=True, scale=0.1)
    t1, t2 = amplitudes(30 + ns, l - ns, ns, True)
    connected, singles = cs.pt_definition(h, u, eps, ns, t1, t2)
    wc, ws = cs.pt_working(u, eps, ns, t1, t2)
    print(f"l = {l}, o = {ns}: E_[T] {connected:.15e} / {wc:.15e}, E_ST {singles:.15e} / {ws:.15e}")
    assert abs(wc - connected) <= 1e-12 * abs(connected)
    assert abs(ws - singles) <= 1e-12 * abs(singles)
    assert abs(singles) > 1e-6                                               # (the random signs cancel most of it)
    assert abs(connected - tr.definition(h, u, eps, ns, t2)) <= 1e-12 * abs(connected)
    # the kernel's own sum on the packed blocks and the factors of RCCSD.triples is the working form
    X = tr.packed_blocks(tr.blocks(u, ns, t2))
    A, G = cs.singles_factors(u, ns, t1)
    todo = tr.triples(ns)
    slots = np.array([tr.slot_row(ns, *ijk) for ijk in todo])
    sslots = np.array([cs.singles_slot_row(ns, *ijk) for ijk in todo])
    eo3 = np.array([eps[i] + eps[j] + eps[k] for i, j, k in todo])
    es = cs.singles_ref(X, slots, A, G, sslots, eo3, eps[ns:])
    assert abs(sum(tr.weight(*ijk) * e for ijk, e in zip(todo, es)) - ws) <= 1e-12 * abs(ws)
    bound = cs.singles_bound(X, slots, A, G, sslots, eo3, eps[ns:])
    wide = cs.singles_ref(X, slots, A, G, sslots, eo3, eps[ns:], extended=True)
    assert (bound > 0).all() and (np.abs(es - wide) <= bound).all()


@pytest.mark.parametrize("complex_", [False, True], ids=["real", "complex"])
def test_two_electrons_are_exact(complex_):
    l, ns = 4, 1
    h, u, _ = rc.closed_shell_problem(l, 7, complex_=complex_, scale=0.1)
    e_corr, t1, t2, its = cs.solve(h, u, ns, tol=1e-13)
    exact = cs.two_electron_ground_state(h, u)
    e_ref = float(np.real(cs.reference_energy(h, u, ns)))
    print(f"E_ref {e_ref:.12f} + E_CCSD {e_corr:.12f} = {e_ref + e_corr:.12f}, exact {exact:.12f} ({its} iterations)")
    assert abs(e_ref + e_corr - exact) <= 1e-11
    assert np.abs(t1).max() > 1e-3                                           # not Hartree-Fock orbitals: singles matter
    # CCD on the same problem is not exact
    e_ccd, _, _ = rc.solve(h, u, np.eye(l), ns, tol=1e-13)
    assert abs(e_ref + e_ccd - exact) > 1e-6
