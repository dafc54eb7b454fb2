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


# -- the helper of tests/test_gpu_triples_singles_scale.py


def set_sums(X, slots, A, G, sslots, eo3, ev, T, x=0):
    """``|singles contribution| / singles_bound`` of every tile set of triple ``x``."""
    terms = cs.singles_terms(X, slots[x], A, G, sslots[x], eo3[x], ev, extended=True)
    sums = np.abs(tr.tile_set_sums(terms, T)).astype(np.float64)
    return sums / cs.singles_bound(X, slots, A, G, sslots, eo3, ev)[x]


@pytest.mark.parametrize("v, T", [(5, 8), (8, 8), (10, 8), (13, 6), (19, 6), (20, 3)])
def test_singles_tile_set_sums_add_up_to_the_reference(v, T):
    X, slots, eo3, ev = tr.kernel_problem(v, 1, 6, 100 + v, complex_=T == 6)
    A, G, sslots = cs.singles_problem(v, 1, 7, 9, 200 + v, complex_=T == 6)
    terms = cs.singles_terms(X, slots[0], A, G, sslots[0], eo3[0], ev, extended=True)
    sums = tr.tile_set_sums(terms, T)
    nt = -(-v // T)
    assert sums.shape == (nt * (nt + 1) * (nt + 2) // 6,) and sums.dtype == np.longdouble
    wide = cs.singles_ref(X, slots, A, G, sslots, eo3, ev, extended=True)[0]
    assert abs(sums.sum() - wide) <= 1e-16 * np.abs(terms).sum()
    assert abs(wide) > 1e-3 * np.abs(terms).sum() / v                    # (not a sum that is 0 anyway)


def test_singles_sensitivity_leaves_out_what_vanishes_by_identity_only():
    T = 8
    for v, share, sshare in ((2 * T + 1, "none", "none"), (T + 2, "none", "none"), (T + 2, "pair", "repeat"),
                             (T + 2, "none", "repeat")):
        X, slots, eo3, ev = tr.kernel_problem(v, 1, 6, 100 + v, share=share)
        A, G, sslots = cs.singles_problem(v, 1, 7, 9, 200 + v, share=sshare)
        sums = set_sums(X, slots, A, G, sslots, eo3, ev, T)
        ratio = cs.singles_tile_set_sensitivity(X, slots, A, G, sslots, eo3, ev, T)
        print(f"v = {v}, {share}, {sshare}: set contributions / bound {sums}, sensitivity {ratio:.3e}")
        if v % T == 1:                                                   # the one-element ragged tile: a = b = c, Z = 0
            assert sums[-1] <= 1 and ratio == sums[:-1].min()
        else:
            assert ratio == sums.min()
        assert ratio >= 100
    # one block six times (Z = 0), and six equal (sa, sg) (V' totally symmetric): nothing to see in any set
    v = T + 2
    X, slots, eo3, ev = tr.kernel_problem(v, 2, 6, 3)
    A, G, sslots = cs.singles_problem(v, 2, 7, 9, 4)
    for blind_slots, blind_sslots in ((True, False), (False, True)):
        s, ss = slots.copy(), sslots.copy()
        if blind_slots:
            s[0] = 4
        if blind_sslots:
            ss[0] = (3, 5)
        assert (set_sums(X, s, A, G, ss, eo3, ev, T) <= 1).all()
        assert (set_sums(X, s, A, G, ss, eo3, ev, T, 1) >= 100).all()
        assert cs.singles_tile_set_sensitivity(X, s[:1], A, G, ss[:1], eo3[:1], ev, T) == np.inf
        assert 100 <= cs.singles_tile_set_sensitivity(X, s, A, G, ss, eo3, ev, T) < np.inf
    # six equal rows of A with different blocks of G, or the reverse, is no identity
    for column in (0, 1):
        ss = sslots.copy()
        ss[:, :, column] = 2
        assert 100 <= cs.singles_tile_set_sensitivity(X, slots, A, G, ss, eo3, ev, T) == min(
            set_sums(X, slots, A, G, ss, eo3, ev, T, x).min() for x in range(2))
    # cyclic tables: even orders one thing, odd orders another -- W (V') is totally symmetric where two indices are equal,
    # all that the diagonal set of a ragged tile of two holds; one element more in that tile and the set counts again
    cyclic = np.array([2, 5, 5, 2, 2, 5], dtype=np.int32)
    other = np.array([2, 5, 5, 2, 5, 2], dtype=np.int32)
    for v, blind in ((T + 2, True), (T + 3, False)):
        X, slots, eo3, ev = tr.kernel_problem(v, 2, 6, 100 + v)
        A, G, sslots = cs.singles_problem(v, 2, 7, 9, 200 + v)
        for which in ("slots", "sslots"):
            s, ss = slots.copy(), sslots.copy()
            if which == "slots":
                s[0], s[1] = cyclic, other
            else:
                ss[0], ss[1] = np.stack([cyclic, cyclic + 1], axis=1), np.stack([other, other + 1], axis=1)
            first, second = (set_sums(X, s, A, G, ss, eo3, ev, T, x) for x in range(2))
            print(f"v = {v}, cyclic {which}: {first}, not cyclic: {second}")
            assert (first[-1] <= 1) == blind and (first[:-1] >= 100).all() and (second >= 100).all()
            assert cs.singles_tile_set_sensitivity(X, s, A, G, ss, eo3, ev, T) >= 100
        # a cyclic column alone (the rows of A cyclic, the blocks of G all different) is no identity
        ss = sslots.copy()
        ss[0, :, 0] = cyclic
        assert 100 <= cs.singles_tile_set_sensitivity(X, slots, A, G, ss, eo3, ev, T) <= set_sums(X, slots, A, G, ss, eo3, ev, T)[-1]


@pytest.mark.parametrize("v, T, complex_", [(10, 8, False), (8, 6, True)])
def test_singles_sensitivity_of_every_slot_pattern(v, T, complex_):
    """The 203 coincidence patterns of ``slots`` at a ragged tile of two with six distinct ``(sa, sg)``: what is left out
    is below one bound (0 by identity), everything else 100 bounds at least."""
    X, _, eo3, ev = tr.kernel_problem(v, 203, 12, 300 + v, complex_=complex_)
    slots = tr.slot_partitions(12, seed=v)
    A, G, sslots = cs.singles_problem(v, 203, 12, 12, 400 + v, complex_=complex_)
    left_out = 0
    for x, row in enumerate(slots):
        sums = set_sums(X, slots, A, G, sslots, eo3, ev, T, x)
        small = sums < 100
        assert (sums[small] <= 1).all(), (tr.coincidence(row), sums)
        if small.any():
            left_out += 1
            assert tr.coincidence(row) in ((0,) * 6, (0, 1, 1, 0, 0, 1)), (tr.coincidence(row), sums)
            assert small.all() or (small == [False, False, False, True]).all()
    assert left_out == 2 and cs.singles_tile_set_sensitivity(X, slots, A, G, sslots, eo3, ev, T) >= 100


@pytest.mark.parametrize("v, T, complex_", [(10, 8, False), (8, 6, True)])
def test_singles_sensitivity_of_repeated_entries(v, T, complex_):
    """``sslots`` rows with repeated entries beside six distinct blocks and beside the table of their own triple: the
    "repeat" share, all six equal, and the physical rows of i = j and of j = k."""
    ns = 3
    rows = [cs.singles_problem(v, 1, ns, ns * ns, 5, share="repeat")[2][0], np.array([(1, 4)] * 6),
            np.array(cs.singles_slot_row(ns, 0, 0, 2)), np.array(cs.singles_slot_row(ns, 0, 2, 2)),
            np.array(cs.singles_slot_row(ns, 1, 1, 2)), np.array(cs.singles_slot_row(ns, 0, 1, 1))]
    sslots = np.array(rows + rows[2:], dtype=np.int32)
    n = len(sslots)
    X, slots, eo3, ev = tr.kernel_problem(v, n, ns ** 3, 500 + v, complex_=complex_)
    for x, ijk in enumerate(((0, 0, 2), (0, 2, 2), (1, 1, 2), (0, 1, 1))):
        slots[6 + x] = tr.slot_row(ns, *ijk)                             # the physical pair: both tables of one triple
        assert tr.coincidence(slots[6 + x]) == tr.coincidence(sslots[6 + x] @ [ns * ns, 1])
    A, G, _ = cs.singles_problem(v, 1, ns, ns * ns, 600 + v, complex_=complex_, share="repeat")
    for x in range(n):
        sums = set_sums(X, slots, A, G, sslots, eo3, ev, T, x)
        print(f"row {x}: set contributions / bound {sums}")
        if x == 1:
            assert (sums <= 1).all()                                     # all six equal: 1e-11 of a bound and less
        else:
            assert (sums >= 100).all()
    assert 100 <= cs.singles_tile_set_sensitivity(X, slots, A, G, sslots, eo3, ev, T) < np.inf
    assert cs.singles_tile_set_sensitivity(X, slots[1:2], A, G, sslots[1:2], eo3[1:2], ev, T) == np.inf


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
