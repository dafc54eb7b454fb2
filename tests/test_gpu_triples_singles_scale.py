"""``kernels.triples_energy_singles`` where tests/test_gpu_triples_singles.py cannot see, after the pattern of
tests/test_gpu_triples_scale.py: more than three tiles along an index, a closing sum of more than 256 singles partials
behind a split of the workspace at ``n * nsets`` in the hundreds, ragged tiles of more than one element, every
coincidence of the six slots beside the singles gather, rows of ``A`` and blocks of ``G`` past 2^31 elements, and
``RCCSD.triples`` at more than one tile.

What the sizes are for (T = ``kernels.triples_tile``: 8 for fp64, 6 for complex128): as in
tests/test_gpu_triples_scale.py -- 3T, 3T + 2, 4T - 1, and 10T + 2 with nt = 11 and 286 tile sets, where both closes
take a second trip of their strided loop; T + 2 for everything about slots and addresses.  Never a ragged tile of ONE
element: its diagonal set holds a = b = c alone, Z = 0, and BOTH partials of that workgroup are 0 by identity.
``tile_set_sensitivity`` and ``singles_tile_set_sensitivity``, from the references alone and before the device result
is looked at, assert that every other tile set of every triple adds 100 ``kernel_bound`` to ``e`` and 100
``singles_bound`` to ``es`` at least, but for what is 0 by identity (one block in all six slots, cyclic slots on the
diagonal set of a ragged tile of two, six equal ``(sa, sg)``: tests/test_ccsd_ref_host.py shows that nothing else is
left out).

Tolerances: ``kernel_bound`` and ``singles_bound`` against the long-double evaluations, and the end-to-end rule of
tests/test_gpu_rccsd.py; nothing else.  Equal bits are asserted as equal bits.

Observed on an MI355X, largest deviation / bound over the triples of a case, ``e`` then ``es`` (fp64; complex128):
3T 8.9e-6, 1.6e-7; 4.1e-6, 1.9e-7.  3T + 2 5.4e-6, 1.1e-7; 2.3e-6, 3.4e-7.  4T - 1 1.2e-6, 8.8e-8; 2.6e-6, 8.1e-8.  10T + 2
1.4e-8, 1.3e-9; 8.1e-8, 9.7e-11.  The 203 slot patterns at T + 2 1.8e-4, 3.7e-5; 6.4e-5, 1.1e-5.  The nine packed rows and
blocks of the far-offset test 8.4e-5, 1.2e-5.  The least tile-set contribution to ``es`` in ``singles_bound``: 3.9e2 and
1.6e2 at 10T + 2, 1.5e5 and more elsewhere (to ``e`` in ``kernel_bound``: 4.0e3 and 5.6e3 at 10T + 2, 1.4e6 and more
elsewhere).  ``RCCSD.triples``, |device - long double| of the tolerance, E_[T] then E_ST: v = 10 real 0 of 3.4e-15, 8.5e-22
of 1.2e-16; v = 8 complex 8.7e-19 of 1.8e-14, 1.7e-21 of 1.0e-15; v = 19 real 2.2e-19 of 2.1e-14, 1.7e-21 of 6.7e-16; the
passes under a small budget gave the bits of the one launch.  Every test of this file takes 1 s or less.

What the file sees, each tried once on a kernel changed for the purpose: a second close that reads the connected
partials fails every test here; a close that takes one trip fails 10T + 2 alone, in ``e`` and in ``es``; a kernel whose
last diagonal tile set stores 0 for its singles partial passes tests/test_gpu_triples_singles.py and fails every test
here; ``G`` read transposed where the three tile indices differ fails every size with three tiles or more, the v = 19
``RCCSD.triples`` included."""

import numpy as np
import pytest
import torch

import _ccsd_ref as cs
import _triples_ref as tr
from test_gpu_rccsd import TOL, spatial_system, triples_reference
from test_gpu_triples_scale import NAMES, tile
from test_gpu_triples_singles import DTYPES, H, dev, mixed_problem, run

pytestmark = pytest.mark.gpu


def check_against_reference(name, X, slots, eo3, ev, A, G, sslots, label):
    """The sensitivity of the inputs, then the assertions of ``test_kernel_against_reference``; returns the device's
    ``(e, es)``."""
    from quantum_systems_amd import kernels

    T = tile(name)
    wide = tr.kernel_ref(X, slots, eo3, ev, extended=True)
    bound = tr.kernel_bound(X, slots, eo3, ev)
    wide_s = cs.singles_ref(X, slots, A, G, sslots, eo3, ev, extended=True)
    bound_s = cs.singles_bound(X, slots, A, G, sslots, eo3, ev)
    least = tr.tile_set_sensitivity(X, slots, eo3, ev, T)
    least_s = cs.singles_tile_set_sensitivity(X, slots, A, G, sslots, eo3, ev, T)
    print(f"{name} {label}: the least tile set adds {least:.3e} bounds to e and {least_s:.3e} bounds to es")
    assert len(ev) % T != 1 and least >= 100 and least_s >= 100         # conditions on the inputs: every workgroup counts
    e, es = run(X, slots, eo3, ev, A, G, sslots)
    log = kernels.last_dispatch()
    # the whole record: one energy launch, then the close twice (the record's run-length form), no plain kernel
    assert log == f"qs::triples_energy_singles_kernel<{1 if name == 'f64' else 2}>;qs::triples_close_kernel x2"
    err = np.abs(e - wide).astype(np.float64)
    err_s = np.abs(es - wide_s).astype(np.float64)
    print(f"{name} {label}: e = {e[:4]}, es = {es[:4]}, largest deviation / bound = {(err / bound).max():.3e} and "
          f"{(err_s / bound_s).max():.3e}")
    assert np.isfinite(e).all() and np.isfinite(es).all()
    assert (err <= bound).all() and (err_s <= bound_s).all()
    alone = H(kernels.triples_energy(dev(X), dev(slots), dev(eo3), dev(ev)))
    assert e.tobytes() == alone.tobytes()                               # the connected part: the bits of triples_energy
    e2, es2 = run(X, slots, eo3, ev, A, G, sslots)
    assert e.tobytes() == e2.tobytes() and es.tobytes() == es2.tobytes()        # the same bits on a second run
    return e, es


# -- more tile sets


def many_sets_problem(name, index):
    T = tile(name)
    v = [3 * T, 3 * T + 2, 4 * T - 1, 10 * T + 2][index]
    complex_ = name == "c128"
    if index < 3:
        return (v,) + mixed_problem(v, complex_, 500 + v)
    # nt = 11, two triples: six distinct blocks with six distinct (sa, sg); the tables of a triple with i = j.  (The seeds:
    # of a dozen tried on the references alone, before any device run, the pair whose least singles set is largest in
    # both types -- 3.9e2 and 1.6e2 bounds; most draws are between 20 and 300 at this size.)
    X, slots, eo3, ev = tr.kernel_problem(v, 2, 7, 505 + v, complex_=complex_)
    slots[0], slots[1] = [3, 0, 5, 1, 6, 2], [4, 2, 4, 2, 0, 0]
    A, G, sslots = cs.singles_problem(v, 2, 7, 9, 506 + v, complex_=complex_)
    sslots[1] = cs.singles_slot_row(3, 1, 1, 2)
    return v, X, slots, eo3, ev, A, G, sslots


@pytest.mark.parametrize("index", range(4))
@pytest.mark.parametrize("name", NAMES)
def test_more_tile_sets(name, index):
    from quantum_systems_amd import _lib, kernels

    v, X, slots, eo3, ev, A, G, sslots = many_sets_problem(name, index)
    nt = -(-v // tile(name))
    nsets = nt * (nt + 1) * (nt + 2) // 6
    assert nt == [3, 4, 4, 11][index] and (nsets > 256) == (index == 3)
    n = len(slots)
    assert n == (4 if index < 3 else 2)
    assert _lib.load().qs_triples_energy_singles_workspace(kernels.dtype_code(DTYPES[name]), v, n) == 16 * n * nsets
    check_against_reference(name, X, slots, eo3, ev, A, G, sslots, f"v = {v}, {nt} tiles")


# -- every coincidence of the six slots, beside the singles gather


def partition_problem(name):
    """203 triples on a dozen blocks at v = T + 2, one per coincidence pattern of ``slots``, six distinct ``(sa, sg)``
    each (the inputs of tests/test_ccsd_ref_host.py::test_singles_sensitivity_of_every_slot_pattern)."""
    v = tile(name) + 2
    X, _, eo3, ev = tr.kernel_problem(v, 203, 12, 300 + v, complex_=name == "c128")
    A, G, sslots = cs.singles_problem(v, 203, 12, 12, 400 + v, complex_=name == "c128")
    return X, tr.slot_partitions(12, seed=v), eo3, ev, A, G, sslots


def differing(first, second, slots):
    e, es = first
    f, fs = second
    rows = np.flatnonzero((e.view(np.uint64) != f.view(np.uint64)) | (es.view(np.uint64) != fs.view(np.uint64)))
    return [(x, tr.coincidence(slots[x]), e[x], f[x], es[x], fs[x]) for x in rows[:5]]


@pytest.mark.parametrize("name", NAMES)
def test_every_slot_pattern_by_index_and_by_value(name):
    X, slots, eo3, ev, A, G, sslots = partition_problem(name)
    n = len(slots)
    assert len({tr.coincidence(row) for row in slots}) == n == 203
    assert all(len(set(row[:, c].tolist())) == 6 for row in sslots for c in (0, 1))
    shared = check_against_reference(name, X, slots, eo3, ev, A, G, sslots, "203 slot patterns")
    # every slot of every row a block of its own with the same values: no block index coincides any more
    copies = np.ascontiguousarray(X[slots.ravel()])
    own = np.arange(n * 6, dtype=np.int32).reshape(n, 6)
    assert copies.nbytes < 20e6
    assert not differing(shared, run(copies, own, eo3, ev, A, G, sslots), slots)
    # every (sa, sg) its own copy of its row of A and of its block of G
    rows, blocks = np.ascontiguousarray(A[sslots[..., 0].ravel()]), np.ascontiguousarray(G[sslots[..., 1].ravel()])
    sown = np.repeat(np.arange(n * 6, dtype=np.int32), 2).reshape(n, 6, 2)
    assert not differing(shared, run(X, slots, eo3, ev, rows, blocks, sown), slots)
    assert not differing(shared, run(copies, own, eo3, ev, rows, blocks, sown), slots)


@pytest.mark.parametrize("name", NAMES)
def test_nothing_else_moves_the_bits(name):
    X, slots, eo3, ev, A, G, sslots = partition_problem(name)
    pick = np.arange(3, 203, 10)                                        # twenty coincidence patterns
    slots, eo3, sslots = slots[pick], eo3[pick], sslots[pick].copy()
    sslots[5] = cs.singles_slot_row(3, 0, 0, 2)                         # and repeated (sa, sg) in two rows
    sslots[15] = cs.singles_slot_row(3, 0, 2, 2)
    first = run(X, slots, eo3, ev, A, G, sslots)
    wide = tr.kernel_ref(X, slots, eo3, ev, extended=True)
    wide_s = cs.singles_ref(X, slots, A, G, sslots, eo3, ev, extended=True)
    assert (np.abs(first[0] - wide) <= tr.kernel_bound(X, slots, eo3, ev)).all()
    assert (np.abs(first[1] - wide_s) <= cs.singles_bound(X, slots, A, G, sslots, eo3, ev)).all()

    def same(second, what):
        assert first[0].tobytes() == second[0].tobytes() and first[1].tobytes() == second[1].tobytes(), (
            what, differing(first, second, slots))

    rng = np.random.default_rng(9)
    # the rows of A and the blocks of G elsewhere, each by its own permutation
    to_a, to_g = rng.permutation(A.shape[0]), rng.permutation(G.shape[0])
    assert (to_a != np.arange(A.shape[0])).sum() >= 8 and (to_g != np.arange(G.shape[0])).sum() >= 8 and (to_a != to_g).any()
    moved_a, moved_g = np.empty_like(A), np.empty_like(G)
    moved_a[to_a], moved_g[to_g] = A, G
    moved = np.stack([to_a[sslots[..., 0]], to_g[sslots[..., 1]]], axis=-1).astype(np.int32)
    same(run(X, slots, eo3, ev, moved_a, moved_g, moved), "A and G permuted")
    # fifty rows and forty blocks more that no triple names
    more_a = np.concatenate([A, rng.standard_normal((50,) + A.shape[1:]).astype(A.dtype)])
    more_g = np.concatenate([G, rng.standard_normal((40,) + G.shape[1:]).astype(G.dtype)])
    same(run(X, slots, eo3, ev, more_a, more_g, sslots), "unused rows and blocks")
    # the triples in the reverse order
    e, es = run(X, slots[::-1], eo3[::-1], ev, A, G, sslots[::-1])
    same((e[::-1], es[::-1]), "reverse order")
    # a triple alone
    for x in (0, 5, 19):
        e, es = run(X, slots[x:x + 1], eo3[x:x + 1], ev, A, G, sslots[x:x + 1])
        assert e.tobytes() == first[0][x:x + 1].tobytes() and es.tobytes() == first[1][x:x + 1].tobytes(), x
    # out= buffers that held something else
    out = tuple(torch.full((len(pick),), sentinel, dtype=torch.float64, device="cuda:0") for sentinel in (7.0, float("nan")))
    same(run(X, slots, eo3, ev, A, G, sslots, out=out), "out=")
    same((H(out[0]), H(out[1])), "the out= buffers themselves")


# -- rows of A and blocks of G past 2^31 elements


def test_rows_past_two_to_the_31_elements():
    """G of 2^31 // 100 + 7 blocks of 10^2 fp64 elements, then (G freed) A of 2^31 // 10 + 7 rows of 10 (17.2 GB each,
    allocated and never filled): the blocks (rows) that straddle byte 2^32 and element 2^31, the first and the last six
    hold data; the expected bits are those of the same rows and blocks packed into small arrays
    (``test_nothing_else_moves_the_bits``: where a row or a block sits does not move them)."""
    from quantum_systems_amd import kernels

    v = tile("f64") + 2
    assert v == 10
    torch.cuda.empty_cache()
    free, _ = torch.cuda.mem_get_info()
    if free < 24 * 2 ** 30:
        pytest.skip("needs 24 GB of free HBM (G, and then A, is 17.2 GB)")
    X, _, eo3, ev = tr.kernel_problem(v, 3, 9, 77)
    slots = np.array([[0, 1, 2, 3, 4, 8], [8, 2, 5, 1, 6, 7], [1, 2, 1, 2, 8, 8]], dtype=np.int32)
    A, G, _ = cs.singles_problem(v, 1, 9, 9, 78)
    sa = [[0, 1, 2, 3, 4, 8], [8, 2, 5, 1, 6, 7], [1, 1, 2, 2, 8, 8]]
    sg = [[1, 0, 3, 2, 8, 4], [7, 8, 2, 5, 1, 6], [2, 8, 1, 8, 1, 2]]
    sslots = np.stack([np.array(sa), np.array(sg)], axis=-1).astype(np.int32)
    assert set(sslots[..., 0].ravel().tolist()) == set(sslots[..., 1].ravel().tolist()) == set(range(9))
    expected = check_against_reference("f64", X, slots, eo3, ev, A, G, sslots, "nine rows and blocks, packed")
    Xd, slotsd, eo3d, evd = dev(X), dev(slots), dev(eo3), dev(ev)
    for which, small, per in (("G", G, v * v), ("A", A, v)):
        count = 2 ** 31 // per + 7
        where = [0, 2 ** 29 // per, 2 ** 31 // per] + list(range(count - 6, count))
        assert where[1] * 8 * per < 2 ** 32 < (where[1] + 1) * 8 * per and where[2] * per < 2 ** 31 < (where[2] + 1) * per
        assert count * per > 2 ** 31 and len(set(where)) == 9 and count < 2 ** 31
        far = sslots.copy()
        far[..., 1 if which == "G" else 0] = np.array(where, dtype=np.int64)[sslots[..., 1 if which == "G" else 0]]
        big = torch.empty((count,) + small.shape[1:], dtype=torch.float64, device="cuda:0")
        pair = None
        try:
            assert big.numel() > 2 ** 31 and big.numel() * 8 > 17e9
            for x, part in zip(where, dev(small)):
                big[x].copy_(part)
            pair = (dev(A), big) if which == "G" else (big, dev(G))
            e, es = kernels.triples_energy_singles(Xd, slotsd, eo3d, evd, *pair, dev(far))
            got = H(e), H(es)
        finally:
            del big, pair
            torch.cuda.empty_cache()
        assert got[0].tobytes() == expected[0].tobytes(), (which, got[0], expected[0])
        assert got[1].tobytes() == expected[1].tobytes(), (which, got[1], expected[1])


# -- RCCSD.triples at more than one tile

CASES = {"v10-real": (13, 3, False), "v8-complex": (11, 3, True), "v19-real": (21, 2, False)}


@pytest.fixture(scope="module")
def solved():
    """Canonical problems, the device's own converged amplitudes, (T) in one launch and its reference; every case once."""
    from quantum_systems_amd import RCCSD

    out = {}

    def case(key):
        if key not in out:
            l, ns, complex_ = CASES[key]
            h, u, eps = tr.canonical_problem(l, ns, 50 + l, complex_=complex_)
            ccsd = RCCSD(spatial_system(ns, h, u))
            ccsd.solve(tol=TOL, max_iter=200)
            assert ccsd.converged
            got = ccsd.triples()
            parts, passes = tuple(ccsd.triples_parts), list(ccsd.triples_passes)
            out[key] = (l, ns, h, u, eps, ccsd, got, parts, passes, triples_reference(u, eps, ns, H(ccsd.t1), H(ccsd.t)))
        return out[key]

    return case


@pytest.mark.parametrize("key", list(CASES))
def test_rccsd_triples_multi_tile(solved, key):
    """v = 10 real and v = 8 complex: T + 2, two tiles, every tile set counts, the seven triples of three occupied
    orbitals with both repeated-index patterns in both tables; v = 19 real: 2T + 3, three tiles, the triples (0, 0, 1) and
    (0, 1, 1)."""
    from quantum_systems_amd import RCCD, kernels

    l, ns, h, u, eps, ccsd, got, parts, passes, (wide, wide_s, tol, tol_s, _) = solved(key)
    complex_ = CASES[key][2]
    T = kernels.triples_tile(torch.complex128 if complex_ else torch.float64)
    assert (-(-(l - ns) // T), (l - ns) % T) == ((3, 3) if l == 21 else (2, 2))
    assert np.abs(H(ccsd.t1)).max() > 1e-4
    print(f"l = {l}, o = {ns}: E_[T] {parts[0]:.15e} (reference {wide:.15e}, deviation {abs(parts[0] - wide):.3e}, tolerance "
          f"{tol:.3e}), E_ST {parts[1]:.15e} (reference {wide_s:.15e}, deviation {abs(parts[1] - wide_s):.3e}, tolerance "
          f"{tol_s:.3e}), {ccsd.iterations} iterations")
    assert isinstance(got, float) and got == parts[0] + parts[1]
    assert abs(parts[0] - wide) <= tol and abs(parts[1] - wide_s) <= tol_s
    assert abs(wide) > 1e6 * tol and abs(wide_s) > 1e3 * tol_s                    # the tolerances are checks
    assert len(passes) == 1 and passes[0][:2] == (len(tr.triples(ns)), ns ** 3)
    assert f"qs::triples_energy_singles_kernel<{2 if complex_ else 1}>" in passes[0][2]
    assert "qs::triples_energy_kernel" not in passes[0][2]
    plain = RCCD(spatial_system(ns, h, u)).triples(ccsd.t)                        # the connected part: RCCD's on the same doubles
    assert abs(plain - wide) <= tol and abs(plain - parts[0]) <= tol


def test_multi_tile_passes(solved):
    from quantum_systems_amd import kernels

    l, ns, h, u, eps, ccsd, one, parts, _, (wide, wide_s, tol, tol_s, summed) = solved("v10-real")
    block = (l - ns) ** 3 * 8
    with kernels.tuning(triples_bytes=3 * block):                                 # one triple per pass
        passes = ccsd.triples()
        record, passes_parts = list(ccsd.triples_passes), tuple(ccsd.triples_parts)
    with kernels.tuning(triples_bytes=13 * block):                                # groups of several triples
        groups = ccsd.triples()
        grouped, groups_parts = list(ccsd.triples_passes), tuple(ccsd.triples_parts)
    todo = tr.triples(ns)
    print(f"one launch {parts}, one triple per pass {passes_parts}, groups {groups_parts}, summed bounds {summed:.3e}")
    assert [p[:2] for p in record] == [(1, len(set(tr.slot_row(ns, *ijk)))) for ijk in todo]
    assert 1 < len(grouped) < len(record) and all(p[1] <= 13 for p in grouped)
    assert sum(p[0] for p in grouped) == len(todo) and sum(p[1] for p in grouped) == sum(p[1] for p in record)
    assert all("qs::triples_energy_singles_kernel<1>" in p[2] and "qs::triples_energy_kernel" not in p[2]
               for p in record + grouped)
    assert abs(passes - one) <= summed and abs(groups - one) <= summed
    for x in (0, 1):
        assert abs(passes_parts[x] - parts[x]) <= summed and abs(groups_parts[x] - parts[x]) <= summed
    assert passes_parts[1] != 0.0 and groups_parts[1] != 0.0
    assert abs(parts[0] - wide) <= tol and abs(parts[1] - wide_s) <= tol_s
