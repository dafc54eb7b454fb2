"""``kernels.triples_energy`` where tests/test_gpu_triples.py cannot see: more than three tiles along an index, a closing
sum of more than 256 partials, ragged tiles of more than one element, every coincidence of the six slots, block offsets
past 2^31 elements, the NaN of a bad slot through the C entry point, and ``RCCD.triples`` at more than one tile.

What the sizes are for (T = ``kernels.triples_tile``: 8 for fp64, 6 for complex128):
  * 3T: three full, different tiles, the set (0, 1, 2) with all 36 tiles in LDS on every thread; 3T + 2: a ragged tile
    of two; 4T - 1: nt = 4, one short; 10T + 2: nt = 11, 286 tile sets, so the closing kernel's strided loop takes a second
    trip.  T + 2 for everything that is about slots and addresses: two tiles, the ragged one of two elements.
  * never a ragged tile of ONE element: its diagonal set holds a = b = c alone, where the six W are equal and Z = 0, so
    the workgroup of that set adds 0 by identity and a kernel that lost it would pass.  ``tile_set_sensitivity``, from the
    reference alone and before the device result is looked at, asserts that every other tile set of every triple adds at
    least 100 ``kernel_bound``: a workgroup skipped or corrupted fails the test.  Two slot patterns are 0 by identity
    themselves and the condition cannot be put to them (they are in the tables for their loads and their bits): ONE
    block in all six slots (W totally symmetric, e = 0: ``e_iii``), all of its sets; and one block at the even orders,
    one at the odd ones (W cyclic, so totally symmetric where two indices are equal), the diagonal set of a ragged tile of
    two.  tests/test_triples_ref_host.py shows that nothing else is left out.

Tolerances: ``kernel_bound`` against the long-double evaluation, and the end-to-end rule of tests/test_gpu_triples.py;
nothing else.  Equal bits are asserted as equal bits.

Observed on an MI355X, largest deviation / ``kernel_bound`` over the triples of a case (fp64, complex128): 3T 3.3e-6,
4.0e-6; 3T + 2 1.2e-6, 1.7e-6; 4T - 1 1.4e-6, 1.4e-6; 10T + 2 7.8e-8, 6.9e-9; the 203 slot patterns at T + 2 1.8e-4, 6.4e-5
(the largest of each type); the nine packed blocks of the far-offset test 8.4e-5.  The least tile-set contribution in
bounds: 2.2e3 and 7.6e3 at 10T + 2, 1.0e6 and more elsewhere.  ``RCCD.triples``, |device - long double| of the tolerance:
v = 9 real 0 of 3.3e-12, complex 1.8e-15 of 5.1e-11; v = 17 4.4e-16 of 4.0e-11; v = 10 0 of 6.6e-12.  Every test of this
file takes 0.2 s or less.  A close that takes one trip fails 10T + 2 alone, of this file and of test_gpu_triples.py; a
kernel whose last diagonal tile set adds nothing passes test_gpu_triples.py at T + 1 and 2T + 1 and fails every kernel
case here."""

import numpy as np
import pytest
import torch

import _triples_ref as tr
from test_gpu_triples import DTYPES, H, dev, end_to_end_case, mixed_problem, run, spatial_system

pytestmark = pytest.mark.gpu
NAMES = ["f64", "c128"]


def tile(name):
    from quantum_systems_amd import kernels

    T = kernels.triples_tile(DTYPES[name])
    assert T == {"f64": 8, "c128": 6}[name]
    return T


def check_against_reference(name, X, slots, eo3, ev, label):
    """The assertions of ``test_kernel_against_reference`` and the sensitivity of the inputs; returns the device's ``e``."""
    from quantum_systems_amd import kernels

    wide = tr.kernel_ref(X, slots, eo3, ev, extended=True)
    bound = tr.kernel_bound(X, slots, eo3, ev)
    least = tr.tile_set_sensitivity(X, slots, eo3, ev, tile(name))
    print(f"{name} {label}: the least tile set adds {least:.3e} bounds")
    assert len(ev) % tile(name) != 1 and least >= 100                   # a condition on the inputs: every workgroup counts
    got = H(run(X, slots, eo3, ev))
    assert f"qs::triples_energy_kernel<{1 if name == 'f64' else 2}>" in kernels.last_dispatch()
    assert "qs::triples_close_kernel" in kernels.last_dispatch()
    err = np.abs(got - wide).astype(np.float64)
    print(f"{name} {label}: e = {got[:4]}, largest deviation / bound = {(err / bound).max():.3e}")
    assert np.isfinite(got).all() and (err <= bound).all()
    again = H(run(X, slots, eo3, ev))
    assert got.tobytes() == again.tobytes()                             # the same bits on a second run
    return got


# -- more tile sets


def many_sets_problem(name, index):
    T = tile(name)
    v = [3 * T, 3 * T + 2, 4 * T - 1, 10 * T + 2][index]
    if index < 3:
        return (v,) + mixed_problem(v, name == "c128", 100 + v)
    # nt = 11: six distinct blocks, and one block six times; 7 blocks
    X, slots, eo3, ev = tr.kernel_problem(v, 2, 7, 100 + v, complex_=name == "c128")
    slots[0], slots[1] = [3, 0, 5, 1, 6, 2], [4] * 6
    return v, X, slots, eo3, ev


@pytest.mark.parametrize("index", range(4))
@pytest.mark.parametrize("name", NAMES)
def test_more_tile_sets(name, index):
    v, X, slots, eo3, ev = many_sets_problem(name, index)
    nt = -(-v // tile(name))
    assert nt == [3, 4, 4, 11][index] and (nt * (nt + 1) * (nt + 2) // 6 > 256) == (index == 3)
    check_against_reference(name, X, slots, eo3, ev, f"v = {v}, {nt} tiles")


# -- every coincidence of the six slots


def partition_problem(name):
    """203 triples on a dozen blocks at v = T + 2, one per coincidence pattern."""
    v = tile(name) + 2
    X, _, eo3, ev = tr.kernel_problem(v, 203, 12, 300 + v, complex_=name == "c128")
    return X, tr.slot_partitions(12, seed=v), eo3, ev


@pytest.mark.parametrize("name", NAMES)
def test_every_slot_pattern_by_index_and_by_value(name):
    X, slots, eo3, ev = partition_problem(name)
    assert len({tr.coincidence(row) for row in slots}) == 203
    shared = check_against_reference(name, X, slots, eo3, ev, "203 slot patterns")
    # every slot of every row a block of its own with the same values: no block index coincides any more
    copies = np.ascontiguousarray(X[slots.ravel()])
    own = np.arange(203 * 6, dtype=np.int32).reshape(203, 6)
    assert copies.nbytes < 20e6
    by_value = H(run(copies, own, eo3, ev))
    differ = np.flatnonzero(shared.view(np.uint64) != by_value.view(np.uint64))
    assert differ.size == 0, [(x, tr.coincidence(slots[x]), shared[x], by_value[x]) for x in differ[:5]]


@pytest.mark.parametrize("name", NAMES)
def test_nothing_else_moves_the_bits(name):
    X, slots, eo3, ev = partition_problem(name)
    pick = np.arange(3, 203, 10)                                        # twenty coincidence patterns
    slots, eo3 = slots[pick], eo3[pick]
    first = H(run(X, slots, eo3, ev))
    wide = tr.kernel_ref(X, slots, eo3, ev, extended=True)
    assert (np.abs(first - wide) <= tr.kernel_bound(X, slots, eo3, ev)).all()
    rng = np.random.default_rng(9)
    # the blocks elsewhere in X
    to = rng.permutation(X.shape[0])
    assert (to != np.arange(X.shape[0])).sum() >= 8
    moved = np.empty_like(X)
    moved[to] = X
    assert H(run(moved, to[slots].astype(np.int32), eo3, ev)).tobytes() == first.tobytes()
    # fifty blocks more that no triple names
    more = np.concatenate([X, rng.standard_normal((50,) + X.shape[1:]).astype(X.dtype)])
    assert H(run(more, slots, eo3, ev)).tobytes() == first.tobytes()
    # the triples in the reverse order
    assert H(run(X, slots[::-1], eo3[::-1], ev))[::-1].tobytes() == first.tobytes()


# -- a slot outside X, through the C entry point (the wrapper refuses such a table before the call)


@pytest.mark.parametrize("name", NAMES)
def test_bad_slot_gives_nan_and_leaves_the_others(name):
    """The kernel tests the six slots of its triple before it forms any address into X and returns (after ONE store of NaN
    to its partial) where one is outside 0 ... nblocks - 1: no load of X depends on the bad entry."""
    from quantum_systems_amd import _lib, kernels

    lib = _lib.load()
    v, n, nblocks = tile(name) + 2, 5, 9
    X, slots, eo3, ev = tr.kernel_problem(v, n, nblocks, 40 + v, complex_=name == "c128")
    code = kernels.dtype_code(DTYPES[name])
    nbytes = lib.qs_triples_energy_workspace(code, v, n)
    assert nbytes == 8 * n * 4                                          # two tiles: four sets
    Xd, eo3d, evd = dev(X), dev(eo3), dev(ev)
    work = torch.empty(nbytes, dtype=torch.uint8, device="cuda:0")

    def call(table):
        sd = dev(table)
        e = torch.full((n,), 7.0, dtype=torch.float64, device="cuda:0")
        rc = lib.qs_triples_energy(code, Xd.data_ptr(), nblocks, sd.data_ptr(), eo3d.data_ptr(), evd.data_ptr(), v, n,
                                   e.data_ptr(), work.data_ptr(), nbytes, kernels._stream())
        torch.cuda.synchronize()
        return rc, H(e)

    rc, good = call(slots)
    assert rc == 0 and np.isfinite(good).all()
    assert good.tobytes() == H(run(X, slots, eo3, ev)).tobytes()
    for entry, value in ((4, nblocks), (0, -1), (3, 2 ** 31 - 1)):
        bad = slots.copy()
        bad[2, entry] = value
        rc, got = call(bad)
        assert rc == 0, value
        assert np.isnan(got[2]), (value, got)
        assert got[[0, 1, 3, 4]].tobytes() == good[[0, 1, 3, 4]].tobytes(), (value, got, good)


# -- block offsets past 2^31 elements


def test_blocks_past_two_to_the_31_elements():
    """X of 2^31 // 1000 + 7 blocks of 10^3 fp64 elements (17.2 GB, allocated and never filled): the blocks that straddle
    byte 2^32 and element 2^31, the first and the last six hold data; the expected bits are those of the same blocks
    packed into a small X (``test_nothing_else_moves_the_bits``: where a block sits does not move them)."""
    from quantum_systems_amd import kernels

    v = tile("f64") + 2
    assert v == 10
    nblocks = 2 ** 31 // 1000 + 7
    torch.cuda.empty_cache()
    free, _ = torch.cuda.mem_get_info()
    if free < 24 * 2 ** 30:
        pytest.skip("needs 24 GB of free HBM (X is 17.2 GB)")
    where = [0, 2 ** 29 // 1000, 2 ** 31 // 1000] + list(range(nblocks - 6, nblocks))
    assert where[1] * 8000 < 2 ** 32 < (where[1] + 1) * 8000 and where[2] * 1000 < 2 ** 31 < (where[2] + 1) * 1000
    assert nblocks * 1000 > 2 ** 31 and len(set(where)) == 9
    small, _, eo3, ev = tr.kernel_problem(v, 3, 9, 77)
    packed = np.array([[0, 1, 2, 3, 4, 8], [8, 2, 5, 1, 6, 7], [1, 2, 1, 2, 8, 8]], dtype=np.int32)
    expected = check_against_reference("f64", small, packed, eo3, ev, "nine blocks, packed")
    X = torch.empty((nblocks, v, v, v), dtype=torch.float64, device="cuda:0")
    assert X.numel() > 2 ** 31
    try:
        for x, block in zip(where, dev(small)):
            X[x].copy_(block)
        far = np.array(where, dtype=np.int64)[packed].astype(np.int32)
        got = H(kernels.triples_energy(X, dev(far), dev(eo3), dev(ev)))
    finally:
        del X
        torch.cuda.empty_cache()
    assert got.tobytes() == expected.tobytes(), (got, expected)


# -- RCCD.triples at more than one tile


@pytest.mark.parametrize("ls, ns, complex_", [(12, 3, False), (12, 3, True), (19, 2, False), (13, 3, False)],
                         ids=["v9-real", "v9-complex", "v17-real", "v10-real"])
def test_rccd_triples_multi_tile(ls, ns, complex_):
    """v = 9: two tiles in both types, the seven triples of three occupied orbitals with both repeated-index patterns;
    v = 17: three tiles, the triples (0, 0, 1) and (0, 1, 1) only, every launch row a shared-block pattern.  In fp64
    both are T + 1 and 2 T + 1, a ragged tile of one element (the blind spot of the module docstring: these cases are
    about the products, the slot table and the groups); v = 10 is the fp64 case whose every tile set counts."""
    from quantum_systems_amd import RCCD, hip, kernels

    h, u, eps, t, wide, tol, _ = end_to_end_case(ls, ns, complex_, 50 + ls)
    dt = torch.complex128 if complex_ else torch.float64
    assert -(-(ls - ns) // kernels.triples_tile(dt)) == (3 if ls == 19 else 2)
    assert ((ls - ns) % kernels.triples_tile(dt) != 1) == (complex_ or ls == 13)
    patterns = {tr.coincidence(tr.slot_row(ns, *ijk)) for ijk in tr.triples(ns)}
    assert {(0, 1, 0, 1, 2, 2), (0, 0, 1, 2, 1, 2)} <= patterns
    ccd = RCCD(spatial_system(ns, h, u))
    got = ccd.triples(hip.asarray(t))
    print(f"l = {ls}, o = {ns}, {'complex' if complex_ else 'real'}: E_T {got:.15e}, reference {wide:.15e}, "
          f"deviation {abs(got - wide):.3e}, tolerance {tol:.3e}")
    assert isinstance(got, float) and got < 0.0
    assert abs(got - wide) <= tol
    assert abs(wide) > 1e6 * tol                                        # the tolerance is a check
    assert len(ccd.triples_passes) == 1 and ccd.triples_passes[0][:2] == (len(tr.triples(ns)), ns ** 3)
    assert f"qs::triples_energy_kernel<{2 if complex_ else 1}>" in ccd.triples_passes[0][2]


def test_multi_tile_passes():
    from quantum_systems_amd import RCCD, hip, kernels

    ls, ns = 12, 3
    h, u, eps, t, wide, tol, summed = end_to_end_case(ls, ns, False, 50 + ls)
    ccd = RCCD(spatial_system(ns, h, u))
    one = ccd.triples(hip.asarray(t))
    assert len(ccd.triples_passes) == 1
    block = (ls - ns) ** 3 * 8
    with kernels.tuning(triples_bytes=3 * block):                       # one triple per pass
        passes = ccd.triples(hip.asarray(t))
        record = list(ccd.triples_passes)
    with kernels.tuning(triples_bytes=13 * block):                      # groups of several triples
        groups = ccd.triples(hip.asarray(t))
        grouped = list(ccd.triples_passes)
    todo = tr.triples(ns)
    print(f"one launch {one:.15e}, one triple per pass {passes:.15e}, groups {groups:.15e}, summed bound {summed:.3e}")
    assert [p[:2] for p in record] == [(1, len(set(tr.slot_row(ns, *ijk)))) for ijk in todo]
    assert 1 < len(grouped) < len(record) and all(p[1] <= 13 for p in grouped)
    assert sum(p[0] for p in grouped) == len(todo) and sum(p[1] for p in grouped) == sum(p[1] for p in record)
    assert all("qs::triples_energy_kernel<1>" in p[2] for p in record + grouped)
    assert abs(passes - one) <= summed and abs(groups - one) <= summed
    assert abs(one - wide) <= tol


def test_one_occupied_orbital_launches_nothing():
    from quantum_systems_amd import RCCD, kernels

    h, u, eps = tr.canonical_problem(4, 1, 12)
    ccd = RCCD(spatial_system(1, h, u))
    before = kernels.last_dispatch()
    kernels.dispatch_log = []
    try:
        got = ccd.triples()
        launched = list(kernels.dispatch_log)
    finally:
        kernels.dispatch_log = None
    assert isinstance(got, float) and got == 0.0
    assert ccd.triples_passes == [] and launched == [] and kernels.last_dispatch() == before
