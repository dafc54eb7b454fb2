"""``kernels.triples_energy_singles`` on the GPU against the NumPy references of tests/_triples_ref.py (the connected
part ``e``) and tests/_ccsd_ref.py (the singles part ``es``; tests/test_ccsd_ref_host.py pins that reference to the
determinant definition of (T)).

Tolerances (derived, not tuned): ``kernel_bound`` and ``singles_bound``, the any-order rounding bounds of the kernel's
two sums, against the ``numpy.longdouble`` evaluation of the same inputs.

The sizes here never make a last diagonal tile set count (where there is more than one tile, the last is a ragged tile of
one element, whose diagonal set adds 0 to both sums by identity): tests/test_gpu_triples_singles_scale.py has the ragged
tiles of two and more, more than three tiles, every slot pattern and the far offsets."""

import numpy as np
import pytest
import torch

import _ccsd_ref as cs
import _triples_ref as tr

pytestmark = pytest.mark.gpu
DTYPES = {"f64": torch.float64, "c128": torch.complex128}


def H(x):
    return torch.as_tensor(x).cpu().numpy()


def dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to("cuda:0")


def run(X, slots, eo3, ev, A, G, sslots, **kw):
    from quantum_systems_amd import kernels

    e, es = kernels.triples_energy_singles(dev(X), dev(slots), dev(eo3), dev(ev), dev(A), dev(G), dev(sslots), **kw)
    return H(e), H(es)


def tile_sizes(name):
    from quantum_systems_amd import kernels

    T = kernels.triples_tile(DTYPES[name])
    assert T == {"f64": 8, "c128": 6}[name]
    return [1, 2, 3, T - 1, T, T + 1, 2 * T + 1]


def mixed_problem(v, complex_, seed):
    """Four triples: six distinct blocks with six distinct (sa, sg); the table of i = j with repeated (sa, sg) entries;
    one block six times with distinct entries; six distinct blocks with repeated entries.  More blocks, rows of A and
    blocks of G than are used."""
    shares = (("none", "none"), ("pair", "repeat"), ("all", "none"), ("none", "repeat"))
    parts = [tr.kernel_problem(v, 1, 20, seed + 7 * x, complex_=complex_, share=share) for x, (share, _) in enumerate(shares)]
    X, _, _, ev = parts[0]
    slots = np.concatenate([p[1] for p in parts])
    eo3 = np.concatenate([p[2] for p in parts])
    singles = [cs.singles_problem(v, 1, 20, 30, seed + 1 + 7 * x, complex_=complex_, share=share)
               for x, (_, share) in enumerate(shares)]
    A, G, _ = singles[0]
    sslots = np.concatenate([s[2] for s in singles])
    assert len(set(sslots[..., 0].ravel().tolist())) < 20 and len(set(sslots[..., 1].ravel().tolist())) < 30
    return X, slots, eo3, ev, A, G, sslots


@pytest.mark.parametrize("index", range(7))
@pytest.mark.parametrize("name", ["f64", "c128"])
def test_kernel_against_reference(name, index):
    from quantum_systems_amd import kernels

    v = tile_sizes(name)[index]
    X, slots, eo3, ev, A, G, sslots = mixed_problem(v, name == "c128", 300 + v)
    wide = tr.kernel_ref(X, slots, eo3, ev, extended=True)
    bound = tr.kernel_bound(X, slots, eo3, ev)
    wide_s = cs.singles_ref(X, slots, A, G, sslots, eo3, ev, extended=True)
    bound_s = cs.singles_bound(X, slots, A, G, sslots, eo3, ev)
    e, es = run(X, slots, eo3, ev, A, G, sslots)
    log = kernels.last_dispatch()
    assert f"qs::triples_energy_singles_kernel<{1 if name == 'f64' else 2}>" in log
    assert "qs::triples_close_kernel" in log and "qs::triples_energy_kernel" not in log
    err = np.abs(e - wide).astype(np.float64)
    err_s = np.abs(es - wide_s).astype(np.float64)
    print(f"{name} v = {v}: e = {e}, deviation / bound = {err / bound}; es = {es}, deviation / bound = {err_s / bound_s}")
    assert np.isfinite(e).all() and (err <= bound).all()
    assert np.isfinite(es).all() and (err_s <= bound_s).all()
    # the bounds are checks on the non-degenerate rows (one block six times: Z = 0; v = 1: a = b = c only, Z = 0)
    rows = [0, 1, 3]
    assert ((np.abs(wide[rows]) > 1e3 * bound[rows]).all() and (np.abs(wide_s[rows]) > 1e3 * bound_s[rows]).all()) or v == 1
    # the connected part is the one of triples_energy
    alone = H(kernels.triples_energy(dev(X), dev(slots), dev(eo3), dev(ev)))
    assert (np.abs(alone - wide) <= bound).all()
    # A = 0: no singles part at all
    e0, es0 = run(X, slots, eo3, ev, np.zeros_like(A), G, sslots)
    assert (es0 == 0.0).all() and e0.tobytes() == e.tobytes()
    # the same bits on a second run
    e2, es2 = run(X, slots, eo3, ev, A, G, sslots)
    assert e.tobytes() == e2.tobytes() and es.tobytes() == es2.tobytes()


@pytest.mark.parametrize("name", ["f64", "c128"])
def test_batch_of_forty_and_a_triple_alone(name):
    v = tile_sizes(name)[5]                                             # T + 1: two tiles, a ragged one
    complex_ = name == "c128"
    X, slots, eo3, ev = tr.kernel_problem(v, 40, 12, 5, complex_=complex_)
    slots[7], slots[8] = [3, 4, 3, 4, 9, 9], [2] * 6
    A, G, sslots = cs.singles_problem(v, 40, 6, 9, 6, complex_=complex_)
    sslots[7] = cs.singles_problem(v, 1, 6, 9, 8, complex_=complex_, share="repeat")[2][0]
    wide = tr.kernel_ref(X, slots, eo3, ev, extended=True)
    wide_s = cs.singles_ref(X, slots, A, G, sslots, eo3, ev, extended=True)
    out = tuple(torch.full((40,), 7.0, dtype=torch.float64, device="cuda:0") for _ in range(2))
    e, es = run(X, slots, eo3, ev, A, G, sslots, out=out)
    assert (np.abs(e - wide) <= tr.kernel_bound(X, slots, eo3, ev)).all()
    assert (np.abs(es - wide_s) <= cs.singles_bound(X, slots, A, G, sslots, eo3, ev)).all()
    assert e.tobytes() == H(out[0]).tobytes() and es.tobytes() == H(out[1]).tobytes()
    for x in (0, 7, 8, 39):                                             # n = 1: the same bits as inside the batch
        e1, es1 = run(X, slots[x:x + 1], eo3[x:x + 1], ev, A, G, sslots[x:x + 1])
        assert e1.tobytes() == e[x:x + 1].tobytes() and es1.tobytes() == es[x:x + 1].tobytes(), x


@pytest.mark.parametrize("name", ["f64", "c128"])
def test_bad_entry_gives_nan_and_leaves_the_others(name):
    """Through the C entry point (the wrapper refuses such tables before the call): the kernel tests the six entries of
    ``slots`` and the twelve of ``sslots`` of its triple before it forms any address and returns, after one store of NaN
    to each of its two partials, where one is out of range: no load depends on the bad entry."""
    from quantum_systems_amd import _lib, kernels

    lib = _lib.load()
    v, n, nblocks, na, ng = tile_sizes(name)[5], 5, 9, 4, 8
    complex_ = name == "c128"
    X, slots, eo3, ev = tr.kernel_problem(v, n, nblocks, 60 + v, complex_=complex_)
    A, G, sslots = cs.singles_problem(v, n, na, ng, 61, complex_=complex_, share="repeat")
    code = kernels.dtype_code(DTYPES[name])
    nbytes = lib.qs_triples_energy_singles_workspace(code, v, n)
    assert nbytes == 16 * n * 4                                         # two tiles: four sets, two partials each
    Xd, eo3d, evd, Ad, Gd = dev(X), dev(eo3), dev(ev), dev(A), dev(G)
    work = torch.empty(nbytes, dtype=torch.uint8, device="cuda:0")

    def call(table, stable):
        sd, ssd = dev(table), dev(stable)
        e, es = (torch.full((n,), 7.0, dtype=torch.float64, device="cuda:0") for _ in range(2))
        rc = lib.qs_triples_energy_singles(code, Xd.data_ptr(), nblocks, sd.data_ptr(), eo3d.data_ptr(), evd.data_ptr(),
                                           Ad.data_ptr(), na, Gd.data_ptr(), ng, ssd.data_ptr(), v, n, e.data_ptr(),
                                           es.data_ptr(), work.data_ptr(), nbytes, kernels._stream())
        torch.cuda.synchronize()
        return rc, H(e), H(es)

    rc, good, good_s = call(slots, sslots)
    assert rc == 0 and np.isfinite(good).all() and np.isfinite(good_s).all()
    first = run(X, slots, eo3, ev, A, G, sslots)
    assert good.tobytes() == first[0].tobytes() and good_s.tobytes() == first[1].tobytes()
    others = [0, 1, 3, 4]
    cases = [("slots", (4,), nblocks), ("slots", (0,), -1), ("sslots", (1, 0), na), ("sslots", (5, 0), -1),
             ("sslots", (0, 1), ng), ("sslots", (3, 1), -1), ("sslots", (2, 1), 2 ** 31 - 1)]
    for which, entry, value in cases:
        bad, sbad = slots.copy(), sslots.copy()
        (bad if which == "slots" else sbad)[(2,) + entry] = value
        rc, e, es = call(bad, sbad)
        assert rc == 0, (which, entry, value)
        assert np.isnan(e[2]) and np.isnan(es[2]), (which, entry, value, e, es)
        assert e[others].tobytes() == good[others].tobytes() and es[others].tobytes() == good_s[others].tobytes()


def test_wrapper_refusals():
    from quantum_systems_amd import kernels

    X, slots, eo3, ev = tr.kernel_problem(3, 2, 6, 1)
    A, G, sslots = cs.singles_problem(3, 2, 6, 7, 2)
    bad = slots.copy()
    bad[1, 4] = 6
    with pytest.raises(ValueError, match="0 ... 5"):
        run(X, bad, eo3, ev, A, G, sslots)
    for column, top in ((0, 6), (1, 7)):
        for value in (top, -1):
            bad = sslots.copy()
            bad[1, 2, column] = value
            with pytest.raises(ValueError, match=f"0 ... {top - 1}"):
                run(X, slots, eo3, ev, A, G, bad)
    good = tuple(torch.empty(2, dtype=torch.float64, device="cuda:0") for _ in range(2))
    with pytest.raises(ValueError, match="out"):
        run(X, slots, eo3, ev, A, G, sslots, out=good[0])
    with pytest.raises(ValueError, match="out"):
        run(X, slots, eo3, ev, A, G, sslots, out=(good[0], torch.empty(3, dtype=torch.float64, device="cuda:0")))
    with pytest.raises(ValueError, match="out"):
        run(X, slots, eo3, ev, A, G, sslots, out=(torch.empty(2, dtype=torch.float64), good[1]))
    with pytest.raises(RuntimeError, match="GPU only"):
        kernels.triples_energy_singles(dev(X), dev(slots), dev(eo3), dev(ev), torch.from_numpy(A), dev(G), dev(sslots))
