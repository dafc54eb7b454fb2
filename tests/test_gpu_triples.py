"""``kernels.triples_energy`` and ``coupled_cluster.RCCD.triples`` on the GPU against the NumPy reference of
tests/_triples_ref.py (tests/test_triples_ref_host.py pins that reference to the determinant definition).

Tolerances (derived, not tuned):
  * the kernel alone: ``kernel_bound``, the any-order rounding bound of its own sum, against the ``numpy.longdouble``
    evaluation of the same blocks;
  * ``RCCD.triples`` end to end: the device forms its blocks from transformed integral blocks, so its inputs differ from
    the reference's by the rounding of those transforms and ``kernel_bound`` alone does not apply: 16 times the
    difference of the fp64 working form from its long-double evaluation for that case (16: the margin for the device's
    other summation order and its transform), plus ``kernel_bound`` summed over the triples with their weights."""

import numpy as np
import pytest
import torch

import _rccd_ref as rc
import _triples_ref as tr

pytestmark = pytest.mark.gpu
E_NUC = 0.25
DTYPES = {"f64": torch.float64, "c128": torch.complex128}


def H(x):
    return torch.as_tensor(x).cpu().numpy()


def dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to("cuda:0")


def run(X, slots, eo3, ev, **kw):
    from quantum_systems_amd import kernels

    return kernels.triples_energy(dev(X), dev(slots), dev(eo3), dev(ev), **kw)


def spatial_system(ns, h, u):
    """2 ns particles in ns doubly occupied of the orthonormal spatial orbitals given as they are."""
    import quantum_systems_amd as qsa
    from quantum_systems_amd import hip

    l = h.shape[0]
    bs = qsa.setup_basis_set(2 * ns, l, hip.asarray(np.eye(l)), hip.asarray(h), hip.asarray(u), 2, -1, hip, False,
                             False, nuclear_repulsion_energy=E_NUC)
    return qsa.SpatialOrbitalSystem(2 * ns, bs)


def tile_sizes(name):
    from quantum_systems_amd import kernels

    T = kernels.triples_tile(DTYPES[name])
    assert T == {"f64": 8, "c128": 6}[name]
    # a lone (ragged) diagonal tile; a full one; two tiles (sets with two and three equal indices); three (all different)
    # (a ragged tile of ONE element, T + 1 and 2 T + 1: its diagonal set holds a = b = c alone and adds 0 by identity --
    # tests/test_gpu_triples_scale.py has the ragged tiles of two and more, and more than three tiles)
    return [1, 2, 3, T - 1, T, T + 1, 2 * T + 1]


def mixed_problem(v, complex_, seed):
    """Three triples: six distinct blocks, the table of i = j, one block six times; more blocks than are used."""
    parts = [tr.kernel_problem(v, 1, 20, seed, complex_=complex_, share=share) for share in ("none", "pair", "all")]
    X, _, _, ev = parts[0]
    slots = np.concatenate([p[1] for p in parts])
    eo3 = np.concatenate([p[2] for p in parts])
    assert len(set(slots.ravel().tolist())) < X.shape[0]
    return X, slots, eo3, ev


@pytest.mark.parametrize("index", range(7))
@pytest.mark.parametrize("name", ["f64", "c128"])
def test_kernel_against_reference(name, index):
    from quantum_systems_amd import kernels

    v = tile_sizes(name)[index]
    X, slots, eo3, ev = mixed_problem(v, name == "c128", 100 + v)
    wide = tr.kernel_ref(X, slots, eo3, ev, extended=True)
    bound = tr.kernel_bound(X, slots, eo3, ev)
    got = H(run(X, slots, eo3, ev))
    assert f"qs::triples_energy_kernel<{1 if name == 'f64' else 2}>" in kernels.last_dispatch()
    assert "qs::triples_close_kernel" in kernels.last_dispatch()
    err = np.abs(got - wide).astype(np.float64)
    print(f"{name} v = {v}: e = {got}, deviation / bound = {err / bound}")
    assert np.isfinite(got).all() and (err <= bound).all()
    assert (np.abs(wide[:2]) > 1e3 * bound[:2]).all() or v == 1       # the bound is a check (v = 1: a = b = c only, e = 0)
    again = H(run(X, slots, eo3, ev))
    assert got.tobytes() == again.tobytes()                             # the same bits on a second run


@pytest.mark.parametrize("name", ["f64", "c128"])
def test_batch_of_forty_and_a_triple_alone(name):
    v = tile_sizes(name)[5]                                             # T + 1: two tiles, a ragged one
    X, slots, eo3, ev = tr.kernel_problem(v, 40, 12, 5, complex_=name == "c128")
    slots[7], slots[8] = [3, 4, 3, 4, 9, 9], [2] * 6
    wide = tr.kernel_ref(X, slots, eo3, ev, extended=True)
    bound = tr.kernel_bound(X, slots, eo3, ev)
    out = torch.full((40,), 7.0, dtype=torch.float64, device="cuda:0")
    got = H(run(X, slots, eo3, ev, out=out))
    assert (np.abs(got - wide) <= bound).all()
    assert got.tobytes() == H(out).tobytes()
    for x in (0, 7, 8, 39):                                             # n = 1: the same bits as inside the batch
        alone = H(run(X, slots[x:x + 1], eo3[x:x + 1], ev))
        assert alone.tobytes() == got[x:x + 1].tobytes(), x


def test_wrapper_refusals():
    from quantum_systems_amd import kernels

    X, slots, eo3, ev = tr.kernel_problem(3, 2, 6, 1)
    bad = slots.copy()
    bad[1, 4] = 6
    with pytest.raises(ValueError, match="0 ... 5"):
        run(X, bad, eo3, ev)
    bad[1, 4] = -1
    with pytest.raises(ValueError, match="0 ... 5"):
        run(X, bad, eo3, ev)
    with pytest.raises(ValueError, match="out"):
        run(X, slots, eo3, ev, out=torch.empty(3, dtype=torch.float64, device="cuda:0"))
    with pytest.raises(ValueError, match="out"):
        run(X, slots, eo3, ev, out=torch.empty(2, dtype=torch.float64))
    with pytest.raises(RuntimeError, match="GPU only"):
        kernels.triples_energy(torch.from_numpy(X), dev(slots), dev(eo3), dev(ev))


# -- RCCD.triples


def end_to_end_case(ls, ns, complex_, seed):
    """A canonical problem, seeded amplitudes, the long-double working form and the tolerance of the module docstring."""
    h, u, eps = tr.canonical_problem(ls, ns, seed, complex_=complex_)
    t = rc.closed_shell_amplitudes(np.random.default_rng(seed + 1), ls - ns, ns, complex_=complex_)
    return (h, u, eps, t) + reference(u, eps, ns, t)


def reference(u, eps, ns, t):
    _, wide = tr.working(u, eps, ns, t, extended=True)
    _, own = tr.working(u, eps, ns, t)
    X = tr.packed_blocks(tr.blocks(u, ns, t))
    todo = tr.triples(ns)
    slots = [tr.slot_row(ns, *ijk) for ijk in todo]
    eo3 = [eps[i] + eps[j] + eps[k] for i, j, k in todo]
    bound = tr.kernel_bound(X, slots, eo3, eps[ns:])
    summed = float(sum(tr.weight(*ijk) * b for ijk, b in zip(todo, bound)))
    return float(wide), 16 * abs(float(own - wide)) + summed, summed


@pytest.mark.parametrize("complex_", [False, True], ids=["real", "complex"])
@pytest.mark.parametrize("ls, ns", [(6, 2), (9, 3)])
def test_rccd_triples_against_working_form(ls, ns, complex_):
    from quantum_systems_amd import RCCD, hip

    h, u, eps, t, wide, tol, _ = end_to_end_case(ls, ns, complex_, 50 + ls)
    ccd = RCCD(spatial_system(ns, h, u))
    got = ccd.triples(hip.asarray(t))
    # observed on an MI355X, |device - long double| against the tolerance: (6, 2) real 0 of 9.7e-15, complex 1.4e-17 of
    # 1.2e-13; (9, 3) real 5.6e-17 of 3.2e-13, complex 0 of 4.6e-12 -- the summed kernel_bound is nearly all of the
    # tolerance.  With C given (the test below): 5e-17 of 6.5e-15 real, 7e-17 of 9.7e-14 complex; first-order amplitudes:
    # below 1e-19 of 1.7e-16
    print(f"l = {ls}, o = {ns}, {'complex' if complex_ else 'real'}: E_T {got:.15e}, reference {wide:.15e}, "
          f"deviation {abs(got - wide):.3e}, tolerance {tol:.3e}")
    assert isinstance(got, float) and got < 0.0
    assert abs(got - wide) <= tol
    assert abs(wide) > 1e6 * tol                                        # the tolerance is a check
    assert len(ccd.triples_passes) == 1 and ccd.triples_passes[0][:2] == (len(tr.triples(ns)), ns ** 3)
    assert "qs::triples_energy_kernel" in ccd.triples_passes[0][2]
    if not complex_:
        assert ccd._dt == torch.float64 and ccd._triples_blocks[0].dtype == torch.float64


@pytest.mark.parametrize("complex_", [False, True], ids=["real", "complex"])
def test_rccd_triples_with_coefficients(complex_):
    """``C`` and ``epsilon`` given, ``u`` in another basis: the same number as on the system in the orbital basis."""
    from quantum_systems_amd import RCCD, hip

    ls, ns = 6, 2
    h, u, eps, t, wide, tol, _ = end_to_end_case(ls, ns, complex_, 70)
    _, _, C = rc.closed_shell_problem(ls, 71, complex_=complex_)          # unitary
    h_ao = C @ h @ C.conj().T
    u_ao = np.einsum("pa,qb,abcd,rc,sd->pqrs", C, C, u, C.conj(), C.conj(), optimize=True)
    moved = RCCD(spatial_system(ns, h_ao, u_ao), hip.asarray(C), hip.asarray(eps)).triples(hip.asarray(t))
    plain = RCCD(spatial_system(ns, h, u)).triples(hip.asarray(t))
    print(f"with C {moved:.15e}, orbital basis {plain:.15e}, reference {wide:.15e}, tolerance {tol:.3e}")
    assert abs(plain - wide) <= tol and abs(moved - wide) <= tol


def test_first_order_amplitudes():
    from quantum_systems_amd import RCCD

    ls, ns = 6, 2
    h, u, eps = tr.canonical_problem(ls, ns, 90, complex_=True)
    t1 = rc.first_order(np.diag(eps).astype(u.dtype), u, ns)
    wide, tol, _ = reference(u, eps, ns, t1)
    ccd = RCCD(spatial_system(ns, h, u))
    ccd.solve(max_iter=0)
    got = ccd.triples()
    print(f"first-order amplitudes: E_T {got:.15e}, reference {wide:.15e}, tolerance {tol:.3e}")
    assert abs(got - wide) <= tol


def test_passes_under_a_small_budget():
    from quantum_systems_amd import RCCD, hip, kernels

    ls, ns = 7, 3
    h, u, eps, t, wide, tol, summed = end_to_end_case(ls, ns, False, 31)
    ccd = RCCD(spatial_system(ns, h, u))
    one = ccd.triples(hip.asarray(t))
    assert len(ccd.triples_passes) == 1
    block = (ls - ns) ** 3 * 8
    with kernels.tuning(triples_bytes=3 * block):                       # three blocks: one triple per pass, also the one
        passes = ccd.triples(hip.asarray(t))                            # that owns six (two with three each would share six)
        record = list(ccd.triples_passes)
    with kernels.tuning(triples_bytes=1):                               # less than one block: still one triple per pass
        least = ccd.triples(hip.asarray(t))
        assert len(ccd.triples_passes) == len(record)
    with kernels.tuning(triples_bytes=13 * block):                      # groups of several triples, blocks of their own only
        groups = ccd.triples(hip.asarray(t))
        assert 1 < len(ccd.triples_passes) < len(record) and all(p[1] <= 13 for p in ccd.triples_passes)
    todo = tr.triples(ns)
    print(f"one launch {one:.15e}, one triple per pass {passes:.15e}, groups {groups:.15e}, summed bound {summed:.3e}")
    assert [p[:2] for p in record] == [(1, len(set(tr.slot_row(ns, *ijk)))) for ijk in todo]
    assert all("qs::triples_energy_kernel<1>" in p[2] for p in record)
    assert abs(passes - one) <= summed and abs(groups - one) <= summed and abs(least - one) <= summed
    assert abs(one - wide) <= tol


def test_refusals_and_hartree_fock_entry_point():
    import quantum_systems_amd as qsa
    from quantum_systems_amd import RCCD, HartreeFock, hip
    from quantum_systems_amd.sharded_module import ShardedTensor4

    ls, ns = 6, 2
    h, u, C = rc.closed_shell_problem(ls, 3)                             # a rotated, non-canonical C
    f, _ = rc.orbital_tensors(h, u, C, ns)
    ccd = RCCD(spatial_system(ns, h, u), hip.asarray(C), hip.asarray(np.real(np.diagonal(f)).copy()))
    with pytest.raises(ValueError, match="canonical"):
        ccd.triples()
    h, u, eps = tr.canonical_problem(ls, ns, 4)
    system = spatial_system(ns, h, u)
    ccd = RCCD(system)
    assert ccd.triples() < 0.0
    for shape in ((ns, ns, ls - ns, ls - ns), (ls - ns, ls - ns, ns), (ls, ls, ns, ns)):
        with pytest.raises(ValueError, match="v, v, o, o"):
            ccd.triples(hip.asarray(np.zeros(shape)))
    system._basis_set.u = ShardedTensor4(torch.as_tensor(system.u).as_subclass(torch.Tensor).contiguous(), ls, 0, 0, 1)
    with pytest.raises(NotImplementedError, match="one device"):
        ccd.triples()
    with pytest.raises(NotImplementedError, match="one device"):
        RCCD(system)

    spatial = qsa.SpatialOrbitalSystem(4, qsa.ODQD(8, 8.0, 201, potential=qsa.ODQD.HOPotential(omega=1.0), np=hip))
    hf = HartreeFock(spatial)
    hf.scf(tol=1e-10)
    assert hf.converged
    ccd = hf.ccd()
    e_ccd = ccd.solve(tol=1e-9)
    e_t = ccd.triples()
    print(f"ODQD l = 8, 4 electrons: RCCD {e_ccd:.10f}, +T {e_t:.10f}")
    assert ccd.converged and e_t < 0.0 and abs(e_t) < abs(e_ccd)
