"""``kernels.transform_two_body_blocks`` / ``kernels.lead_contract`` (qs_lead_contract.hip) and MP2 on the GPU.

Parity is against the numpy.longdouble restatement (tests/_blocks_ref.py) under its any-order bound
gamma_(4L+8) * A (complex: times 2 sqrt 2), every element of every case; the largest error / bound per form is printed
and, when QS_BLOCKS_PARITY_OUT names a file, appended there.  The bit tests state what the C ABI promises of
``qs_lead_contract``: one chain per element, whatever the row count, the width, the leading dimension or the base.

Measured on the MI355X (profiles/r08_blocks.txt): largest error / bound 0.010 (fp64), 0.004 (complex128), 0.003
(mixed); MP2 differences against the restatement <= 3e-17 under tolerances of 3e-14 ... 3e-12; 17 tests in 10 s."""

import os

import numpy as np
import pytest
import torch

import _blocks_ref as ref

pytestmark = pytest.mark.gpu
FORMS = ["fp64", "complex128", "mixed"]
# L, (M0, M1, M2, M3)
LEAD_ROWS_MAX = 32
CASES = [(5, (1, 1, 4, 4)), (20, (3, 3, 17, 17)), (33, (10, 10, 23, 23)), (55, (6, 6, 49, 49)), (24, (24, 2, 5, 7)),
         (40, (33, 4, 4, 4))]


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def host(t):
    return torch.as_tensor(t).cpu().numpy()


def rand(rng, form, which, *shape):
    x = rng.standard_normal(shape)
    cplx = form == "complex128" or (form == "mixed" and which == "C")
    return x + 1j * rng.standard_normal(shape) if cplx else x


def operands(form, L, M, seed):
    rng = np.random.default_rng(seed)
    u = rand(rng, form, "u", L, L, L, L)
    return u, rand(rng, form, "C", M[0], L), rand(rng, form, "C", M[1], L), rand(rng, form, "C", L, M[2]), \
        rand(rng, form, "C", L, M[3])


def last_dispatch():
    from quantum_systems_amd import _lib

    return _lib.load().qs_last_dispatch().decode()


@pytest.mark.parametrize("form", FORMS)
def test_parity_within_the_bound_against_long_double(form):
    from quantum_systems_amd import kernels

    # every case with M0 <= 32 on the lead kernel (the library's default keeps it to the measured crossover); the
    # default itself is covered by the other tests of this file
    kernels.tuning_set("lead_rows_max", LEAD_ROWS_MAX)
    worst = 0.0
    for L, M in CASES:
        ops = operands(form, L, M, seed=1000 + L)
        got = host(kernels.transform_two_body_blocks(*map(dev, ops)))
        ran = last_dispatch()
        assert got.shape == M and got.dtype == (np.float64 if form == "fp64" else np.complex128)
        if M[0] <= LEAD_ROWS_MAX:
            assert "lead_contract_kernel" in ran, (L, M, ran)
        else:
            assert "lead_contract_kernel" not in ran and "gemm" in ran, (L, M, ran)
        exact = ref.blocks(*ops, extended=True)
        bound = ref.error_bound(*ops)
        ratio = float((np.abs(got - exact) / bound).max())
        print(f"blocks parity {form} L={L} M={M}: max error / bound = {ratio:.4f}  [{ran}]")
        worst = max(worst, ratio)
        assert ratio <= 1.0, (form, L, M, ratio)
    line = f"blocks parity {form}: largest error / bound over {len(CASES)} cases = {worst:.4f}"
    print(line)
    if os.environ.get("QS_BLOCKS_PARITY_OUT"):
        with open(os.environ["QS_BLOCKS_PARITY_OUT"], "a") as f:
            f.write(line + "\n")


@pytest.mark.parametrize("form", FORMS)
def test_agreement_with_the_full_transform(form):
    from quantum_systems_amd import kernels

    # every Mi = L: the block transform IS the full transform (other contraction order: the sum of the two bounds)
    L = 12
    rng = np.random.default_rng(7)
    u, C = rand(rng, form, "u", L, L, L, L), rand(rng, form, "C", L, L)
    Ct = C.conj().T
    full = host(kernels.transform_two_body(dev(u), dev(C)))
    blk = host(kernels.transform_two_body_blocks(dev(u), dev(Ct), dev(Ct), dev(C), dev(C)))
    assert np.all(np.abs(blk - full) <= 2 * ref.error_bound(u, Ct, Ct, C, C))

    # a block: the sliced full transform
    L, o = 20, 4
    u, C = rand(rng, form, "u", L, L, L, L), rand(rng, form, "C", L, L)
    Ct = C.conj().T
    full = host(kernels.transform_two_body(dev(u), dev(C)))
    ops = (u, Ct[:o], Ct[:o], C[:, o:], C[:, o:])
    blk = host(kernels.transform_two_body_blocks(*map(dev, ops)))
    assert "lead_contract_kernel" in last_dispatch()
    both = ref.error_bound(*ops) + ref.error_bound(u, Ct, Ct, C, C)[:o, :o, o:, o:]
    assert np.all(np.abs(blk - full[:o, :o, o:, o:]) <= both)


@pytest.mark.parametrize("form", FORMS)
def test_lead_contract_bits(form):
    from quantum_systems_amd import kernels

    rng = np.random.default_rng(11)
    m, L = 6, 55
    n = L**3
    A, B = dev(rand(rng, form, "C", m, L)), dev(rand(rng, form, "u", L, n))
    T = kernels.lead_contract(A, B)
    assert f"lead_contract_kernel<{FORMS.index(form)}, 8>" in last_dispatch()
    # (one inner product of length L: the block bound's gamma_(4L+8) covers it with room)
    ld = np.longdouble if form == "fp64" else np.clongdouble
    exact = host(A).astype(ld) @ host(B).astype(ld)
    bound = ref.gamma(4 * L + 8) * (np.abs(host(A)) @ np.abs(host(B))) * (1.0 if form == "fp64" else 2.0 * np.sqrt(2.0))
    assert np.all(np.abs(host(T) - exact) <= bound)
    # rows: row i of the 6-row call is the 1-row call on that row (other instantiation, same chain)
    for i in range(m):
        assert torch.equal(kernels.lead_contract(A[i:i + 1], B), T[i:i + 1]), i
    # columns: the first n' columns are the call on the contiguous copy, n' odd and even; then as a view (ldb > n')
    for n1 in (1, 2, 255, 256, 513, 3001, 3002, n - 1):
        compact = kernels.lead_contract(A, B[:, :n1].contiguous())
        assert torch.equal(compact, T[:, :n1]), n1
        assert torch.equal(kernels.lead_contract(A, B[:, :n1]), compact), n1
    # a base offset by 8 bytes (one real element; a complex tensor has 16-byte elements: one element)
    flat = torch.empty(L * n + 1, dtype=B.dtype, device=B.device)
    flat[1:] = B.reshape(-1)
    assert torch.equal(kernels.lead_contract(A, flat[1:].view(L, n)), T)
    # more rows than one instantiation: every row block against the 1-row call
    A32 = dev(rand(rng, form, "C", 32, L))
    small = B[:, :4097].contiguous()
    T32 = kernels.lead_contract(A32, small)
    for rows in (3, 4, 5, 8, 9, 16, 17, 31):
        assert torch.equal(kernels.lead_contract(A32[:rows], small), T32[:rows]), rows


@pytest.mark.parametrize("form", FORMS)
def test_padding_hygiene(form):
    from quantum_systems_amd import kernels

    # B is the narrow slice of a wider buffer whose surplus columns are NaN: with an odd n the last 16-byte item of
    # each row of a real B straddles into the surplus, and the select must drop that half
    rng = np.random.default_rng(13)
    m, k, n, ld = 5, 37, 333, 340
    A = dev(rand(rng, form, "C", m, k))
    wide = torch.full((k, ld), float("nan"), dtype=torch.complex128 if form == "complex128" else torch.float64, device="cuda")
    Bh = rand(rng, form, "u", k, n)
    wide[:, :n] = dev(Bh)
    got = kernels.lead_contract(A, wide[:, :n])
    assert bool(torch.isfinite(torch.view_as_real(got) if got.is_complex() else got).all())
    assert torch.equal(got, kernels.lead_contract(A, dev(Bh)))


def _spatial(l, n, complex_, seed):
    import quantum_systems_amd as qsa
    from quantum_systems_amd import hip

    h, u, s = ref.hermitian_problem(l, seed=seed, complex_=complex_)
    return qsa.construct_custom_system(n, l, hip.asarray(s), hip.asarray(h), hip.asarray(u), dim=2, np=hip,
                                       system_type="spatial", nuclear_repulsion_energy=0.25)


def _reference_mp2(system, C, eps, general):
    """(E2 of the NumPy restatement on the long-double block, the propagated tolerance) for the same C and eps."""
    from quantum_systems_amd.array_module import to_host

    u, C, eps = to_host(system.u), host(C), host(eps).real.astype(np.float64)
    n_occ = system.n           # occupied orbitals: a SpatialOrbitalSystem keeps half its particle number
    Co, Cv = C[:, :n_occ], C[:, n_occ:]
    ops = (u, Co.conj().T, Co.conj().T, Cv, Cv)
    g = ref.blocks(*ops, extended=True)
    delta = ref.error_bound(*ops)
    e2 = ref.mp2_general(g, eps, n_occ, system._basis_set._anti_symmetrized_u) if general else ref.mp2_spatial(g, eps, n_occ)
    return e2, ref.mp2_tolerance(g, delta, eps, n_occ), g


@pytest.mark.parametrize("complex_", [False, True])
def test_mp2_against_the_restatement_and_between_rhf_and_ghf(complex_):
    from quantum_systems_amd import HartreeFock, mp2_energy, hip

    l, n, tol = 10, 4, 1e-10
    system = _spatial(l, n, complex_, seed=210)
    hf = HartreeFock(system)
    with pytest.raises(RuntimeError, match="scf"):
        hf.mp2()
    C, eps, _ = hf.scf(tol=tol, max_iter=200)
    assert hf.converged
    e2 = hf.mp2()
    e2_ref, tol_rhf, g = _reference_mp2(system, C, eps, general=False)
    print(f"mp2 rhf complex={complex_}: {e2:.15e} ref {e2_ref:.15e} |diff| {abs(e2 - e2_ref):.2e} tolerance {tol_rhf:.2e}")
    assert abs(e2 - e2_ref) <= tol_rhf
    assert e2 < 0

    # GHF on the spin-doubled system, its own SCF, same C and eps on both sides
    gos = _spatial(l, n, complex_, seed=210).construct_general_orbital_system()
    ghf = HartreeFock(gos)
    Cg, eg, _ = ghf.scf(tol=tol, max_iter=200)
    e2g = ghf.mp2()
    e2g_ref, tol_ghf, _ = _reference_mp2(gos, Cg, eg, general=True)
    print(f"mp2 ghf complex={complex_}: {e2g:.15e} ref {e2g_ref:.15e} |diff| {abs(e2g - e2g_ref):.2e} tolerance {tol_ghf:.2e}")
    assert abs(e2g - e2g_ref) <= tol_ghf

    # RHF against GHF without a second SCF: the RHF orbitals spin-doubled (spin orbital 2 p + sigma)
    Cd = np.kron(host(C), np.eye(2))
    ed = np.repeat(host(eps).real, 2)
    e2d = mp2_energy(gos, hip.asarray(Cd), hip.asarray(ed))
    _, tol_d, _ = _reference_mp2(gos, Cd, ed, general=True)
    print(f"mp2 rhf vs spin-doubled complex={complex_}: {e2:.15e} {e2d:.15e} |diff| {abs(e2 - e2d):.2e} "
          f"tolerance {tol_rhf + tol_d:.2e}")
    assert abs(e2d - e2) <= tol_rhf + tol_d

    # canonical basis: after the change the blocks are slices of u and eps the Fock diagonal (SCF-limited agreement)
    hf.change_system_basis()
    with pytest.raises(RuntimeError, match="mp2_energy"):
        hf.mp2()
    e2c = mp2_energy(system)
    D = ref.denominators(host(eps).real.astype(np.float64), system.n)
    slack = 100 * tol * float((np.abs(g).astype(np.float64) ** 2 / D**2).sum()) + tol_rhf
    print(f"mp2 canonical complex={complex_}: {e2c:.15e} |diff| {abs(e2c - e2):.2e} tolerance {slack:.2e}")
    assert abs(e2c - e2) <= slack


def test_numpy_staging_path_and_sharded_refusal():
    import quantum_systems_amd as qsa

    l, n = 6, 2
    h, u, s = ref.hermitian_problem(l, seed=5, complex_=False)
    system = qsa.construct_custom_system(n, l, s, h, u, dim=2, np=np, system_type="spatial")
    rng = np.random.default_rng(2)
    C = rng.standard_normal((l, l))
    ops = (u, C.T[:1], C.T[:1], C[:, 1:], C[:, 1:])
    got = system.transform_two_body_blocks((ops[1], ops[2]), (ops[3], ops[4]))
    assert isinstance(got, np.ndarray) and got.shape == (1, 1, 5, 5)
    assert np.all(np.abs(got - ref.blocks(*ops, extended=True)) <= ref.error_bound(*ops))
    np.testing.assert_array_equal(np.asarray(system.u), u)           # the basis set is left as it is


@pytest.mark.parametrize("l,n", [(21, 2), (36, 6)])
def test_mp2_on_the_two_dimensional_dot(l, n):
    import quantum_systems_amd as qsa
    from quantum_systems_amd import HartreeFock, hip

    basis = qsa.TwoDimensionalHarmonicOscillator(l, 6.0, 41, omega=1.0, np=hip)
    system = qsa.SpatialOrbitalSystem(n, basis)
    hf = HartreeFock(system)
    _, _, energies = hf.scf(tol=1e-10, max_iter=200)
    assert hf.converged
    e2 = hf.mp2()
    line = f"mp2 2-D dot n={n} l={l}: E_HF = {energies[-1]:.10f}  E2 = {e2:.10f}  E_MP2 = {energies[-1] + e2:.10f}"
    print(line)
    if os.environ.get("QS_BLOCKS_PARITY_OUT"):
        with open(os.environ["QS_BLOCKS_PARITY_OUT"], "a") as f:
            f.write(line + "\n")
    assert e2 < 0 and abs(e2) < abs(energies[-1])
