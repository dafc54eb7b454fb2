"""``kernels.mean_field`` (qs_mean_field.hip) on the GPU: parity against the CPU restatement (tests/_mean_field_ref.py)
under a bound that holds for ANY summation order, the bit-level properties the C ABI promises, the system-level
methods against the reference-generated golden values, and the SCF driver.

Parity bound (derived, not tuned): an element of W is a sum of n = 2 R L products; every summation order satisfies
|W - W_exact| <= gamma_(n+2) * A with gamma_k = k eps / (1 - k eps), eps = 2^-53, A = the formula on |u|, |D|, |cj|,
|ck| (complex results: a further factor 2 sqrt 2); W_exact is the numpy.longdouble evaluation.  The largest observed
error / bound per dtype form is printed and, when QS_MEAN_FIELD_PARITY_OUT names a file, written there.

The sizes here stop at L = 96; the launch geometries above that (more than one column block, CT = 8, two live waves per
tile row, capped chunk lengths) are run by tests/test_gpu_mean_field_geometry.py."""

import os

import numpy as np
import pytest
import torch

import _mean_field_ref as ref

pytestmark = pytest.mark.gpu
TOL = dict(rtol=1e-11, atol=1e-11)                       # tests/test_gpu_fock_energy.py
SIZES = [1, 2, 5, 8, 16, 31, 55, 64, 65, 96]
WEIGHTS = [(1.0, 0.0), (1.0, -0.5), (1.0, -1.0), (0.0, 1.0)]
FORMS = ["fp64", "complex128", "mixed"]


def H(x):
    return torch.as_tensor(x).cpu().numpy() if not isinstance(x, (complex, float, np.ndarray, np.generic)) else x


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def operands(form, L, seed):
    rng = np.random.default_rng(seed)
    u = rng.standard_normal((L, L, L, L))
    D = rng.standard_normal((L, L))
    if form == "complex128":
        u = u + 1j * rng.standard_normal((L, L, L, L))
    if form != "fp64":
        D = D + 1j * rng.standard_normal((L, L))
    return u, D


def slabs(u, L):
    """(name, slab (P, R, L, L), p_lo, r_lo): the whole tensor, rows with P < L, a second-index slab with r_lo > 0
    (for L = 1 neither exists: the whole tensor three times)."""
    p_lo, P = L // 4, max(1, L // 3)
    r_lo = L // 3 if L > 2 else L - 1
    return [("full", u, 0, 0), ("rows", u[p_lo:p_lo + P], p_lo, 0),
            ("second", np.ascontiguousarray(u[:, r_lo:]), 0, r_lo)]


@pytest.mark.parametrize("form", FORMS)
def test_parity_within_the_summation_bound(form):
    from quantum_systems_amd import kernels

    worst = 0.0
    for L in SIZES:
        u, D = operands(form, L, 1000 + L)
        d_D = dev(D)
        for name, slab, _, r_lo in slabs(u, L):
            J, K = ref.jk(slab, D, r_lo, extended=True)
            aJ, aK = ref.jk(np.abs(slab), np.abs(D), r_lo)
            n = 2 * slab.shape[1] * L
            scale = ref.gamma(n + 2) * (1.0 if form == "fp64" else 2.0 * np.sqrt(2.0))
            d_slab = dev(slab)
            for cj, ck in WEIGHTS:
                W = kernels.mean_field(d_slab, d_D, cj=cj, ck=ck, r_lo=r_lo)
                assert W.dtype == (torch.float64 if form == "fp64" else torch.complex128)
                assert tuple(W.shape) == (slab.shape[0], L)
                err = np.abs(W.cpu().numpy().astype(J.dtype) - (cj * J + ck * K)).astype(np.float64)
                bound = scale * (abs(cj) * aJ + abs(ck) * aK)
                ratio = float((err / bound).max())
                worst = max(worst, ratio)
                assert ratio <= 1.0, (form, L, name, cj, ck, ratio)
            del d_slab
    line = f"{form}: largest |W - W_exact| / bound = {worst:.3e}"
    print(line)
    path = os.environ.get("QS_MEAN_FIELD_PARITY_OUT")
    if path:
        with open(path, "a") as fh:
            fh.write(line + "\n")


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("L", [5, 31, 64, 65])
def test_bit_level_properties(form, L):
    from quantum_systems_amd import kernels

    u, D = operands(form, L, 7 + L)
    d_u, d_D = dev(u), dev(D)
    for cj, ck in [(1.0, -0.5), (0.0, 1.0), (1.0, 0.0)]:
        full = kernels.mean_field(d_u, d_D, cj=cj, ck=ck)
        again = kernels.mean_field(d_u, d_D, cj=cj, ck=ck)
        assert torch.equal(full.view(torch.float64).view(torch.int64), again.view(torch.float64).view(torch.int64))
        # rows of a P < L call: the same bits as those rows of the full call
        for p_lo, P in [(0, 1), (L // 4, max(1, L // 3)), (L - 2, 2)]:
            rows = kernels.mean_field(d_u[p_lo:p_lo + P], d_D, cj=cj, ck=ck)
            assert torch.equal(rows.view(torch.float64).view(torch.int64),
                               full[p_lo:p_lo + P].contiguous().view(torch.float64).view(torch.int64)), (p_lo, P)
        # second-index slabs [0, R1) + [R1, L): partial sums add up within the bound (the outer sum is re-associated)
        R1 = L // 3 + 1
        a = kernels.mean_field(d_u[:, :R1].contiguous(), d_D, cj=cj, ck=ck, r_lo=0)
        b = kernels.mean_field(d_u[:, R1:].contiguous(), d_D, cj=cj, ck=ck, r_lo=R1)
        exact = ref.mean_field(u, D, cj, ck, extended=True)
        err = np.abs((a + b).cpu().numpy().astype(exact.dtype) - exact).astype(np.float64)
        assert (err <= ref.error_bound(u, D, cj, ck, extra_terms=1)).all()
        out = torch.empty_like(full)
        assert kernels.mean_field(d_u, d_D, cj=cj, ck=ck, out=out) is out
        assert torch.equal(out.view(torch.float64), full.view(torch.float64))


@pytest.mark.parametrize("form", FORMS)
def test_no_leakage_across_rows_and_padding_contributes_nothing(form):
    from quantum_systems_amd import kernels

    L, p0 = 31, 7
    u, D = operands(form, L, 99)
    clean = kernels.mean_field(dev(u), dev(D), cj=1.0, ck=-0.5)
    bad = u.copy()
    bad[p0, 3, 30, 30] = np.nan          # last element of an odd row: its 16-byte item straddles the next row
    bad[p0, L - 1, L - 1, L - 1] = np.inf
    bad[p0, 0, 0, 0] = -np.inf
    got = kernels.mean_field(dev(bad), dev(D), cj=1.0, ck=-0.5)
    keep = [p for p in range(L) if p != p0]
    assert torch.equal(got[keep].view(torch.float64), clean[keep].view(torch.float64))
    assert not torch.isfinite(got[p0].abs()).all()
    # odd L, constant u, D = 1: every element of W is (cj + ck) c L^2 exactly -- padding lanes add nothing
    for L in (1, 5, 31, 65):
        c = 0.5
        cu = np.full((L, L, L, L), c) if form != "complex128" else np.full((L, L, L, L), c + 0.25j)
        cD = np.ones((L, L)) if form == "fp64" else np.ones((L, L)) * (1.0 + 0j)
        W = kernels.mean_field(dev(cu), dev(cD), cj=1.0, ck=-0.5).cpu().numpy()
        assert (W == 0.5 * cu[0, 0, 0, 0] * L * L).all(), (form, L)


def test_wrapper_validates_its_arguments():
    from quantum_systems_amd import kernels

    u = torch.zeros(4, 4, 4, 4, dtype=torch.float64, device="cuda")
    D = torch.zeros(4, 4, dtype=torch.float64, device="cuda")
    with pytest.raises(ValueError):
        kernels.mean_field(u, D[:3])
    with pytest.raises(ValueError):
        kernels.mean_field(u[:, :2].contiguous(), D, r_lo=3)
    with pytest.raises(ValueError):
        kernels.mean_field(u, D, out=torch.empty(4, 4, dtype=torch.complex128, device="cuda"))
    kernels.mean_field(u, D, cj=1.0, ck=-0.5)
    assert kernels.last_dispatch().count("qs::mean_field_kernel<0, true, true>") == 1
    kernels.mean_field(u, D.to(torch.complex128), cj=0.0, ck=1.0)
    assert "qs::mean_field_kernel<2, false, true>" in kernels.last_dispatch()


def _spatial(g, mod, prefix=""):
    import quantum_systems_amd as qsa

    l, n = int(g[prefix + "l"]), int(g[prefix + "n"])
    s = g["s"] if not prefix else np.eye(l, dtype=np.complex128)
    return qsa.construct_custom_system(
        n, l, mod.asarray(s), mod.asarray(g[prefix + "h"]), mod.asarray(g[prefix + "u"]), dim=2, np=mod,
        system_type="spatial", nuclear_repulsion_energy=float(g[prefix + "e_nuc"]))


def _rho(system, mod, occupation):
    return mod.asarray(ref.reference_density(system.l, system.n, occupation))


@pytest.mark.parametrize("which", ["hip", "numpy"])
def test_system_methods_match_reference_values(golden, which):
    from quantum_systems_amd import hip

    mod = hip if which == "hip" else np
    g = golden("fock_energy_random_basis")
    spas = _spatial(g, mod)

    def check(system, occupation, fock, energy):
        rho = _rho(system, mod, occupation)
        np.testing.assert_allclose(H(system.construct_fock_matrix_from_density(rho)), g[fock], **TOL)
        np.testing.assert_allclose(complex(H(system.compute_energy_from_density(rho))), g[energy], **TOL)
        f = mod.zeros_like(system.h) + 1
        assert system.construct_fock_matrix_from_density(rho, h=system.h, u=system.u, f=f) is f
        np.testing.assert_allclose(H(f), g[fock], **TOL)
        # and the existing einsum forms agree with the one-pass kernel on the same system
        np.testing.assert_allclose(H(system.construct_fock_matrix(system.h, system.u)), H(f), **TOL)

    check(spas, 2.0, "spas_fock", "spas_energy")
    gos = spas.construct_general_orbital_system()
    check(gos, 1.0, "gos_fock", "gos_energy")
    plain = spas.construct_general_orbital_system(anti_symmetrize=False)    # ck = -1 on the plain spin tensor
    np.testing.assert_allclose(H(plain.construct_fock_matrix_from_density(_rho(plain, mod, 1.0))), g["gos_fock"], **TOL)
    spas.change_basis(mod.asarray(g["C"]))
    check(spas, 2.0, "spas_cb_fock", "spas_cb_energy")
    gos.change_basis(mod.asarray(g["C_gos"]))
    check(gos, 1.0, "gos_cb_fock", "gos_cb_energy")
    sb = _spatial(g, mod, "b_")
    sb.change_basis(mod.asarray(g["b_C"]))
    check(sb, 2.0, "b_cb_fock", "b_cb_energy")
    with pytest.raises(NotImplementedError):
        spas.change_to_hf_basis()


@pytest.mark.parametrize("world", [1, 2, 3])
@pytest.mark.parametrize("axis", [0, 1])
def test_sharded_forms_per_emulated_rank(golden, world, axis):
    # what sharded_basis.mean_field runs on each rank's ShardedTensor4.rows, every emulated rank on this one GPU:
    # rows concatenated (leading index sharded) or partial sums added (second index sharded)
    from quantum_systems_amd import hip, sharded

    g = golden("fock_energy_random_basis")
    spas = _spatial(g, hip)
    gos = spas.construct_general_orbital_system()
    spas.change_basis(hip.asarray(g["C"]))
    gos.change_basis(hip.asarray(g["C_gos"]))
    for system, occupation, f_ref in ((spas, 2.0, g["spas_cb_fock"]), (gos, 1.0, g["gos_cb_fock"])):
        h, u = torch.as_tensor(system.h), torch.as_tensor(system.u)
        rho = torch.as_tensor(_rho(system, hip, occupation))
        cj, ck = system._mean_field_weights()
        parts = []
        for rank in range(world):
            lo, hi = sharded.SlabPartition(system.l, world).bounds(rank)
            rows = (u[lo:hi] if axis == 0 else u[:, lo:hi].transpose(0, 1)).contiguous()
            parts.append(sharded.mean_field_local(rows, rho, cj, ck, lo, axis))
        W = torch.cat(parts) if axis == 0 else sum(parts)
        np.testing.assert_allclose((h + W).cpu().numpy(), f_ref, **TOL)
        np.testing.assert_allclose((h + W).cpu().numpy(), H(system.construct_fock_matrix_from_density(rho)), **TOL)


def _check_scf(system, occupation, tol=1e-10):
    """Converges; the basis it returns makes the system's own Fock matrix diagonal with the returned orbital energies;
    the energies agree with the system's own and with the independent plain SCF."""
    from quantum_systems_amd import HartreeFock, kernels
    from quantum_systems_amd.array_module import to_host

    h, u, s = to_host(system.h), to_host(system.u), to_host(system.s)
    cj, ck = system._mean_field_weights()
    e_ref, e_core, _ = ref.plain_scf(h, u, s, system.n, occupation, cj, ck, system.nuclear_repulsion_energy, tol=tol)

    hf = HartreeFock(system)
    kernels.dispatch_log = []
    try:
        C, eps, energies = hf.scf(tol=tol, max_iter=200)
        log = list(kernels.dispatch_log)
    finally:
        kernels.dispatch_log = None
    assert hf.converged and len(energies) == hf.iterations
    # every iteration's O(l^4) work is ONE launch of the one-pass kernel (plus its closing launch)
    assert sum(entry.count("qs::mean_field_kernel") for entry in log) == hf.iterations
    assert all("gemm" not in entry and "mean_field_kernel" in entry for entry in log)
    assert energies[-1] <= energies[0] + 1e-12                    # not above the core-guess determinant's
    np.testing.assert_allclose(energies[0], e_core, rtol=1e-10, atol=1e-10)
    # two SCF runs stopped at the same commutator tolerance: the energy is stationary, its error is second order
    np.testing.assert_allclose(energies[-1], e_ref, rtol=0, atol=1e-9)

    hf.change_system_basis()
    f = H(system.construct_fock_matrix(system.h, system.u))
    eps = H(eps)
    # the occupied space moves by <= tol / gap when the last Fock matrix is diagonalised, the Fock matrix by that times
    # |u| l: a factor 100 covers gap >= 0.1 and |u| l <= 10, which holds for these problems
    slack = 100 * tol
    o, v = system.o, system.v
    assert np.abs(f[o, v]).max() <= slack and np.abs(f[v, o]).max() <= slack
    assert np.abs(f - np.diag(eps)).max() <= slack
    np.testing.assert_allclose(complex(H(system.compute_reference_energy())).real, energies[-1], rtol=0, atol=1e-9)
    np.testing.assert_allclose(H(system.s), np.eye(system.l), atol=1e-10)
    return energies[-1]


@pytest.mark.parametrize("l,n", [(8, 4), (12, 6)])
def test_hartree_fock_on_a_seeded_hermitian_problem(l, n):
    import quantum_systems_amd as qsa
    from quantum_systems_amd import hip

    h, u, s = ref.hermitian_problem(l, seed=100 + l)

    def spatial():
        return qsa.construct_custom_system(n, l, hip.asarray(s), hip.asarray(h), hip.asarray(u), dim=2, np=hip,
                                           system_type="spatial", nuclear_repulsion_energy=0.25)

    e_rhf = _check_scf(spatial(), 2.0)
    e_ghf = _check_scf(spatial().construct_general_orbital_system(), 1.0)      # GHF from the same guess: the RHF solution
    np.testing.assert_allclose(e_ghf, e_rhf, rtol=0, atol=1e-8)


@pytest.mark.parametrize("l,n", [(15, 2), (28, 6)])
def test_hartree_fock_on_the_two_dimensional_dot(l, n):
    import quantum_systems_amd as qsa
    from quantum_systems_amd import hip

    basis = qsa.TwoDimensionalHarmonicOscillator(l, 6.0, 41, omega=1.0, np=hip)
    system = qsa.SpatialOrbitalSystem(n, basis)
    _check_scf(system, 2.0)
    with pytest.raises(NotImplementedError):
        system.change_to_hf_basis()
