"""CPU-only checks of the mean-field entry (``qs_mean_field`` / ``qs_mean_field_workspace``): the workspace formula
the header documents, every refused argument (no GPU is touched: the checks run before any HIP call), the launch
geometry of every L <= 1024 as ``qs_mean_field_plan`` reports it, the census of geometry classes against the case table
of the GPU tests (tests/_mean_field_cases.py), and the pin of the TESTS' oracle (tests/_mean_field_ref.py) to reference-generated numbers
(tests/golden/fock_energy_random_basis.npz)."""

import numpy as np
import pytest

import _mean_field_cases as cases
import _mean_field_ref as ref

F64, C128 = 0, 1
# cases per form in tests/_mean_field_cases.py: the classes do not capture everything the table was chosen for (chunk
# lengths up to 10, the benchmark sizes), so a case that leaves the table has to be taken out here as well
CASES_PER_FORM = {"fp64": 43, "complex128": 44, "mixed": 43}


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as entry

    entry.build()
    from quantum_systems_amd import _lib

    return _lib.load()


def documented_chunks(L, R, d_dtype):
    """include/qs_amd.h: Rc = min(ceil(R / min(ceil(4096 / L), R)), max(1, floor(2048 / (Le * dw))))."""
    cdiv = lambda a, b: -(-a // b)  # noqa: E731
    Le, dw = (L + 1) // 2 * 2, (2 if d_dtype == C128 else 1)
    Rc = min(cdiv(R, min(cdiv(4096, L), R)), max(1, 2048 // (Le * dw)))
    return cdiv(R, Rc)


@pytest.mark.parametrize("u_dtype,d_dtype", [(F64, F64), (C128, C128), (F64, C128)])
def test_workspace_is_rows_times_chunks(lib, u_dtype, d_dtype):
    es = 16 if d_dtype == C128 else 8
    for L, P, R in [(1, 1, 1), (5, 5, 5), (5, 2, 5), (31, 31, 7), (64, 64, 64), (96, 17, 96), (256, 256, 256),
                    (256, 32, 256), (256, 256, 32), (1024, 3, 1024)]:
        got = lib.qs_mean_field_workspace(u_dtype, d_dtype, L, P, R)
        assert got == P * L * documented_chunks(L, R, d_dtype) * es, (L, P, R)
        assert got == P * lib.qs_mean_field_workspace(u_dtype, d_dtype, L, 1, R)        # linear in P
    assert lib.qs_mean_field_workspace(C128, F64, 8, 8, 8) == -6
    assert lib.qs_mean_field_workspace(7, F64, 8, 8, 8) == -6
    assert lib.qs_mean_field_workspace(u_dtype, d_dtype, 0, 1, 1) == -1
    assert lib.qs_mean_field_workspace(u_dtype, d_dtype, 8, 9, 8) == -1
    assert lib.qs_mean_field_workspace(u_dtype, d_dtype, 8, 8, 9) == -1
    assert lib.qs_mean_field_workspace(u_dtype, d_dtype, 8, 8, 0) == -1


def test_refused_arguments_without_gpu(lib):
    # fake, well-separated device addresses: every call below returns before any HIP call is made
    u, D, W, work = 1 << 40, 2 << 40, 3 << 40, 4 << 40
    L, P, R = 8, 8, 8
    need = lib.qs_mean_field_workspace(F64, F64, L, P, R)

    def call(u_dtype=F64, d_dtype=F64, u=u, D=D, W=W, L=L, P=P, R=R, r_lo=0, work=work, nbytes=need):
        return lib.qs_mean_field(u_dtype, d_dtype, u, D, W, L, P, R, r_lo, 1.0, -0.5, work, nbytes, None)

    assert call(u=None) == -2 and call(D=None) == -2 and call(W=None) == -2 and call(work=None) == -2
    assert call(L=0) == -1 and call(L=-3) == -1
    assert call(P=0) == -1 and call(P=9) == -1 and call(R=0) == -1
    assert call(R=4, r_lo=5) == -1                       # r_lo + R > L
    assert call(R=4, r_lo=-1) == -1
    assert call(u_dtype=C128, d_dtype=F64) == -6         # complex u with a real D
    assert call(u_dtype=3) == -6 and call(d_dtype=-1) == -6
    assert call(nbytes=need - 1) == -4
    assert call(u=u + 4) == -3 and call(D=D + 4) == -3 and call(W=W + 4) == -3 and call(work=work + 8) == -3
    assert call(u_dtype=C128, d_dtype=C128, u=u + 8, nbytes=2 * need) == -3     # complex operands: 16 bytes
    assert call(W=u) == -7 and call(W=D) == -7 and call(W=work) == -7
    assert call(W=u + 8 * (P * R * L * L - 1)) == -7     # W starts inside u
    assert call(W=D - 8) == -7                           # W reaches into D


def test_error_strings_and_binding(lib):
    from quantum_systems_amd import _lib, kernels

    assert "qs_mean_field" in _lib.SIGNATURES and "qs_mean_field_workspace" in _lib.SIGNATURES
    assert lib.qs_abi_version() == 4
    import torch

    with pytest.raises(RuntimeError, match="GPU only"):
        kernels.mean_field(torch.zeros(3, 3, 3, 3, dtype=torch.float64), torch.zeros(3, 3, dtype=torch.float64))


def test_restatement_reproduces_reference_values(golden):
    # the numbers of the reference's own system classes, from formula (1) with the reference-determinant density
    from oracle import qs_oracle as orc

    g = golden("fock_energy_random_basis")
    l, n, e_nuc = int(g["l"]), int(g["n"]) // 2, float(g["e_nuc"])
    h, u = g["h"], g["u"]
    rho = ref.reference_density(l, n, 2.0)
    tol = dict(rtol=1e-11, atol=1e-11)               # the tolerance of tests/test_gpu_fock_energy.py
    np.testing.assert_allclose(ref.fock_from_density(h, u, rho, 1.0, -0.5), g["spas_fock"], **tol)
    np.testing.assert_allclose(ref.energy_from_density(h, u, rho, 1.0, -0.5, e_nuc), g["spas_energy"], **tol)

    C = g["C"]
    h_cb, u_cb = orc.transform_one_body(h, C), orc.transform_two_body(u, C)
    np.testing.assert_allclose(ref.fock_from_density(h_cb, u_cb, rho, 1.0, -0.5), g["spas_cb_fock"], **tol)
    np.testing.assert_allclose(ref.energy_from_density(h_cb, u_cb, rho, 1.0, -0.5, e_nuc), g["spas_cb_energy"], **tol)

    # spin orbitals: anti-symmetrised u carries the exchange (cj = 1, ck = 0); a plain u needs ck = -1
    h_gos = orc.add_spin_one_body(h).astype(np.complex128)
    u_plain = orc.add_spin_two_body(u)
    u_gos = orc.anti_symmetrize_u(u_plain)
    rho_gos = ref.reference_density(2 * l, 2 * n, 1.0)
    np.testing.assert_allclose(h_gos, g["gos_h"], **tol)
    np.testing.assert_allclose(ref.fock_from_density(h_gos, u_gos, rho_gos, 1.0, 0.0), g["gos_fock"], **tol)
    np.testing.assert_allclose(ref.fock_from_density(h_gos, u_plain, rho_gos, 1.0, -1.0), g["gos_fock"], **tol)
    np.testing.assert_allclose(ref.energy_from_density(h_gos, u_gos, rho_gos, 1.0, 0.0, e_nuc), g["gos_energy"], **tol)
    C2 = g["C_gos"]
    h2, u2 = orc.transform_one_body(h_gos, C2), orc.transform_two_body(u_gos, C2)
    np.testing.assert_allclose(ref.fock_from_density(h2, u2, rho_gos, 1.0, 0.0), g["gos_cb_fock"], **tol)
    np.testing.assert_allclose(ref.energy_from_density(h2, u2, rho_gos, 1.0, 0.0, e_nuc), g["gos_cb_energy"], **tol)

    # the second closed-shell case, rectangular change of basis 10 -> 8
    bl, bn = int(g["b_l"]), int(g["b_n"]) // 2
    Cb = g["b_C"]
    hb, ub = orc.transform_one_body(g["b_h"], Cb), orc.transform_two_body(g["b_u"], Cb)
    rho_b = ref.reference_density(Cb.shape[1], bn, 2.0)
    np.testing.assert_allclose(ref.fock_from_density(hb, ub, rho_b, 1.0, -0.5), g["b_cb_fock"], **tol)
    np.testing.assert_allclose(ref.energy_from_density(hb, ub, rho_b, 1.0, -0.5, float(g["b_e_nuc"])),
                               g["b_cb_energy"], **tol)
    assert bl == 10


def test_plain_scf_helper_lowers_the_core_guess_energy():
    h, u, s = ref.hermitian_problem(6, seed=5)
    e, e0, its = ref.plain_scf(h, u, s, 2, 2.0, 1.0, -0.5)
    assert e <= e0 + 1e-12 and its > 1


def plan_of(lib, form, L, P, R):
    import ctypes

    u_dtype, d_dtype = cases.FORMS[form][:2]
    out = (ctypes.c_int64 * 7)()
    assert lib.qs_mean_field_plan(u_dtype, d_dtype, L, P, R, ctypes.cast(out, ctypes.c_void_p), 7) == 0, (form, L, P, R)
    return tuple(out)


def plan_Rs(L):
    return sorted({min(L, max(1, R)) for R in (1, 2, L // 3 + 1, L - 1, L)})


@pytest.mark.parametrize("form", list(cases.FORMS))
def test_plan_of_every_size(lib, form):
    u_dtype, d_dtype, cpi, dw = cases.FORMS[form]
    es = 8 * dw
    for L in range(1, 1025):
        Le = (L + 1) // 2 * 2
        tiles = set()
        for R in plan_Rs(L):
            plan = plan_of(lib, form, L, 1, R)
            Rc, nchunk, ct_log, ncb, nrb, lds_bytes, grid = plan
            where = (form, L, R, plan)
            CT = 1 << ct_log
            RT = 256 // CT
            RB, WPR = 8 * RT, max(1, CT // 64)
            assert 8 <= CT <= 128, where
            assert ncb * CT * cpi >= L > (ncb - 1) * CT * cpi, where
            assert nrb * RB >= L > (nrb - 1) * RB, where
            assert Rc >= 1 and nchunk == cases.cdiv(R, Rc), where
            assert Rc * Le * dw <= 2048 or Rc == 1, where
            # Dc [Rc][Le], Jl [nrb * RB], Kl [ncb * CT * cpi], redJ [RB][WPR], redK [256][cpi], dw doubles each
            carved = 8 * dw * (Rc * Le + nrb * RB + ncb * CT * cpi + RB * WPR + 256 * cpi)
            assert lds_bytes == carved <= 65536, where
            assert grid == nchunk, where
            assert nchunk == documented_chunks(L, R, d_dtype), where
            for P in sorted({1, 2, L // 2 + 1, L} & set(range(1, L + 1))):
                other = plan_of(lib, form, L, P, R)
                assert other[:6] == plan[:6] and other[6] == P * nchunk, (where, P)       # nothing but the grid sees P
                assert lib.qs_mean_field_workspace(u_dtype, d_dtype, L, P, R) == P * L * nchunk * es, (where, P)
            tiles.add(cases.tile_class(plan, L))
        assert len(tiles) == 1, (form, L, tiles)            # the tile geometry does not depend on R


def census(lib, form):
    """{tile class: [L, ...]} and the set of chunk classes over L = 1 ... 1024, from the library's own plans."""
    tiles, chunks = {}, set()
    for L in range(1, 1025):
        for R in plan_Rs(L):
            plan = plan_of(lib, form, L, 1, R)
            chunks.add(cases.chunk_class(plan, L, R))
        tiles.setdefault(cases.tile_class(plan, L), []).append(L)
    return tiles, chunks


@pytest.mark.parametrize("form", list(cases.FORMS))
def test_case_table_covers_every_geometry_class(lib, form):
    mine = [c for c in cases.CASES if c[0] == form]
    assert len(mine) == CASES_PER_FORM[form] and len(set(mine)) == len(mine)
    assert {c[0] for c in cases.CASES} == set(cases.FORMS) and len(cases.CASES) == sum(CASES_PER_FORM.values())
    for _, L, P, p_lo, R, r_lo in mine:
        assert 1 <= L <= 1024 and P in (1, 2, 3) and P * R * L * L <= cases.MAX_ELEMENTS, (form, L, P, R)
        assert 0 <= p_lo and p_lo + P <= L and 0 <= r_lo and 1 <= R and r_lo + R <= L, (form, L, P, p_lo, R, r_lo)
        assert p_lo > 0 or P == L, (form, L, P)
    assert 2 * sum(c[5] > 0 for c in mine) >= len(mine)
    plans = {c: plan_of(lib, form, c[1], c[2], c[4]) for c in mine}

    tiles, chunks = census(lib, form)
    print(f"{form}: {len(tiles)} tile classes, {len(chunks)} chunk classes, {len(mine)} cases")
    assert {L for Ls in tiles.values() for L in Ls} == set(range(1, 1025))
    sizes = {c[1] for c in mine}
    for key, Ls in tiles.items():
        assert min(Ls) in sizes and max(Ls) in sizes, (form, key, min(Ls), max(Ls))
    assert {1023, 1024} <= sizes
    assert chunks <= {cases.chunk_class(plans[c], c[1], c[4]) for c in mine}, form

    # more than one column block: at both ends of the class's window a case with Rc > 1 and a short last chunk where
    # the size cap leaves one at that L (a complex D above L = 512 has room for one column only: then R >= 3)
    for key, Ls in tiles.items():
        if not key[1]:
            continue
        for L in (min(Ls), max(Ls)):
            here = [c for c in mine if c[1] == L]
            if any(plans[c][0] > 1 and c[4] % plans[c][0] for c in here):
                continue
            for R in range(1, min(L, cases.MAX_ELEMENTS // (L * L)) + 1):
                Rc = plan_of(lib, form, L, 1, R)[0]
                assert not (Rc > 1 and R % Rc), (form, key, L, "no case with a short last chunk, but one exists: R =", R)
            assert any(c[4] >= 3 for c in here), (form, key, L)


def test_plan_hook_refuses_what_the_workspace_query_refuses(lib):
    import ctypes

    out = (ctypes.c_int64 * 8)(*([-99] * 8))
    ptr = ctypes.cast(out, ctypes.c_void_p)
    for args in [(C128, F64, 8, 8, 8), (7, F64, 8, 8, 8), (F64, -1, 8, 8, 8), (F64, F64, 0, 1, 1), (F64, F64, 1025, 1, 1),
                 (F64, F64, 8, 9, 8), (F64, F64, 8, 0, 8), (F64, C128, 8, 8, 9), (C128, C128, 8, 8, 0)]:
        refused = lib.qs_mean_field_workspace(*args)
        assert refused < 0 and lib.qs_mean_field_plan(*args, ptr, 7) == refused, args
    assert lib.qs_mean_field_plan(F64, F64, 8, 8, 8, ptr, 6) == -1           # short n_out
    assert lib.qs_mean_field_plan(F64, F64, 8, 8, 8, ptr, 0) == -1
    assert lib.qs_mean_field_plan(F64, F64, 8, 8, 8, None, 7) == -2
    assert list(out) == [-99] * 8                                             # a refused call writes nothing
    assert lib.qs_mean_field_plan(F64, F64, 8, 8, 8, ptr, 8) == 0
    assert out[7] == -99 and all(x > 0 for x in out[:7])                      # seven values, no more
