"""CPU-only checks of the block-transform entries (``qs_lead_contract``, ``qs_transform_two_body_blocks`` and its
workspace query): the workspace formula the header documents, every refused argument (no GPU is touched: the checks run
before any HIP call), the ABI version, the new tuning key, and the CPU restatement's own consistency."""

import numpy as np
import pytest

import _blocks_ref as ref

F64, C128 = 0, 1
PAIRS = [(F64, F64), (C128, C128), (F64, C128)]


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as entry

    entry.build()
    from quantum_systems_amd import _lib

    return _lib.load()


def documented_workspace(c_dtype, L, M0, M1, M2, M3):
    """include/qs_amd.h: Le(L (M0 + M2)) + M0 L^3 + M0 M1 L^2 elements of the result dtype."""
    even = lambda x: (x + 1) // 2 * 2  # noqa: E731
    return (even(L * (M0 + M2)) + M0 * L**3 + M0 * M1 * L**2) * (16 if c_dtype == C128 else 8)


@pytest.mark.parametrize("u_dtype,c_dtype", PAIRS)
def test_workspace_is_the_documented_formula(lib, u_dtype, c_dtype):
    for L, M in [(1, (1, 1, 1, 1)), (5, (1, 1, 4, 4)), (20, (3, 3, 17, 17)), (33, (10, 10, 23, 23)), (55, (6, 6, 49, 49)),
                 (24, (24, 2, 5, 7)), (40, (33, 4, 4, 4)), (256, (6, 6, 250, 250)), (256, (256, 256, 256, 256)),
                 (1024, (3, 5, 7, 1024)), (4096, (1, 1, 1, 1))]:
        got = lib.qs_transform_two_body_blocks_workspace(u_dtype, c_dtype, L, *M)
        assert got == documented_workspace(c_dtype, L, *M), (L, M)
        # within the issue's budget: the three intermediates plus the two small coefficient scratches
        M0, M1, M2, M3 = M
        es = 16 if c_dtype == C128 else 8
        assert got <= (M0 * L**3 + M0 * M1 * L**2 + M0 * M1 * L * M3 + L * (M0 + M2) + 1) * es
    q = lib.qs_transform_two_body_blocks_workspace
    assert q(C128, F64, 8, 2, 2, 2, 2) == -6 and q(7, F64, 8, 2, 2, 2, 2) == -6 and q(F64, -1, 8, 2, 2, 2, 2) == -6
    assert q(u_dtype, c_dtype, 0, 1, 1, 1, 1) == -1 and q(u_dtype, c_dtype, 4097, 1, 1, 1, 1) == -1
    for pos in range(4):
        for bad in (0, 9, -2):
            M = [2, 2, 2, 2]
            M[pos] = bad
            assert q(u_dtype, c_dtype, 8, *M) == -1, (pos, bad)


def test_blocks_refused_arguments_without_gpu(lib):
    # fake, well-separated device addresses: every call below returns before any HIP call is made
    u, c0, c1, c2, c3, out, work = (k << 40 for k in range(1, 8))
    L, M = 8, (2, 3, 4, 5)
    need = lib.qs_transform_two_body_blocks_workspace(F64, F64, L, *M)

    def call(u_dtype=F64, c_dtype=F64, u=u, c0=c0, c1=c1, c2=c2, c3=c3, out=out, work=work, nbytes=need, L=L, M=M):
        return lib.qs_transform_two_body_blocks(u_dtype, c_dtype, u, c0, c1, c2, c3, out, work, nbytes, L, *M, None)

    for name in ("u", "c0", "c1", "c2", "c3", "out", "work"):
        assert call(**{name: None}) == -2, name
    assert call(L=0) == -1 and call(L=-3) == -1 and call(L=4097) == -1
    assert call(M=(0, 3, 4, 5)) == -1 and call(M=(2, 9, 4, 5)) == -1 and call(M=(2, 3, 0, 5)) == -1
    assert call(M=(2, 3, 4, 9)) == -1
    assert call(u_dtype=C128, c_dtype=F64) == -6 and call(u_dtype=3) == -6 and call(c_dtype=-1) == -6
    assert call(nbytes=need - 1) == -4
    for name, base in (("u", u), ("c0", c0), ("c1", c1), ("c2", c2), ("c3", c3), ("out", out)):
        assert call(**{name: base + 4}) == -3, name
    assert call(work=work + 8) == -3
    assert call(u_dtype=C128, c_dtype=C128, u=u + 8, nbytes=2 * need) == -3         # complex operands: 16 bytes
    assert call(u_dtype=F64, c_dtype=C128, c0=c0 + 8, nbytes=2 * need) == -3
    assert call(u_dtype=F64, c_dtype=C128, u=u + 8, nbytes=2 * need - 1) == -4      # (a real u needs 8 bytes only)
    assert call(out=u) == -7 and call(out=work) == -7 and call(out=c0) == -7 and call(out=c3) == -7
    assert call(out=u + 8 * (L**4 - 1)) == -7              # out starts inside u
    assert call(out=work - 8) == -7                        # out reaches into the workspace
    assert call(work=u + 16) == -7                         # the workspace inside u


def test_lead_contract_refused_arguments_without_gpu(lib):
    A, B, T = 1 << 40, 2 << 40, 3 << 40

    def call(a_dtype=F64, b_dtype=F64, A=A, B=B, T=T, m=6, n=125, k=5, lda=5, ldb=125, ldt=125):
        return lib.qs_lead_contract(a_dtype, b_dtype, A, B, T, m, n, k, lda, ldb, ldt, None)

    assert call(A=None) == -2 and call(B=None) == -2 and call(T=None) == -2
    assert call(m=0) == -1 and call(m=33) == -1 and call(n=0) == -1 and call(k=0) == -1
    assert call(lda=4) == -1 and call(ldb=124) == -1 and call(ldt=124) == -1
    assert call(a_dtype=F64, b_dtype=C128) == -6 and call(a_dtype=2) == -6 and call(b_dtype=-1) == -6
    assert call(A=A + 4) == -3 and call(B=B + 4) == -3 and call(T=T + 4) == -3
    assert call(a_dtype=C128, b_dtype=C128, B=B + 8) == -3 and call(a_dtype=C128, T=T + 8) == -3
    assert call(T=A) == -7 and call(T=B) == -7 and call(T=B + 8 * (5 * 125 - 1)) == -7 and call(T=A - 8) == -7


def test_abi_version_binding_and_tuning_key(lib):
    from quantum_systems_amd import _lib, kernels

    for name in ("qs_lead_contract", "qs_transform_two_body_blocks", "qs_transform_two_body_blocks_workspace"):
        assert name in _lib.SIGNATURES
    assert lib.qs_abi_version() == 4
    try:
        assert lib.qs_tuning_set(b"lead_rows_max", 33) == -1
        assert lib.qs_tuning_set(b"lead_rows_max", -1) == -1
        assert lib.qs_tuning_set(b"lead_rows_max", 0) == 0 and lib.qs_tuning_set(b"lead_rows_max", 32) == 0
    finally:
        lib.qs_tuning_reset()
    import torch

    z = torch.zeros
    with pytest.raises(RuntimeError, match="GPU only"):
        kernels.transform_two_body_blocks(z(3, 3, 3, 3, dtype=torch.float64), z(1, 3, dtype=torch.float64),
                                          z(1, 3, dtype=torch.float64), z(3, 2, dtype=torch.float64),
                                          z(3, 2, dtype=torch.float64))
    with pytest.raises(RuntimeError, match="GPU only"):
        kernels.lead_contract(z(2, 3, dtype=torch.float64), z(3, 5, dtype=torch.float64))


def test_restatement_agrees_with_the_one_matrix_transform_and_with_itself():
    from oracle import qs_oracle as orc

    rng = np.random.default_rng(3)
    L = 6
    u = rng.standard_normal((L, L, L, L)) + 1j * rng.standard_normal((L, L, L, L))
    C = rng.standard_normal((L, L)) + 1j * rng.standard_normal((L, L))
    Ct = C.conj().T
    full = orc.transform_two_body(u, C)
    np.testing.assert_allclose(ref.blocks(u, Ct, Ct, C, C), full, rtol=1e-11, atol=1e-11)
    blk = ref.blocks(u, Ct[:2], Ct[1:3], C[:, 2:], C[:, 3:5])
    np.testing.assert_allclose(blk, full[:2, 1:3, 2:, 3:5], rtol=1e-11, atol=1e-11)
    exact = ref.blocks(u, Ct[:2], Ct[1:3], C[:, 2:], C[:, 3:5], extended=True)
    assert np.all(np.abs(blk - exact) <= ref.error_bound(u, Ct[:2], Ct[1:3], C[:, 2:], C[:, 3:5]))


def test_mp2_restatements_agree_between_spatial_and_spin_orbitals():
    # a closed-shell block spin-doubled (index 2 p + sigma) gives the same energy from the spin-orbital formula
    rng = np.random.default_rng(4)
    o, v = 2, 3
    l = o + v
    w = rng.standard_normal((l, l, l, l))
    w = w + w.transpose(1, 0, 3, 2)
    eps = np.sort(rng.standard_normal(l)) + np.arange(l)
    g = w[:o, :o, o:, o:]
    e_rhf = ref.mp2_spatial(g, eps, o)
    d = np.eye(2)
    ws = np.einsum("pqrs,ac,bd->paqbrcsd", w, d, d).reshape(2 * l, 2 * l, 2 * l, 2 * l)
    eps2 = np.repeat(eps, 2)
    gs = ws[: 2 * o, : 2 * o, 2 * o:, 2 * o:]
    assert abs(ref.mp2_general(gs, eps2, 2 * o, False) - e_rhf) <= 1e-12 * abs(e_rhf)
    ga = gs - gs.transpose(0, 1, 3, 2)
    assert abs(ref.mp2_general(ga, eps2, 2 * o, True) - e_rhf) <= 1e-12 * abs(e_rhf)
    assert e_rhf < 0
    assert ref.mp2_tolerance(g, np.zeros_like(g), eps, o) < 1e-12 * abs(e_rhf)
