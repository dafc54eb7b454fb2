"""CPU-only checks of the pair-contraction entry (``qs_pair_contract`` / ``_workspace``): the symbols, every refused
argument (no GPU is touched: the checks run before any HIP call), the workspace query, and the tuning key."""

import pytest

F64, C128 = 0, 1
FORMS = {"fp64": (F64, F64), "complex128": (C128, C128), "mixed": (F64, C128)}


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as entry

    entry.build()
    from quantum_systems_amd import _lib

    return _lib.load()


def test_symbols_are_exported_and_bound(lib):
    import ctypes

    from quantum_systems_amd import _lib

    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name in ("qs_pair_contract", "qs_pair_contract_workspace"):
        assert hasattr(raw, name) and name in _lib.SIGNATURES
    assert lib.qs_abi_version() == 4


@pytest.mark.parametrize("form", list(FORMS))
def test_workspace_is_linear_in_k_or_zero(lib, form):
    u_dtype, t_dtype = FORMS[form]
    q = lib.qs_pair_contract_workspace
    for X, Y in [(1, 1), (9, 9), (15, 63), (3025, 3025), (65536, 65536), (7, 1 << 24), (1 << 32, 5)]:
        one = q(u_dtype, t_dtype, X, Y, 1)
        assert one >= 0, (X, Y)
        for K in (1, 2, 7, 8, 9, 33, 65536):
            assert q(u_dtype, t_dtype, X, Y, K) == K * one, (X, Y, K)
    assert q(C128, F64, 8, 8, 2) == -6 and q(7, F64, 8, 8, 2) == -6 and q(F64, -1, 8, 8, 2) == -6
    assert q(u_dtype, t_dtype, 0, 8, 2) == -1 and q(u_dtype, t_dtype, 8, 0, 2) == -1
    assert q(u_dtype, t_dtype, 8, 8, 0) == -1 and q(u_dtype, t_dtype, -8, 8, 2) == -1
    assert q(u_dtype, t_dtype, 8, (1 << 24) + 1, 2) == -1 and q(u_dtype, t_dtype, 8, 8, 65537) == -1


def test_refused_arguments_without_gpu(lib):
    # fake, well-separated device addresses: every call below returns before any HIP call is made
    U, T, S, work = 1 << 40, 2 << 40, 3 << 40, 4 << 40
    X, Y, K = 9, 15, 3
    need = lib.qs_pair_contract_workspace(F64, F64, X, Y, K)

    def call(u_dtype=F64, t_dtype=F64, U=U, T=T, S=S, X=X, Y=Y, K=K, ldu=Y, work=work, n=need):
        return lib.qs_pair_contract(u_dtype, t_dtype, U, T, S, X, Y, K, ldu, work, n, None)

    assert call(U=None) == -2 and call(T=None) == -2 and call(S=None) == -2
    assert call(X=0) == -1 and call(X=-1) == -1 and call(Y=0) == -1 and call(K=0) == -1 and call(K=-2) == -1
    assert call(ldu=Y - 1) == -1 and call(ldu=0) == -1 and call(ldu=(1 << 24) + 1) == -1
    assert call(u_dtype=C128, t_dtype=F64) == -6 and call(u_dtype=3) == -6 and call(t_dtype=-1) == -6
    assert call(u_dtype=3, U=None) == -6 and call(X=0, U=None) == -1          # order: dtype pair, extents, null
    assert call(U=U + 4) == -3 and call(T=T + 4) == -3 and call(S=S + 4) == -3
    assert call(u_dtype=C128, t_dtype=C128, U=U + 8) == -3                    # a complex element is 16 bytes
    assert call(t_dtype=C128, T=T + 8) == -3 and call(t_dtype=C128, S=S + 8) == -3
    assert call(n=need - 1) == -4                                             # short workspace
    assert call(S=U) == -7 and call(S=T) == -7
    assert call(S=U + 8 * ((X - 1) * Y + Y - 1)) == -7                        # S starts inside U's last row
    assert call(S=U + 8 * ((X - 1) * 17 + Y - 1), ldu=17) == -7               # ... of a wider slab
    assert call(S=U - 8) == -7                                                # S reaches into U
    assert call(S=T + 8 * (K * Y - 1)) == -7 and call(S=T - 8 * K * X + 8) == -7
    assert call(S=U, n=need - 1) == -7                                        # alias is reported before the size


def test_tuning_key_accepts_group_sizes_only(lib):
    from quantum_systems_amd import kernels

    try:
        for good in (0, 1, 2, 4, 8):
            assert lib.qs_tuning_set(b"pair_contract_g", good) == 0
        for bad in (-1, 3, 5, 6, 7, 9, 16, 1 << 40):
            assert lib.qs_tuning_set(b"pair_contract_g", bad) == -1
    finally:
        lib.qs_tuning_reset()
    with kernels.tuning(pair_contract_g=2):
        pass
    with pytest.raises(Exception):
        with kernels.tuning(pair_contract_g=3):
            pass


def test_wrapper_is_gpu_only():
    import torch

    from quantum_systems_amd import kernels

    with pytest.raises(RuntimeError, match="GPU only"):
        kernels.pair_contract(torch.zeros(3, 3, 3, 3, dtype=torch.float64), torch.zeros(2, 3, 3, dtype=torch.float64))
