"""CPU-only checks of the exchange-symmetric pair-contraction entry (``qs_pair_contract_exchange`` / ``_workspace``): the
symbols, every refused argument in the order of ``qs_pair_contract_antisym`` (no GPU is touched: the checks run before
any HIP call), the workspace query, and the Python layer's refusals."""

import pytest

F64, C128 = 0, 1


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
    for name in ("qs_pair_contract_exchange", "qs_pair_contract_exchange_workspace"):
        assert hasattr(raw, name) and name in _lib.SIGNATURES
    assert lib.qs_abi_version() == 4                      # an added entry: the version of the existing ones stays


def test_workspace_is_zero_and_refuses_bad_arguments(lib):
    q = lib.qs_pair_contract_exchange_workspace
    for dt in (F64, C128):
        for l in (1, 2, 3, 17, 110, 4096):
            for K in (1, 8, 9, 65536):
                assert q(dt, dt, l, K) == 0, (dt, l, K)
        assert q(dt, dt, 0, 2) == -1 and q(dt, dt, -3, 2) == -1 and q(dt, dt, 4097, 2) == -1
        assert q(dt, dt, 8, 0) == -1 and q(dt, dt, 8, -1) == -1 and q(dt, dt, 8, 65537) == -1
    # no kernel form for a real U against complex T (the Python layer splits T), nor the other way round
    assert q(F64, C128, 8, 2) == -6 and q(C128, F64, 8, 2) == -6 and q(7, F64, 8, 2) == -6 and q(F64, -1, 8, 2) == -6
    assert q(7, 7, 0, 2) == -6                            # order: dtype pair, then extents


def test_refused_arguments_without_gpu(lib):
    # fake, well-separated device addresses: every call below returns before any HIP call is made
    U, T, S, work = 1 << 40, 2 << 40, 3 << 40, 4 << 40
    l, K = 5, 3

    def call(u_dtype=F64, t_dtype=F64, U=U, T=T, S=S, l=l, K=K, ldu=l * l, work=work, n=0):
        return lib.qs_pair_contract_exchange(u_dtype, t_dtype, U, T, S, l, K, ldu, work, n, None)

    assert call(U=None) == -2 and call(T=None) == -2 and call(S=None) == -2
    assert call(l=0, ldu=0) == -1 and call(l=-2) == -1 and call(K=0) == -1 and call(K=-2) == -1 and call(K=65537) == -1
    assert call(ldu=l * l - 1) == -1 and call(ldu=0) == -1 and call(ldu=(1 << 24) + 1) == -1
    assert call(l=4097, ldu=4097 * 4097) == -1
    assert call(u_dtype=F64, t_dtype=C128) == -6 and call(u_dtype=C128, t_dtype=F64) == -6
    assert call(u_dtype=3) == -6 and call(t_dtype=-1) == -6
    assert call(u_dtype=3, U=None) == -6 and call(l=0, ldu=0, U=None) == -1   # order: dtype pair, extents, null
    assert call(U=None, T=T + 4) == -2                                        # ... null before alignment
    assert call(U=U + 4) == -3 and call(T=T + 4) == -3 and call(S=S + 4) == -3
    assert call(u_dtype=C128, t_dtype=C128, U=U + 8) == -3                    # a complex element is 16 bytes
    assert call(u_dtype=C128, t_dtype=C128, T=T + 8) == -3 and call(u_dtype=C128, t_dtype=C128, S=S + 8) == -3
    assert call(S=S + 4, n=-1) == -3                                          # alignment before alias and size
    assert call(n=-1) == -4                                                   # short workspace
    assert call(S=U) == -7 and call(S=T) == -7
    assert call(S=U + 8 * (l ** 4 - 1)) == -7                                 # S starts at U's last element
    assert call(S=U + 8 * ((l * l - 1) * 28 + l * l - 1), ldu=28) == -7       # ... of a padded tensor
    assert call(S=U - 8) == -7                                                # S reaches into U
    assert call(S=T + 8 * (K * l * l - 1)) == -7 and call(S=T - 8 * K * l * l + 8) == -7
    assert call(S=U, n=-1) == -7                                              # alias is reported before the size


def test_wrapper_refusals_without_gpu():
    import numpy as np
    import torch

    import quantum_systems_amd as qsa
    from quantum_systems_amd import kernels

    with pytest.raises(RuntimeError, match="GPU only"):
        kernels.pair_contract_exchange(torch.zeros(3, 3, 3, 3, dtype=torch.float64), torch.zeros(2, 3, 3, dtype=torch.float64))
    for shape in ((3, 3, 3, 4), (0, 0, 0, 0), (3, 3, 3)):
        with pytest.raises(ValueError):
            kernels.pair_contract_exchange(torch.zeros(shape, dtype=torch.float64), torch.zeros(3, 3, dtype=torch.float64))
    with pytest.raises(TypeError):
        kernels.pair_contract_exchange([[0.0]], torch.zeros(3, 3, dtype=torch.float64))
    # the system method takes one of its two flags, and RCCD a closed shell only
    np.random.seed(3)
    spatial = qsa.SpatialOrbitalSystem(2, qsa.RandomBasisSet(4, 2))
    with pytest.raises(ValueError, match="one of them"):
        spatial.contract_two_body_pairs(np.zeros((4, 4)), antisymmetric=True, exchange=True)
    general = object.__new__(qsa.GeneralOrbitalSystem)        # the type alone is looked at (building one needs a GPU)
    with pytest.raises(TypeError, match="coupled_cluster.CCD"):
        qsa.RCCD(general)
    with pytest.raises(TypeError, match="SpatialOrbitalSystem"):
        qsa.RCCD(None)
    with pytest.raises(ValueError, match="ladder"):
        qsa.RCCD(spatial, ladder="antisym")
    with pytest.raises(ValueError, match="both C and epsilon"):
        qsa.RCCD(spatial, np.eye(4))
    with pytest.raises(ValueError, match="occupied"):
        qsa.RCCD(qsa.SpatialOrbitalSystem(8, qsa.RandomBasisSet(4, 2)))
    with pytest.raises(AssertionError):
        qsa.SpatialOrbitalSystem(3, qsa.RandomBasisSet(4, 2))                 # an odd particle number never reaches RCCD
