"""The two byte movers of ``exchange_leading=2`` alone (``qs_exchange_pair_transpose``, ``qs_exchange_pair_transpose_back``),
bit for bit against a torch permutation: both dtypes, at sizes below one tile, one element past one tile and one past
two (the tile side is 32; the way back of fp64 takes 64 elements along d, so it also runs at L = 129 with few new
orbitals), and for the way back at L != M in both directions.

The destination is filled with a sentinel first: the half that is written must equal the permuted source and the other
half must still be the sentinel.  For the way back the source's lower pairs (d < c) are NaN: they are never read -- the
lower half of the result comes from the upper pairs, turned."""

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
DTYPES = [torch.float64, torch.complex128]
TILE = 32
SENTINEL = -7.25


def _rand(shape, dtype, seed):
    g = torch.Generator(device=DEV).manual_seed(seed)
    a = torch.randn(shape, dtype=torch.float64, device=DEV, generator=g)
    return torch.complex(a, torch.randn(shape, dtype=torch.float64, device=DEV, generator=g)) if dtype.is_complex else a


def _upper(n):
    """mask[i, j] = j >= i"""
    return torch.ones(n, n, dtype=torch.bool, device=DEV).triu()


@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "c128"])
@pytest.mark.parametrize("L", [5, TILE + 1, 2 * TILE + 1])
def test_way_in(L, dtype):
    from quantum_systems_amd import kernels as K

    src = _rand((L, L, L, L), dtype, seed=L)
    keep = src.clone()
    dst = torch.full((L, L, L, L), SENTINEL, dtype=dtype, device=DEV)
    K.dispatch_log = log = []
    try:
        assert K.exchange_pair_transpose(src, dst) is dst
    finally:
        K.dispatch_log = None
    assert len(log) == 1 and log[0].startswith("qs::exchange_pair_transpose_kernel<") and "transpose_back" not in log[0]
    assert torch.equal(src, keep)
    want = src.permute(2, 3, 0, 1)                                # want[c, d, a, b] = src[a, b, c, d]
    written = _upper(L)                                           # d >= c
    assert torch.equal(dst[written], want[written])
    assert torch.equal(dst[~written], torch.full_like(dst[~written], SENTINEL))


@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "c128"])
@pytest.mark.parametrize("L,M", [(5, 5), (TILE + 1, TILE + 1), (2 * TILE + 1, 2 * TILE + 1), (12, 20), (20, 12), (4 * TILE + 1, 12)])
def test_way_back(L, M, dtype):
    from quantum_systems_amd import kernels as K

    full = _rand((L, L, M, M), dtype, seed=100 * L + M)
    full = full + full.permute(1, 0, 3, 2)                        # full[c,d,p,q] == full[d,c,q,p]: what the stored half stands for
    src = full.clone()
    src[~_upper(L)] = float("nan")                                # the pairs d < c are not stored
    dst = torch.full((M, M, L, L), SENTINEL, dtype=dtype, device=DEV)
    K.dispatch_log = log = []
    try:
        assert K.exchange_pair_transpose_back(src, dst) is dst
    finally:
        K.dispatch_log = None
    assert len(log) == 1 and log[0].startswith("qs::exchange_pair_transpose_back_kernel<")
    want = full.permute(2, 3, 0, 1)                               # want[p, q, c, d] = full[c, d, p, q]
    written = _upper(M)                                           # q >= p
    assert not torch.isnan(torch.view_as_real(dst) if dtype.is_complex else dst).any()
    assert torch.equal(dst[written], want[written])
    assert torch.equal(dst[~written], torch.full_like(dst[~written], SENTINEL))


def test_wrappers_refuse_what_the_entries_cannot_take():
    from quantum_systems_amd import kernels as K

    a = torch.zeros((4, 4, 4, 4), dtype=torch.float64, device=DEV)
    with pytest.raises(ValueError):
        K.exchange_pair_transpose(a, torch.zeros((4, 4, 4, 5), dtype=torch.float64, device=DEV))
    with pytest.raises(ValueError):
        K.exchange_pair_transpose(a, a.to(torch.complex128))
    with pytest.raises(ValueError):
        K.exchange_pair_transpose_back(torch.zeros((4, 4, 6, 6), dtype=torch.float64, device=DEV), a)
    with pytest.raises(ValueError):
        K.exchange_pair_transpose(a, a)                           # QS_ERR_ALIAS
