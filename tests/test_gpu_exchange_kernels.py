"""The two bandwidth kernels of the exchange-symmetry route (qs_permute.hip) on their own.

Check kernel (``kernels.two_body_exchange_symmetric``): bit patterns of u[a,b,c,d] against u[b,a,d,c] at sizes below,
at and above the 32-element tile edge.  Mirror kernel (``kernels.exchange_mirror_``): t[a,b,r,s] = t[b,a,s,r] below the
block diagonal, everything else bit-identical, with ragged last blocks, a block larger than n and block = 1."""

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
DTYPES = [torch.float64, torch.complex128]


def _symmetric(l, dtype, seed=0):
    g = torch.Generator(device=DEV).manual_seed(seed)
    u = torch.randn((l, l, l, l), dtype=torch.float64, device=DEV, generator=g)
    if dtype.is_complex:
        u = torch.complex(u, torch.randn((l, l, l, l), dtype=torch.float64, device=DEV, generator=g))
    u = u + u.permute(1, 0, 3, 2)              # x + y is commutative in IEEE arithmetic: exactly symmetric
    return u.contiguous()


def _flip_low_bit(u, idx):
    """Flip the lowest mantissa bit of (the real part of) u[idx]."""
    words = torch.view_as_real(u)[..., 0] if u.is_complex() else u
    bits = words.view(torch.int64)
    bits[idx] ^= 1


@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "c128"])
@pytest.mark.parametrize("l", [5, 31, 32, 33])
def test_check_kernel(l, dtype):
    from quantum_systems_amd import kernels as K

    u = _symmetric(l, dtype, seed=l)
    assert torch.equal(u, u.permute(1, 0, 3, 2))
    assert K.two_body_exchange_symmetric(u) is True
    assert K.last_dispatch() == f"qs::exchange_transpose_check_kernel<{'f64x2' if dtype.is_complex else 'double'}>"
    last = l - 1
    for idx in [(1, 3, 2, 4), (last, 0, last, 1),          # off-diagonal pairs
                (2, 2, 1, 3), (last, last, 0, last),       # u[a,a] must be a symmetric matrix
                (last, last, last, last - 1), (0, 1, 0, 0)]:
        v = u.clone()
        _flip_low_bit(v, idx)
        assert K.two_body_exchange_symmetric(v) is False, idx
    v = u.clone()                                          # the very last element pairs with itself: flipping it alone keeps
    _flip_low_bit(v, (last, last, last, last))             # the symmetry, flipping its neighbour in the last row does not
    assert K.two_body_exchange_symmetric(v) is True
    if dtype.is_complex:                                   # the imaginary part is compared too
        v = u.clone()
        torch.view_as_real(v)[..., 1].view(torch.int64)[(3, 1, 0, 2)] ^= 1
        assert K.two_body_exchange_symmetric(v) is False
    # -0.0 against +0.0: equal values, different bits
    v = u.clone()
    v[1, 2, 3, 4] = 0.0
    v[2, 1, 4, 3] = 0.0
    assert K.two_body_exchange_symmetric(v) is True
    v[2, 1, 4, 3] = -0.0
    assert torch.equal(v, v.permute(1, 0, 3, 2))           # torch compares values
    assert K.two_body_exchange_symmetric(v) is False
    # identical NaNs on both sides: same bits
    v = u.clone()
    v[0, 4, 1, 2] = float("nan")
    v[4, 0, 2, 1] = float("nan")
    v[3, 3, 2, 2] = float("nan")
    assert K.two_body_exchange_symmetric(v) is True
    assert torch.equal(v, u) is False


def test_check_on_a_capturing_stream_launches_nothing_and_says_no():
    from quantum_systems_amd import kernels as K

    u = _symmetric(8, torch.float64)
    assert K.two_body_exchange_symmetric(u) is True
    K.workspace.get(1 << 12, u.device)                     # no allocation inside the capture
    side = torch.cuda.Stream(device=DEV)
    side.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        verdict = K.two_body_exchange_symmetric(u)
        dispatch = K.last_dispatch()
    assert verdict is False and dispatch == ""


@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "c128"])
@pytest.mark.parametrize("n,m,block", [(20, 12, 8), (8, 33, 1), (16, 32, 8), (7, 31, 16), (12, 20, 4)])
def test_mirror_kernel(n, m, block, dtype):
    from quantum_systems_amd import kernels as K

    g = torch.Generator(device=DEV).manual_seed(n * 100 + m)
    t = torch.randn((n, n, m, m), dtype=torch.float64, device=DEV, generator=g)
    if dtype.is_complex:
        t = torch.complex(t, torch.randn((n, n, m, m), dtype=torch.float64, device=DEV, generator=g))
    blk = torch.arange(n, device=DEV) // block
    lower = blk[:, None] > blk[None, :]                    # (a, b) with a // block > b // block
    t[lower] = float("nan")
    before = t.clone()
    got = K.exchange_mirror_(t, block)
    assert got is t
    if lower.any():
        assert K.last_dispatch() == f"qs::exchange_transpose_kernel<{'f64x2' if dtype.is_complex else 'double'}>"
    else:
        assert K.last_dispatch() == ""                     # one block row: nothing to write, nothing launched
    want = before.permute(1, 0, 3, 2)
    assert torch.equal(t[lower], want[lower])
    assert not torch.isnan(torch.view_as_real(t) if dtype.is_complex else t).any()
    assert torch.equal(t[~lower], before[~lower])          # (no NaN up there: torch.equal is a bit test on these values)
