"""The exchange route's d and c contractions as one triangular-batch launch each (``exchange_pairs=1``, the default)
against the launches per block of rows and per row (``exchange_pairs=0``): c is the same kernel on the same tiles; d
may tile differently (L rows per pair against (L - a0) L flat rows per block), and every tiled form sums along k in the
same order -- so the results are ``torch.equal``; both within the project's 1e-10 * max|ref| of the NumPy oracle.

Run with ``exchange=2`` and with the strip, stream, skinny and fitted routes off, square and rectangular, blocks that do
not divide the size, both dtypes, out of place and in place.  At L = M = 128 the dispatch holds exactly one product
launch for d and one for c -- five product launches in all (d, c, a and the closing product's two blocks of 64 rows),
every one an exact form of the fast product kernel.  At that size the result is bounded against the plain route, as
tests/test_gpu_exchange_route.py does it (a NumPy oracle of 128^4 elements would be gigabytes on the host), and that
route against the oracle at the small sizes.  A non-symmetric tensor still takes the plain route, bit for bit."""

import numpy as np
import pytest
import torch

from oracle import qs_oracle as orc

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BOUND = 1e-10
DTYPES = [torch.float64, torch.complex128]
OTHER_ROUTES_OFF = dict(gemm_strip=0, gemm_stream=0, gemm_skinny=0, gemm_fit=0)


def _inputs(L, M, dtype, seed, symmetric=True):
    rng = np.random.default_rng(seed)

    def rand(*shape):
        a = rng.standard_normal(shape)
        return a + 1j * rng.standard_normal(shape) if dtype.is_complex else a

    u = rand(L, L, L, L)
    if symmetric:
        u = u + u.transpose(1, 0, 3, 2)
    return np.ascontiguousarray(u), rand(L, M), rand(M, L)


def _name(kernel, dtype):
    return f"qs::{kernel}<{'f64x2' if dtype.is_complex else 'double'}>"


def _launches(dispatch):
    """[(kernel name, launches)] of a dispatch record ("name xN" stands for N launches in a row)."""
    out = []
    for item in dispatch.split(";"):
        name, sep, count = item.rpartition(" x")
        out.append((name, int(count)) if sep and count.isdigit() else (item, 1))
    return out


def _route(K, u, C, Ct, pairs, block, inplace=False):
    with K.tuning(**OTHER_ROUTES_OFF, exchange=2, exchange_block=block, exchange_pairs=pairs):
        got = K.transform_two_body_(u.clone(), C, Ct) if inplace else K.transform_two_body(u, C, Ct)
        return got, K.last_dispatch()


@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "c128"])
@pytest.mark.parametrize("L,M,block", [(24, 24, 8), (33, 33, 8), (20, 12, 8), (12, 20, 8)])
def test_pairs_launches_give_the_bits_of_the_row_launches(L, M, block, dtype):
    from quantum_systems_amd import kernels as K

    u_h, C_h, Ct_h = _inputs(L, M, dtype, seed=L * 100 + M)
    ref = orc.transform_two_body(u_h, C_h, Ct_h)
    scale = np.abs(ref).max()
    u, C, Ct = (torch.from_numpy(x).to(DEV) for x in (u_h, C_h, Ct_h))
    keep = u.clone()
    rows, rows_dispatch = _route(K, u, C, Ct, 0, block)
    got, dispatch = _route(K, u, C, Ct, 1, block)
    assert torch.equal(u, keep)
    mirror = _name("exchange_transpose_kernel", dtype)
    assert mirror in dispatch.split(";") and mirror in rows_dispatch.split(";")
    products = lambda d: sum(n for name, n in _launches(d) if "transpose" not in name)     # noqa: E731
    # c is one launch in place of L; d at most as many as before
    assert products(dispatch) <= products(rows_dispatch) - (L - 1), (dispatch, rows_dispatch)
    assert torch.equal(got, rows), "exchange_pairs=1 differs from exchange_pairs=0"
    err = np.abs(got.cpu().numpy() - ref).max() / scale
    print(f"exchange pairs route L={L} M={M} block={block} {dtype}: vs oracle {err:.2e}; {dispatch}")
    assert err <= BOUND
    if M <= L:
        inplace, inplace_dispatch = _route(K, u, C, Ct, 1, block, inplace=True)
        assert inplace_dispatch == dispatch
        assert torch.equal(inplace, got)
        assert torch.equal(_route(K, u, C, Ct, 0, block, inplace=True)[0], got)


@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "c128"])
def test_one_launch_each_for_d_and_c_at_128(dtype):
    from quantum_systems_amd import kernels as K

    L = 128
    g = torch.Generator(device=DEV).manual_seed(11)

    def rand(*shape):
        a = torch.randn(shape, dtype=torch.float64, device=DEV, generator=g)
        return torch.complex(a, torch.randn(shape, dtype=torch.float64, device=DEV, generator=g)) if dtype.is_complex else a

    u = rand(L, L, L, L)
    for a in range(L):                                     # symmetrise slab by slab (x + y is exactly commutative)
        s = u[a, a:] + u[a:, a].transpose(1, 2)
        u[a, a:] = s
        u[a:, a] = s.transpose(1, 2)
    C, Ct = rand(L, L) / L**0.5, rand(L, L) / L**0.5
    assert K.two_body_exchange_symmetric(u)
    with K.tuning(exchange=0):
        plain = K.transform_two_body(u, C, Ct)
    rows, rows_dispatch = _route(K, u, C, Ct, 0, 64)
    got, dispatch = _route(K, u, C, Ct, 1, 64)
    assert torch.equal(got, rows), "exchange_pairs=1 differs from exchange_pairs=0"
    scale = plain.abs().max().item()
    err = (got - plain).abs().max().item() / scale
    print(f"exchange pairs route L=M=128 block=64 {dtype}: vs plain route {err:.2e}; {dispatch}")
    assert err <= BOUND                                    # (the plain route is within 1e-10 of the oracle: test_gpu_exchange_route.py)
    if dtype.is_complex:
        exact = {"qs::gemm_fast_kernel<true, 4, 2, true, false>", "qs::gemm_fast_kernel<true, 2, 4, true, false>"}
    else:
        exact = {"qs::gemm_fast_kernel<false, 4, 4, true, false>", "qs::gemm_fast_kernel<false, 2, 4, true, false>"}
    mirror = _name("exchange_transpose_kernel", dtype)
    launches = _launches(dispatch)
    prods = [(name, n) for name, n in launches if name != mirror]
    assert all(name in exact for name, _ in prods), dispatch
    assert sum(n for _, n in prods) == 5, dispatch                      # d, c, a, and the closing product's two blocks
    # the order: d and c (one launch each), the mirror of T2, a, the closing blocks, the mirror of the result
    kinds = [name == mirror for name, n in launches for _ in range(n)]
    assert kinds == [False, False, True, False, False, False, True], dispatch
    inplace, inplace_dispatch = _route(K, u, C, Ct, 1, 64, inplace=True)
    assert inplace_dispatch == dispatch and torch.equal(inplace, got)


@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "c128"])
def test_non_symmetric_input_keeps_the_plain_route(dtype):
    from quantum_systems_amd import kernels as K

    u_h, C_h, Ct_h = _inputs(24, 24, dtype, seed=3, symmetric=False)
    u, C, Ct = (torch.from_numpy(x).to(DEV) for x in (u_h, C_h, Ct_h))
    with K.tuning(**OTHER_ROUTES_OFF, exchange=0):
        plain = K.transform_two_body(u, C, Ct)
        plain_dispatch = K.last_dispatch()
    for pairs in (0, 1):
        got, dispatch = _route(K, u, C, Ct, pairs, 8)
        assert dispatch == plain_dispatch and "transpose" not in dispatch
        assert torch.equal(got, plain)
