"""The transform's route for a tensor with particle-exchange symmetry (qs_api.hip), forced at small sizes with
``K.tuning(exchange=2, exchange_block=b)``: against the NumPy oracle and against the plain route, both within the
project's bound 1e-10 * max|ref| (measured on MI355X: 2.4e-16 ... 8.7e-16 against either, 1.3e-15 / 2.3e-15 at 128;
each case prints its figures), with general C and C_tilde that are not adjoints, square and rectangular, blocks that do
not divide the size.

Also: a non-symmetric tensor under the same knobs is the plain route bit for bit, and at L = M = 128 -- the smallest
size whose strided launches reach the exact forms of the fast product kernel -- the dispatch names only those."""

import numpy as np
import pytest
import torch

from oracle import qs_oracle as orc

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BOUND = 1e-10
DTYPES = [torch.float64, torch.complex128]


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


@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "c128"])
@pytest.mark.parametrize("L,M,block", [(24, 24, 8), (40, 40, 16), (33, 33, 8), (20, 12, 8), (12, 20, 8)])
def test_route_against_oracle_and_plain_route(L, M, block, dtype):
    from quantum_systems_amd import kernels as K

    u_h, C_h, Ct_h = _inputs(L, M, dtype, seed=L * 100 + M)
    ref = orc.transform_two_body(u_h, C_h, Ct_h)
    scale = np.abs(ref).max()
    u, C, Ct = (torch.from_numpy(x).to(DEV) for x in (u_h, C_h, Ct_h))
    keep = u.clone()
    with K.tuning(exchange=0):
        plain = K.transform_two_body(u, C, Ct)
        assert "transpose" not in K.last_dispatch()
    K.dispatch_log = log = []
    try:
        with K.tuning(exchange=2, exchange_block=block):
            got = K.transform_two_body(u, C, Ct)
            dispatch = K.last_dispatch()
    finally:
        K.dispatch_log = None
    assert torch.equal(u, keep)                                    # u untouched
    assert log[0] == _name("exchange_transpose_check_kernel", dtype) and log[1] == dispatch and len(log) == 2
    assert _name("exchange_transpose_kernel", dtype) in dispatch.split(";")
    err_ref = np.abs(got.cpu().numpy() - ref).max() / scale
    err_plain = (got - plain).abs().max().item() / scale
    print(f"exchange route L={L} M={M} block={block} {dtype}: vs oracle {err_ref:.2e}, vs plain route {err_plain:.2e}")
    assert err_ref <= BOUND and err_plain <= BOUND
    # the mirrored blocks are copies: out[p,q,r,s] == out[q,p,s,r] bit for bit for p, q in different blocks
    blk = torch.arange(M, device=DEV) // block
    apart = blk[:, None] != blk[None, :]
    assert torch.equal(got[apart], got.permute(1, 0, 3, 2)[apart])
    if M <= L:
        with K.tuning(exchange=2, exchange_block=block):
            inplace = K.transform_two_body_(u.clone(), C, Ct)
            assert _name("exchange_transpose_kernel", dtype) in K.last_dispatch().split(";")
        assert torch.equal(inplace, got)


@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "c128"])
def test_non_symmetric_input_takes_the_plain_route(dtype):
    from quantum_systems_amd import kernels as K

    u_h, C_h, Ct_h = _inputs(24, 24, dtype, seed=3, symmetric=False)
    u, C, Ct = (torch.from_numpy(x).to(DEV) for x in (u_h, C_h, Ct_h))
    with K.tuning(exchange=0):
        plain = K.transform_two_body(u, C, Ct)
        plain_dispatch = K.last_dispatch()
    K.dispatch_log = log = []
    try:
        with K.tuning(exchange=2, exchange_block=8):
            got = K.transform_two_body(u, C, Ct)
            assert K.last_dispatch() == plain_dispatch
            off = K.transform_two_body(u, C, Ct, exchange=False)      # the keyword skips the check too
    finally:
        K.dispatch_log = None
    assert log == [_name("exchange_transpose_check_kernel", dtype), plain_dispatch, plain_dispatch]
    assert torch.equal(got, plain) and torch.equal(off, plain)
    # a real tensor against complex coefficients keeps the plain (mixed) route, symmetric or not
    if not dtype.is_complex:
        us = u + u.permute(1, 0, 3, 2)
        Cc = torch.complex(C, C.flip(0))
        with K.tuning(exchange=0):
            want = K.transform_two_body(us, Cc)
            mixed_dispatch = K.last_dispatch()
        with K.tuning(exchange=2):
            assert torch.equal(K.transform_two_body(us, Cc), want) and K.last_dispatch() == mixed_dispatch


@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "c128"])
def test_fast_kernel_size_takes_only_exact_forms(dtype):
    """L = M = 128, block 64: d on (128 - a0) * 128 rows, c per a on 128 x 128, the closing product on 128 and 64 rows."""
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
        plain_dispatch = K.last_dispatch()
        assert "transpose" not in plain_dispatch
    assert torch.equal(K.transform_two_body(u, C, Ct), plain) and K.last_dispatch() == plain_dispatch    # automatic: never at 128
    with K.tuning(exchange=2, exchange_block=64):
        got = K.transform_two_body(u, C, Ct)
        dispatch = K.last_dispatch()
    names = {item.rpartition(" x")[0] if " x" in item else item for item in dispatch.split(";")}
    if dtype.is_complex:
        exact = {"qs::gemm_fast_kernel<true, 4, 2, true, false>", "qs::gemm_fast_kernel<true, 2, 4, true, false>"}
    else:
        exact = {"qs::gemm_fast_kernel<false, 4, 4, true, false>", "qs::gemm_fast_kernel<false, 2, 4, true, false>"}
    assert names <= exact | {_name("exchange_transpose_kernel", dtype)}, dispatch
    assert _name("exchange_transpose_kernel", dtype) in names and names & exact
    scale = plain.abs().max().item()
    err = (got - plain).abs().max().item() / scale
    print(f"exchange route L=M=128 block=64 {dtype}: vs plain route {err:.2e}")
    assert err <= BOUND
    assert torch.equal(got[:64, 64:], got.permute(1, 0, 3, 2)[:64, 64:])

