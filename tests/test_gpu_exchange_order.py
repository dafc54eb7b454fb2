"""The exchange route with the leading indices contracted first (``exchange_order=2``: a, the closing blocks b, then d
and c on the pairs q >= p of the M x M grid, and ONE mirror of the result at the very end) against the NumPy oracle and
against the order that contracts the trailing indices first (``exchange_order=0``), both within the project's
1e-10 * max|ref|; general C and C_tilde that are not adjoints, square and rectangular (M < L forced: the automatic rule
never takes the order there), blocks that do not divide the size, both dtypes, out of place and in place.

The mirror is a copy, so ``out[p,q,r,s] == out[q,p,s,r]`` bit for bit for every p != q.  ``exchange_pairs=0`` (c per row
p, d per block of rows) gives the bits of the one-launch forms.  With ``exchange_order`` at its default the forced route
at 24 orbitals is the old order: the automatic rule starts no lower than the route itself does.

At L = M = 128 the product launches are a, the closing product's two blocks of 64 rows, d and c, every one an exact
form of the fast product kernel -- for fp64 the c launch is the form that stores the mirror from its own epilogue, and
the record has no mirror kernel; the result is bounded against the plain route there, as tests/test_gpu_exchange_route.py
does it (a NumPy oracle of 128^4 elements would be gigabytes on the host)."""

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


def _route(K, u, C, Ct, block, inplace=False, **knobs):
    with K.tuning(exchange=2, exchange_block=block, **knobs):
        got = K.transform_two_body_(u.clone(), C, Ct) if inplace else K.transform_two_body(u, C, Ct)
        return got, K.last_dispatch()


@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "c128"])
@pytest.mark.parametrize("L,M,block", [(24, 24, 8), (33, 33, 8), (40, 40, 16), (12, 20, 8), (20, 12, 8)])
def test_leading_indices_first_against_oracle_and_old_order(L, M, block, dtype):
    from quantum_systems_amd import kernels as K

    u_h, C_h, Ct_h = _inputs(L, M, dtype, seed=L * 100 + M)
    ref = orc.transform_two_body(u_h, C_h, Ct_h)
    scale = np.abs(ref).max()
    u, C, Ct = (torch.from_numpy(x).to(DEV) for x in (u_h, C_h, Ct_h))
    keep = u.clone()
    old, old_dispatch = _route(K, u, C, Ct, block, exchange_order=0)
    K.dispatch_log = log = []
    try:
        got, dispatch = _route(K, u, C, Ct, block, exchange_order=2)
    finally:
        K.dispatch_log = None
    assert torch.equal(u, keep)                                    # u untouched
    # the check's record alone first, then the route's
    assert log[0] == _name("exchange_transpose_check_kernel", dtype) and log[1] == dispatch and len(log) == 2
    mirror = _name("exchange_transpose_kernel", dtype)
    launches = _launches(dispatch)
    # mirror items only at the very end and at most once (the old order has one in the middle too)
    assert [i for i, (name, _) in enumerate(launches) if name == mirror] in ([], [len(launches) - 1]), dispatch
    assert all(n == 1 for name, n in launches if name == mirror), dispatch
    assert dispatch != old_dispatch
    err_ref = np.abs(got.cpu().numpy() - ref).max() / scale
    err_old = (got - old).abs().max().item() / scale
    print(f"exchange order 2 L={L} M={M} block={block} {dtype}: vs oracle {err_ref:.2e}, vs order 0 {err_old:.2e}; {dispatch}")
    assert err_ref <= BOUND and err_old <= BOUND
    # the mirrored pairs are copies: out[p,q,r,s] == out[q,p,s,r] bit for bit for every p != q
    apart = ~torch.eye(M, dtype=torch.bool, device=DEV)
    assert torch.equal(got[apart], got.permute(1, 0, 3, 2)[apart])
    # c per row p and d per block of rows: the same bits
    rows, rows_dispatch = _route(K, u, C, Ct, block, exchange_order=2, exchange_pairs=0)
    assert torch.equal(rows, got), "exchange_pairs=0 differs from exchange_pairs=1"
    products = lambda d: sum(n for name, n in _launches(d) if "transpose" not in name)     # noqa: E731
    assert products(dispatch) <= products(rows_dispatch) - (M - 1), (dispatch, rows_dispatch)
    if M <= L:
        inplace, inplace_dispatch = _route(K, u, C, Ct, block, inplace=True, exchange_order=2)
        assert inplace_dispatch == dispatch
        assert torch.equal(inplace, got)
        assert torch.equal(_route(K, u, C, Ct, block, inplace=True, exchange_order=2, exchange_pairs=0)[0], got)


@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "c128"])
def test_non_symmetric_input_keeps_the_plain_route(dtype):
    from quantum_systems_amd import kernels as K

    u_h, C_h, Ct_h = _inputs(24, 24, dtype, seed=3, symmetric=False)
    u, C, Ct = (torch.from_numpy(x).to(DEV) for x in (u_h, C_h, Ct_h))
    with K.tuning(exchange=0):
        plain = K.transform_two_body(u, C, Ct)
        plain_dispatch = K.last_dispatch()
    for pairs in (0, 1):
        got, dispatch = _route(K, u, C, Ct, 8, exchange_order=2, exchange_pairs=pairs)
        assert dispatch == plain_dispatch and "transpose" not in dispatch
        assert torch.equal(got, plain)


@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "c128"])
def test_default_order_at_24_is_the_old_order(dtype):
    """The policy floor: a forced route (``exchange=2``) far below the automatic thresholds keeps the launches and the
    bits of ``exchange_order=0``."""
    from quantum_systems_amd import kernels as K

    u_h, C_h, Ct_h = _inputs(24, 24, dtype, seed=2424)
    u, C, Ct = (torch.from_numpy(x).to(DEV) for x in (u_h, C_h, Ct_h))
    old, old_dispatch = _route(K, u, C, Ct, 8, exchange_order=0)
    got, dispatch = _route(K, u, C, Ct, 8)
    auto, auto_dispatch = _route(K, u, C, Ct, 8, exchange_order=1)
    assert dispatch == old_dispatch and auto_dispatch == old_dispatch
    assert torch.equal(got, old) and torch.equal(auto, old)
    mirror = _name("exchange_transpose_kernel", dtype)
    assert sum(n for name, n in _launches(dispatch) if name == mirror) == 2, dispatch
    assert _route(K, u, C, Ct, 8, exchange_order=2)[1] != old_dispatch


@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "c128"])
def test_a_closing_blocks_d_c_at_128(dtype):
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
    got, dispatch = _route(K, u, C, Ct, 64, exchange_order=2, **OTHER_ROUTES_OFF)
    scale = plain.abs().max().item()
    err = (got - plain).abs().max().item() / scale
    print(f"exchange order 2 L=M=128 block=64 {dtype}: vs plain route {err:.2e}; {dispatch}")
    assert err <= BOUND                                    # (the plain route is within 1e-10 of the oracle: test_gpu_exchange_route.py)
    if dtype.is_complex:
        exact = {"qs::gemm_fast_kernel<true, 4, 2, true, false>", "qs::gemm_fast_kernel<true, 2, 4, true, false>"}
    else:
        exact = {"qs::gemm_fast_kernel<false, 4, 4, true, false>", "qs::gemm_fast_kernel<false, 2, 4, true, false>"}
    mirror = _name("exchange_transpose_kernel", dtype)
    # fp64: the c launch is the 128 x 128 form whose epilogue also stores the mirror (the record names the overload), and
    # no separate mirror follows; complex128 has no such form and ends with the mirror kernel
    fused = "qs::gemm_fast_kernel<false, 4, 4, true, false>(qs::FastPairsMirrorArgs)"
    launches = _launches(dispatch)
    prods = [(name, n) for name, n in launches if name != mirror]
    assert all(name in exact | {fused} for name, _ in prods), dispatch
    assert sum(n for _, n in prods) == 5, dispatch                      # a, the closing product's two blocks, d, c
    kinds = [name == mirror for name, n in launches for _ in range(n)]
    if dtype.is_complex:
        assert kinds == [False] * 5 + [True] and fused not in dispatch, dispatch
    else:
        assert kinds == [False] * 5 and launches[-1] == (fused, 1), dispatch
    # which product is which: the old order at this size launches the same five shapes as d, c, a, closing, closing, so
    # its record read in the new order's sequence (a, closing, closing, d, c) is this one
    old_dispatch = _route(K, u, C, Ct, 64, exchange_order=0, **OTHER_ROUTES_OFF)[1]
    old_prods = [name for name, n in _launches(old_dispatch) if name != mirror for _ in range(n)]
    new_prods = [name.partition("(")[0] for name, n in prods for _ in range(n)]
    assert new_prods == old_prods[2:] + old_prods[:2], (dispatch, old_dispatch)
    apart = ~torch.eye(L, dtype=torch.bool, device=DEV)
    assert torch.equal(got[apart], got.permute(1, 0, 3, 2)[apart])
    # c per row and the separate mirror kernel: the bits of the mirror stored by the c launch itself
    rows, rows_dispatch = _route(K, u, C, Ct, 64, exchange_order=2, exchange_pairs=0, **OTHER_ROUTES_OFF)
    assert mirror in rows_dispatch.split(";") and fused not in rows_dispatch
    assert torch.equal(rows, got)
    inplace, inplace_dispatch = _route(K, u, C, Ct, 64, inplace=True, exchange_order=2, **OTHER_ROUTES_OFF)
    assert inplace_dispatch == dispatch and torch.equal(inplace, got)
