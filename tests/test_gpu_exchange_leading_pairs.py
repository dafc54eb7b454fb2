"""The exchange route with its leading indices contracted on pairs (``exchange=2, exchange_order=2,
exchange_leading=2``: u turned on the pairs d >= c, b and a as two products over those pairs, the way back with the
other half filled in, then d and c on the pairs q >= p as before) against the NumPy oracle and against the same order
with ``exchange_leading=0`` (a as one product, then the closing blocks), both within the project's 1e-10 * max|ref|;
general C and C_tilde that are not adjoints, sizes one past one and two tiles of the movers, M > L, both dtypes, out of
place and in place.

The record: the check's alone first; then the route's, with the two movers, no closing blocks (as many product launches
between the movers as after them where L == M: b + a, d + c) and at most one mirror kernel, at the very end.  Where the
pair-wise part cannot hold its intermediates (M < L) key value 2 is key value 0, launch for launch and bit for bit; a
tensor without the symmetry keeps the plain route; and with the key at its default, a forced route at 24 orbitals and the
route at 128 are those of key value 0."""

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
    return f"qs::{kernel}<{'f64x2' if dtype.is_complex else 'double'}"          # (the movers' names go on: tile side, walk)


def _launches(dispatch):
    """[(kernel name, launches)] of a dispatch record ("name xN" stands for N launches in a row)."""
    out = []
    for item in dispatch.split(";"):
        name, sep, count = item.rpartition(" x")
        out.append((name, int(count)) if sep and count.isdigit() else (item, 1))
    return out


def _route(K, u, C, Ct, block, inplace=False, **knobs):
    knobs.setdefault("exchange_order", 2)
    with K.tuning(exchange=2, exchange_block=block, **knobs):
        got = K.transform_two_body_(u.clone(), C, Ct) if inplace else K.transform_two_body(u, C, Ct)
        return got, K.last_dispatch()


@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "c128"])
@pytest.mark.parametrize("L,M,block", [(24, 24, 8), (33, 33, 8), (40, 40, 16), (65, 65, 16), (12, 20, 8)])
def test_leading_indices_on_pairs_against_oracle_and_blocks(L, M, block, dtype):
    from quantum_systems_amd import kernels as K

    u_h, C_h, Ct_h = _inputs(L, M, dtype, seed=L * 100 + M)
    ref = orc.transform_two_body(u_h, C_h, Ct_h)
    scale = np.abs(ref).max()
    u, C, Ct = (torch.from_numpy(x).to(DEV) for x in (u_h, C_h, Ct_h))
    keep = u.clone()
    blocks, blocks_dispatch = _route(K, u, C, Ct, block, exchange_leading=0)
    K.dispatch_log = log = []
    try:
        got, dispatch = _route(K, u, C, Ct, block, exchange_leading=2)
    finally:
        K.dispatch_log = None
    assert torch.equal(u, keep)                                    # u untouched
    # the check's record alone first, then the route's
    assert log[0] == _name("exchange_transpose_check_kernel", dtype) + ">" and log[1] == dispatch and len(log) == 2
    launches = _launches(dispatch)
    names = [name for name, _ in launches]
    way_in, way_back = _name("exchange_pair_transpose_kernel", dtype), _name("exchange_pair_transpose_back_kernel", dtype)
    mirror = _name("exchange_transpose_kernel", dtype) + ">"
    i_in = [i for i, name in enumerate(names) if name.startswith(way_in + ",")]
    i_back = [i for i, name in enumerate(names) if name.startswith(way_back + ",")]
    assert i_in == [0] and len(i_back) == 1 and launches[0][1] == 1 and launches[i_back[0]][1] == 1, dispatch
    assert way_in not in blocks_dispatch and way_back not in blocks_dispatch
    # mirror items only at the very end and at most once
    assert [i for i, name in enumerate(names) if name == mirror] in ([], [len(launches) - 1]), dispatch
    assert all(n == 1 for name, n in launches if name == mirror), dispatch
    # no closing blocks: the products are b + a between the movers and d + c after them, each pair of phases either two
    # launches or, where the one d-shaped launch would pad more, 1 + a launch per block of rows
    products = lambda items: sum(n for name, n in items if "transpose" not in name)     # noqa: E731
    between, after = products(launches[1:i_back[0]]), products(launches[i_back[0] + 1:])
    blk_d = min(block, 16)
    assert between in (2, 1 + -(-L // blk_d)) and after in (2, 1 + -(-M // blk_d)), dispatch
    if L == M:
        assert between == after, dispatch                          # the same number of product launches as d + c, twice
    assert products(launches) == between + after
    assert products(_launches(blocks_dispatch)) == 1 + -(-M // block) + after, (dispatch, blocks_dispatch)
    err_ref = np.abs(got.cpu().numpy() - ref).max() / scale
    err_blocks = (got - blocks).abs().max().item() / scale
    print(f"exchange leading 2 L={L} M={M} block={block} {dtype}: vs oracle {err_ref:.2e}, vs leading 0 {err_blocks:.2e}, "
          f"bits {'agree' if torch.equal(got, blocks) else 'differ'}; {dispatch}")
    assert err_ref <= BOUND and err_blocks <= BOUND
    # the mirrored pairs are copies: out[p,q,r,s] == out[q,p,s,r] bit for bit for every p != q
    apart = ~torch.eye(M, dtype=torch.bool, device=DEV)
    assert torch.equal(got[apart], got.permute(1, 0, 3, 2)[apart])
    if M == L:
        inplace, inplace_dispatch = _route(K, u, C, Ct, block, inplace=True, exchange_leading=2)
        assert inplace_dispatch == dispatch
        assert torch.equal(inplace, got)


@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "c128"])
def test_fewer_new_orbitals_take_the_blocks(dtype):
    """M < L: the pair-wise part has nowhere to hold its intermediates; key value 2 is key value 0 there."""
    from quantum_systems_amd import kernels as K

    u_h, C_h, Ct_h = _inputs(20, 12, dtype, seed=2012)
    u, C, Ct = (torch.from_numpy(x).to(DEV) for x in (u_h, C_h, Ct_h))
    blocks, blocks_dispatch = _route(K, u, C, Ct, 8, exchange_leading=0)
    got, dispatch = _route(K, u, C, Ct, 8, exchange_leading=2)
    assert dispatch == blocks_dispatch and "exchange_pair_transpose" not in dispatch
    assert torch.equal(got, blocks)
    inplace, inplace_dispatch = _route(K, u, C, Ct, 8, inplace=True, exchange_leading=2)
    assert inplace_dispatch == blocks_dispatch and torch.equal(inplace, blocks)


@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "c128"])
def test_non_symmetric_input_keeps_the_plain_route(dtype):
    from quantum_systems_amd import kernels as K

    u_h, C_h, Ct_h = _inputs(24, 24, dtype, seed=3, symmetric=False)
    u, C, Ct = (torch.from_numpy(x).to(DEV) for x in (u_h, C_h, Ct_h))
    with K.tuning(exchange=0):
        plain = K.transform_two_body(u, C, Ct)
        plain_dispatch = K.last_dispatch()
    got, dispatch = _route(K, u, C, Ct, 8, exchange_leading=2)
    assert dispatch == plain_dispatch and "transpose" not in dispatch
    assert torch.equal(got, plain)


@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "c128"])
def test_default_key_at_24_is_the_blocks(dtype):
    """The policy floor: a forced route far below the automatic thresholds keeps the launches and the bits of key value 0,
    in the leading-first order and at the default order alike."""
    from quantum_systems_amd import kernels as K

    u_h, C_h, Ct_h = _inputs(24, 24, dtype, seed=2424)
    u, C, Ct = (torch.from_numpy(x).to(DEV) for x in (u_h, C_h, Ct_h))
    for order in (1, 2):
        blocks, blocks_dispatch = _route(K, u, C, Ct, 8, exchange_order=order, exchange_leading=0)
        got, dispatch = _route(K, u, C, Ct, 8, exchange_order=order)
        auto, auto_dispatch = _route(K, u, C, Ct, 8, exchange_order=order, exchange_leading=1)
        assert dispatch == blocks_dispatch and auto_dispatch == blocks_dispatch and "exchange_pair_transpose" not in dispatch
        assert torch.equal(got, blocks) and torch.equal(auto, blocks)
    assert _route(K, u, C, Ct, 8, exchange_leading=2)[1] != blocks_dispatch


@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "c128"])
def test_default_key_at_128_is_the_blocks(dtype):
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
    with K.tuning(exchange=0):
        plain = K.transform_two_body(u, C, Ct)
    blocks, blocks_dispatch = _route(K, u, C, Ct, 64, exchange_leading=0, **OTHER_ROUTES_OFF)
    got, dispatch = _route(K, u, C, Ct, 64, **OTHER_ROUTES_OFF)
    assert dispatch == blocks_dispatch and "exchange_pair_transpose" not in dispatch
    assert torch.equal(got, blocks)
    scale = plain.abs().max().item()
    # ... and on pairs at this size: every product an exact form, bounded against the plain route
    pairs, pairs_dispatch = _route(K, u, C, Ct, 64, exchange_leading=2, **OTHER_ROUTES_OFF)
    err = (pairs - plain).abs().max().item() / scale
    print(f"exchange leading 2 L=M=128 {dtype}: vs plain route {err:.2e}; {pairs_dispatch}")
    assert err <= BOUND and (blocks - plain).abs().max().item() / scale <= BOUND
    assert sum(n for name, n in _launches(pairs_dispatch) if "transpose" not in name) == 4, pairs_dispatch
