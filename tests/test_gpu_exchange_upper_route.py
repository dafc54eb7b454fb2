"""The exchange route with its leading indices on the column triangle (``exchange=2, exchange_order=2,
exchange_upper=2``: b and a as two ``qs_matmul_upper`` products on the column blocks d >= c of u's trailing indices, for
all leading indices, one fill of the triangles d < c of the pairs q >= p, then d and c on those pairs as before) against
the NumPy oracle and against the same order with ``exchange_leading=0`` (a as one product, then the closing blocks), both
within the project's 1e-10 * max|ref|; general C and C_tilde that are not adjoints; L of 3, 4, 5 and 8 segments, M of one
and two 64-row tiles, M > L, M == L and M < L, out of place and in place.

The record: the check's alone first; then the route's, with two ``(qs::FastUpperArgs)`` launches first, the fill, no pair
mover, then the launches of d and c that key value 0 ends with.  Where the product refuses (L no multiple of 16, M none
of 64) key value 2 is key value 0 launch for launch and bit for bit; a tensor without the symmetry keeps the plain route;
and with the key at its default a forced route at 24 orbitals and the route at 128 are those of key value 0."""

import numpy as np
import pytest
import torch

from oracle import qs_oracle as orc

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BOUND = 1e-10
UPPER = "(qs::FastUpperArgs)"
FILL = "qs::exchange_transpose_lower_kernel<double>"
OTHER_ROUTES_OFF = dict(gemm_strip=0, gemm_stream=0, gemm_skinny=0, gemm_fit=0)


def _inputs(L, M, seed, symmetric=True):
    rng = np.random.default_rng(seed)
    u = rng.standard_normal((L, L, L, L))
    if symmetric:
        u = u + u.transpose(1, 0, 3, 2)
    return np.ascontiguousarray(u), rng.standard_normal((L, M)), rng.standard_normal((M, L))


def _names(dispatch):
    """The kernel names of a dispatch record, one per launch ("name xN" stands for N launches in a row)."""
    out = []
    for item in dispatch.split(";"):
        name, sep, count = item.rpartition(" x")
        out += [name] * int(count) if sep and count.isdigit() else [item]
    return out


def _route(K, u, C, Ct, inplace=False, **knobs):
    knobs.setdefault("exchange_order", 2)
    with K.tuning(exchange=2, **knobs):
        got = K.transform_two_body_(u.clone(), C, Ct) if inplace else K.transform_two_body(u, C, Ct)
        return got, K.last_dispatch()


@pytest.mark.parametrize("L,M", [(64, 64), (48, 64), (80, 128), (64, 128), (80, 64)])
def test_leading_indices_on_the_column_triangle_against_oracle_and_blocks(L, M):
    from quantum_systems_amd import kernels as K

    u_h, C_h, Ct_h = _inputs(L, M, seed=L * 1000 + M)
    ref = orc.transform_two_body(u_h, C_h, Ct_h)
    scale = np.abs(ref).max()
    u, C, Ct = (torch.from_numpy(x).to(DEV) for x in (u_h, C_h, Ct_h))
    keep = u.clone()
    blocks, blocks_dispatch = _route(K, u, C, Ct, exchange_leading=0, exchange_upper=0)
    K.dispatch_log = log = []
    try:
        got, dispatch = _route(K, u, C, Ct, exchange_upper=2)
    finally:
        K.dispatch_log = None
    assert torch.equal(u, keep)                                    # u untouched
    assert log[0] == "qs::exchange_transpose_check_kernel<double>" and log[1] == dispatch and len(log) == 2
    names, blocks_names = _names(dispatch), _names(blocks_dispatch)
    form = f"qs::gemm_fast_kernel<false, {4 if M % 128 == 0 else 2}, 4, true, false>{UPPER}"
    assert names[:3] == [form, form, FILL], dispatch
    assert sum(UPPER in name for name in names) == 2 and names.count(FILL) == 1, dispatch
    assert "exchange_pair_transpose" not in dispatch and UPPER not in blocks_dispatch and FILL not in blocks_dispatch
    # d + c (and the mirror, where c does not store it itself) as key value 0 ends
    tail = names[3:]
    assert len(tail) >= 2 and tail == blocks_names[len(blocks_names) - len(tail):], (dispatch, blocks_dispatch)
    assert sum("transpose" not in name for name in blocks_names) == 1 + -(-M // 64) + sum("transpose" not in name for name in tail)
    err_ref = np.abs(got.cpu().numpy() - ref).max() / scale
    err_blocks = (got - blocks).abs().max().item() / scale
    print(f"exchange upper 2 L={L} M={M}: vs oracle {err_ref:.2e}, vs leading 0 {err_blocks:.2e}; {dispatch}")
    assert err_ref <= BOUND and err_blocks <= BOUND
    # the mirrored pairs are copies: out[p,q,r,s] == out[q,p,s,r] bit for bit for every p != q
    apart = ~torch.eye(M, dtype=torch.bool, device=DEV)
    assert torch.equal(got[apart], got.permute(1, 0, 3, 2)[apart])
    if M <= L:
        inplace, inplace_dispatch = _route(K, u, C, Ct, inplace=True, exchange_upper=2)
        assert inplace_dispatch == dispatch
        assert torch.equal(inplace, got)


@pytest.mark.parametrize("L,M", [(40, 64), (48, 72)])
def test_sizes_the_product_refuses_keep_the_launches_of_key_value_0(L, M):
    from quantum_systems_amd import kernels as K

    u_h, C_h, Ct_h = _inputs(L, M, seed=L * 1000 + M)
    u, C, Ct = (torch.from_numpy(x).to(DEV) for x in (u_h, C_h, Ct_h))
    for leading in (0, 2):
        before, before_dispatch = _route(K, u, C, Ct, exchange_leading=leading, exchange_upper=0)
        got, dispatch = _route(K, u, C, Ct, exchange_leading=leading, exchange_upper=2)
        assert dispatch == before_dispatch and UPPER not in dispatch and FILL not in dispatch
        assert torch.equal(got, before)


def test_non_symmetric_input_keeps_the_plain_route():
    from quantum_systems_amd import kernels as K

    u_h, C_h, Ct_h = _inputs(64, 64, seed=3, symmetric=False)
    u, C, Ct = (torch.from_numpy(x).to(DEV) for x in (u_h, C_h, Ct_h))
    with K.tuning(exchange=0):
        plain = K.transform_two_body(u, C, Ct)
        plain_dispatch = K.last_dispatch()
    got, dispatch = _route(K, u, C, Ct, exchange_upper=2)
    assert dispatch == plain_dispatch and "transpose" not in dispatch and UPPER not in dispatch
    assert torch.equal(got, plain)


def test_default_key_at_24_is_unchanged():
    from quantum_systems_amd import kernels as K

    u_h, C_h, Ct_h = _inputs(24, 24, seed=2424)
    u, C, Ct = (torch.from_numpy(x).to(DEV) for x in (u_h, C_h, Ct_h))
    for order in (1, 2):
        for leading in (0, 1, 2):
            before, before_dispatch = _route(K, u, C, Ct, exchange_order=order, exchange_leading=leading, exchange_upper=0)
            got, dispatch = _route(K, u, C, Ct, exchange_order=order, exchange_leading=leading)
            assert dispatch == before_dispatch and UPPER not in dispatch and FILL not in dispatch
            assert torch.equal(got, before)


def test_default_key_at_128_is_unchanged():
    from quantum_systems_amd import kernels as K

    L = 128
    g = torch.Generator(device=DEV).manual_seed(11)
    u = torch.randn((L, L, L, L), dtype=torch.float64, device=DEV, generator=g)
    for a in range(L):                                     # symmetrise slab by slab (x + y is exactly commutative)
        s = u[a, a:] + u[a:, a].transpose(1, 2)
        u[a, a:] = s
        u[a:, a] = s.transpose(1, 2)
    C = torch.randn((L, L), dtype=torch.float64, device=DEV, generator=g) / L**0.5
    Ct = torch.randn((L, L), dtype=torch.float64, device=DEV, generator=g) / L**0.5
    for leading in (1, 2):
        before, before_dispatch = _route(K, u, C, Ct, exchange_leading=leading, exchange_upper=0, **OTHER_ROUTES_OFF)
        got, dispatch = _route(K, u, C, Ct, exchange_leading=leading, **OTHER_ROUTES_OFF)
        assert dispatch == before_dispatch and UPPER not in dispatch and FILL not in dispatch
        assert torch.equal(got, before)
    # ... and on the column triangle at this size: every product an exact 128-row form, bounded against key value 0
    upper, upper_dispatch = _route(K, u, C, Ct, exchange_upper=2, **OTHER_ROUTES_OFF)
    scale = before.abs().max().item()
    err = (upper - before).abs().max().item() / scale
    print(f"exchange upper 2 L=M=128: vs exchange_upper 0 {err:.2e}; {upper_dispatch}")
    assert err <= BOUND
    names = _names(upper_dispatch)
    assert names[:3] == [f"qs::gemm_fast_kernel<false, 4, 4, true, false>{UPPER}"] * 2 + [FILL], upper_dispatch
    assert sum("transpose" not in name for name in names) == 4, upper_dispatch
