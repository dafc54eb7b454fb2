"""The exchange route's column-triangle pass without its fill (``exchange=2, exchange_order=2, exchange_upper=2,
exchange_lower=2``: after the two ``qs_matmul_upper`` products the d launch over the pairs q >= p runs as
``qs_matmul_pairs_lower`` and takes the blocks below the block diagonal from the mirror pair) against the NumPy oracle
and against the same pass with the fill (``exchange_upper=2`` alone), both within the project's 1e-10 * max|ref|; general
C and C_tilde that are not adjoints; M > L, M == L and M < L, out of place and in place (there the never-written blocks
hold stale u).

The record where the d launch exists (L a multiple of 64, M of 128): the check's alone first; then two
``(qs::FastUpperArgs)`` launches, NO fill, one ``(qs::FastPairsLowerArgs)``, then c as the pass with the fill ends.  Where
it does not exist -- M = 64 here, and the edge forms (48, 64) and (80, 128) -- the key changes nothing: launch for launch
and bit for bit the pass with the fill.  A tensor without the symmetry keeps the plain route."""

import functools

import numpy as np
import pytest
import torch

from oracle import qs_oracle as orc

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BOUND = 1e-10
UPPER = "(qs::FastUpperArgs)"
LOWER = "(qs::FastPairsLowerArgs)"
FILL = "qs::exchange_transpose_lower_kernel<double>"
WITH_FILL = dict(exchange_upper=2)
NO_FILL = dict(exchange_upper=2, exchange_lower=2)


@functools.lru_cache(maxsize=None)
def _inputs(L, M, symmetric=True):
    """Device operands and the oracle's result (computed once per shape)."""
    g = torch.Generator(device=DEV).manual_seed(L * 1000 + M)
    u = torch.randn((L, L, L, L), dtype=torch.float64, device=DEV, generator=g)
    if symmetric:
        u = u + u.permute(1, 0, 3, 2)                      # (x + y is exactly commutative)
    C = torch.randn((L, M), dtype=torch.float64, device=DEV, generator=g) / L**0.5
    Ct = torch.randn((M, L), dtype=torch.float64, device=DEV, generator=g) / L**0.5
    ref = orc.transform_two_body(u.cpu().numpy(), C.cpu().numpy(), Ct.cpu().numpy())
    return u.contiguous(), C, Ct, ref


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


@pytest.mark.parametrize("L,M", [(64, 64), (128, 128), (64, 128), (128, 64)])
def test_pass_without_the_fill_against_oracle_and_the_fill(L, M):
    from quantum_systems_amd import kernels as K

    u, C, Ct, ref = _inputs(L, M)
    scale = np.abs(ref).max()
    keep = u.clone()
    filled, filled_dispatch = _route(K, u, C, Ct, **WITH_FILL)
    K.dispatch_log = log = []
    try:
        got, dispatch = _route(K, u, C, Ct, **NO_FILL)
    finally:
        K.dispatch_log = None
    assert torch.equal(u, keep)                                    # u untouched
    assert log[0] == "qs::exchange_transpose_check_kernel<double>" and log[1] == dispatch and len(log) == 2
    names, filled_names = _names(dispatch), _names(filled_dispatch)
    assert filled_names.count(FILL) == 1 and LOWER not in filled_dispatch, filled_dispatch
    eligible = L % 64 == 0 and M % 128 == 0
    assert lib_says(K, L, M) == eligible
    if eligible:
        # two products on the column triangle, no fill, d from the mirror pair, then c as the pass with the fill ends
        form = f"qs::gemm_fast_kernel<false, 4, 4, true, false>{UPPER}"
        d_form = f"qs::gemm_fast_kernel<false, {4 if L % 128 == 0 else 2}, 4, true, false>{LOWER}"
        assert names[:3] == [form, form, d_form], dispatch
        assert FILL not in dispatch and sum(LOWER in name for name in names) == 1 and sum(UPPER in name for name in names) == 2
        assert filled_names[:3] == [form, form, FILL] and LOWER not in filled_names[3] and names[3:] == filled_names[4:], (dispatch, filled_dispatch)
    else:
        assert dispatch == filled_dispatch
        assert torch.equal(got, filled)
    err_ref = np.abs(got.cpu().numpy() - ref).max() / scale
    err_fill = (got - filled).abs().max().item() / scale
    print(f"exchange lower L={L} M={M}: vs oracle {err_ref:.2e}, vs the pass with the fill {err_fill:.2e}; {dispatch}")
    assert err_ref <= BOUND and err_fill <= BOUND
    # the mirrored pairs are copies: out[p,q,r,s] == out[q,p,s,r] bit for bit for every p != q
    apart = ~torch.eye(M, dtype=torch.bool, device=DEV)
    assert torch.equal(got[apart], got.permute(1, 0, 3, 2)[apart])
    if M <= L:
        inplace, inplace_dispatch = _route(K, u, C, Ct, inplace=True, **NO_FILL)
        assert inplace_dispatch == dispatch
        err_inplace = np.abs(inplace.cpu().numpy() - ref).max() / scale
        assert err_inplace <= BOUND
        assert torch.equal(inplace, got)                           # (the stale blocks are read by nothing)


def lib_says(K, L, M):
    with K.tuning(exchange=2, exchange_order=2, **NO_FILL):
        return bool(K._lib.load().qs_transform_two_body_exchange_lower_d(0, L, M))


@pytest.mark.parametrize("L,M", [(48, 64), (80, 128)])
def test_edge_forms_keep_the_launches_with_the_fill(L, M):
    from quantum_systems_amd import kernels as K

    u, C, Ct, _ = _inputs(L, M)
    filled, filled_dispatch = _route(K, u, C, Ct, **WITH_FILL)
    got, dispatch = _route(K, u, C, Ct, **NO_FILL)
    assert dispatch == filled_dispatch and FILL in dispatch and LOWER not in dispatch
    assert torch.equal(got, filled)


def test_non_symmetric_input_keeps_the_plain_route():
    from quantum_systems_amd import kernels as K

    u, C, Ct, _ = _inputs(64, 128, symmetric=False)
    with K.tuning(exchange=0):
        plain = K.transform_two_body(u, C, Ct)
        plain_dispatch = K.last_dispatch()
    got, dispatch = _route(K, u, C, Ct, **NO_FILL)
    assert dispatch == plain_dispatch and "transpose" not in dispatch and UPPER not in dispatch and LOWER not in dispatch
    assert torch.equal(got, plain)
