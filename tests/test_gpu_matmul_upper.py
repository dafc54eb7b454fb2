"""The product on a column triangle (``qs_matmul_upper``, include/qs_amd.h) alone: the n columns are a stack of row-major
side x side matrices (c, d); a tile's 128 columns are R rows c of S contiguous columns d (S = 16, R = 8 as shipped; S = 32,
R = 4 under ``gemm_upper_s=32``), and a tile exists iff its last column >= its first row.

Every kept element is compared bit for bit with ``kernels.matmul`` on the same operands (on its tiled forms: every tiled
form sums along k in the same order): both tile heights (m = 64, 128), one, two and three k-stages (k = 16, 32, 48), sides
of 2, 6 and 12 tiles at S = 16 (8 and 24 at S = 32), stacks of 1 and 3 with batches of 1 and 2, ``ldb`` and ``ldc`` larger than n,
one tile per workgroup, walks of 3 tiles and the fully persistent grid (``gemm_fast_persist`` = 0, 3, 2), so that a
workgroup re-aims its cursor across blocks, stack entries and batch entries.  The output starts as a NaN sentinel: kept
blocks are finite and the product's bits, everything else is still the sentinel; B is NaN outside the kept blocks, so
nothing else is read.  The kept set is computed here from the sentence above, not from the library.  Every refusal
returns before a launch."""

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SENTINEL_BITS = 0x7FF8DEAD0000BEEF                       # a quiet NaN with a payload of its own
TILED = dict(gemm_strip=0, gemm_stream=0, gemm_skinny=0, gemm_fit=0)
SIDES = {16: (16, 32, 48), 32: (32, 64)}
TILES = {(16, 16): 2, (16, 32): 6, (16, 48): 12, (32, 32): 8, (32, 64): 24}


def _kept(side, S):
    """(side, side) bool: the blocks of R = 128 / S rows and S columns whose last column >= their first row."""
    R = 128 // S
    first_row = (torch.arange(side, device=DEV) // R) * R
    last_col = (torch.arange(side, device=DEV) // S) * S + S - 1
    return last_col[None, :] >= first_row[:, None]


def _sentinel(shape):
    return torch.full(shape, SENTINEL_BITS, dtype=torch.int64, device=DEV).view(torch.float64)


@pytest.mark.parametrize("S", [16, 32])
@pytest.mark.parametrize("k", [16, 32, 48])
@pytest.mark.parametrize("m", [64, 128])
def test_kept_blocks_are_the_product_and_nothing_else_is_touched(m, k, S):
    from quantum_systems_amd import kernels as K

    f64 = torch.float64
    name = f"qs::gemm_fast_kernel<false, {m // 32}, 4, true, false>(qs::FastUpperArgs)"
    g = torch.Generator(device=DEV).manual_seed(1000 * m + 10 * k + S)
    A = torch.randn((m, k), dtype=f64, device=DEV, generator=g)
    for side in SIDES[S]:
        kept1 = _kept(side, S)
        assert int(kept1.sum()) == TILES[(S, side)] * 128      # the tile list the issue counts
        for stack, batch in ((1, 1), (3, 2)):
            n = stack * side * side
            ldb, ldc = n + 8, n + 4
            kept = kept1.reshape(-1).repeat(stack)                               # (n,)
            clean = torch.randn((batch, k, n), dtype=f64, device=DEV, generator=g)
            with K.tuning(**TILED):
                want = K.matmul(A, clean)                                        # (batch, m, n)
            B = torch.full((batch, k + 1, ldb), float("nan"), dtype=f64, device=DEV)
            B[:, :k, :n] = torch.where(kept, clean, torch.full_like(clean, float("nan")))
            for persist in (0, 3, 2):
                out = _sentinel((batch, m + 1, ldc))
                with K.tuning(gemm_fast_persist=persist, gemm_upper_s=S):
                    K.matmul_upper(f64, A, B, out, m, side, stack, k, k, ldb, ldc, batch, 0, (k + 1) * ldb, (m + 1) * ldc)
                    dispatch = K.last_dispatch()
                where = f"m={m} k={k} S={S} side={side} stack={stack} batch={batch} persist={persist}"
                assert dispatch == name, (where, dispatch)
                body = out[:, :m, :n]
                assert bool(torch.isfinite(body[:, :, kept]).all()), where
                assert torch.equal(body[:, :, kept], want[:, :, kept]), where
                bits = out.view(torch.int64)
                assert bool((bits[:, :m, :n][:, :, ~kept] == SENTINEL_BITS).all()), where
                assert bool((bits[:, :, n:] == SENTINEL_BITS).all()) and bool((bits[:, m] == SENTINEL_BITS).all()), where


def test_refusals_launch_nothing():
    from quantum_systems_amd import kernels as K

    f64 = torch.float64

    def refused(dt, m, side, k, **kw):
        n = side * side
        A = torch.zeros((m, k), dtype=dt, device=DEV)
        B = torch.zeros((k, n), dtype=dt, device=DEV)
        out = torch.full((m, n), -777.25, dtype=dt, device=DEV)
        with pytest.raises(ValueError):
            K.matmul_upper(dt, A, B, out, m, side, 1, k, k, n, n, **kw)
        assert K.last_dispatch() == ""
        torch.cuda.synchronize()
        assert bool((out == -777.25).all())

    refused(f64, 64, 24, 16)                         # side no multiple of S
    refused(f64, 64, 40, 16)
    with K.tuning(gemm_upper_s=32):
        refused(f64, 64, 48, 16)                     # a multiple of 16, not of 32
    refused(torch.complex128, 64, 32, 16)            # complex128: not built
    refused(f64, 64, 32, 16, accumulate=True)
    refused(f64, 96, 32, 16)                         # m no whole number of 64-row tiles
    refused(f64, 64, 32, 24)                         # k no whole k-stage
    with K.tuning(gemm_fast=0):                      # the general kernel walks no column triangle
        refused(f64, 64, 32, 16)
    # the same shape without a reason to refuse runs
    A = torch.zeros((64, 16), dtype=f64, device=DEV)
    K.matmul_upper(f64, A, torch.zeros((16, 1024), dtype=f64, device=DEV), torch.zeros((64, 1024), dtype=f64, device=DEV),
                   64, 32, 1, 16, 16, 1024, 1024)
    assert K.last_dispatch() == "qs::gemm_fast_kernel<false, 2, 4, true, false>(qs::FastUpperArgs)"
