"""The triangular batch that also stores its mirror (``qs_matmul_pairs_mirrored``, include/qs_amd.h), driven through its C
entry: entry (i, j > i) of the n x n grid is stored a second time, transposed, at entry (j, i) -- out of the registers
that hold it, so bit for bit.

fp64 on the exact 128 x 128 form (the one form with this epilogue) at m = n = 128 (one tile per pair) and 256 (four), k =
16 and 32 (one and two k-stages), grids of 1, 2 and 5 rows, one tile per workgroup and walks of 3 and 9 tiles
(``gemm_fast_persist``), so that a workgroup's walk crosses rows of pairs and diagonal entries, whose epilogue stores
once.  The shapes are the route's c launch: a shared A (``stride_a = 0``); the output has ``ldc = n + 4`` and one spare
row between entries, both filled with a sentinel; the operand entries of the pairs j < i, which nothing may read into an
output, are NaN.  (The 64 x 128 form needs n % 128 == 0 and m == n makes that the 128 x 128 form: it has no mirrored
instantiation.)"""

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SENTINEL = -777.25
MIRRORED = "qs::gemm_fast_kernel<false, 4, 4, true, false>(qs::FastPairsMirrorArgs)"
PLAIN = "qs::gemm_fast_kernel<false, 4, 4, true, false>"


def _operands(m, k, grid, seed):
    g = torch.Generator(device=DEV).manual_seed(seed)
    A = torch.randn((m, k), dtype=torch.float64, device=DEV, generator=g)
    B = torch.randn((grid, grid, k, m), dtype=torch.float64, device=DEV, generator=g)
    lower = torch.tril(torch.ones((grid, grid), dtype=torch.bool, device=DEV), diagonal=-1)
    B[lower] = float("nan")
    return A, B


def _launch(K, A, B, m, k, grid, mirror):
    """The (grid, grid, m + 1, m + 4) output buffer after the launch, and the dispatch record."""
    ldc = m + 4
    out = torch.full((grid, grid, m + 1, ldc), SENTINEL, dtype=torch.float64, device=DEV)
    K.gemm_raw(torch.float64, A, B, out, m, m, k, k, m, ldc, 0, 0, k * m, (m + 1) * ldc, pairs=grid, mirror=mirror)
    return out, K.last_dispatch()


@pytest.mark.parametrize("k", [16, 32])
@pytest.mark.parametrize("m", [128, 256])
def test_mirrored_pairs_against_the_unmirrored_launch(m, k):
    from quantum_systems_amd import kernels as K

    for grid in (1, 2, 5):
        A, B = _operands(m, k, grid, seed=1000 * m + 10 * k + grid)
        upper = torch.triu(torch.ones((grid, grid), dtype=torch.bool, device=DEV))
        strict = torch.triu(upper, diagonal=1)
        diag = torch.eye(grid, dtype=torch.bool, device=DEV)
        # the unmirrored launch is the product: every entry j >= i against A . B[i, j], to the rounding of k terms
        want = torch.matmul(A, B[upper])
        bound = 2 * k * 2.0**-52 * torch.matmul(A.abs(), B[upper].abs())
        for persist in (0, 3, 9):
            with K.tuning(gemm_fast_persist=persist):
                plain, plain_dispatch = _launch(K, A, B, m, k, grid, mirror=False)
                got, dispatch = _launch(K, A, B, m, k, grid, mirror=True)
            where = f"m={m} k={k} grid={grid} persist={persist}"
            assert plain_dispatch == PLAIN and dispatch == MIRRORED, (where, plain_dispatch, dispatch)
            assert bool(((plain[upper][:, :m, :m] - want).abs() <= bound).all()), where
            # entries j >= i, diagonal included: the unmirrored launch's bits
            assert torch.equal(got[upper], plain[upper]), where
            assert torch.equal(got[diag], plain[diag]), where
            # entries j < i: the transposes of their partners (and nothing from the NaN operand entries)
            mirrored = got.transpose(0, 1)[strict][:, :m, :m]        # entry (j, i) for every (i, j > i)
            assert torch.equal(mirrored, got[strict][:, :m, :m].transpose(1, 2)), where
            assert not bool(torch.isnan(got).any()), where
            # padding columns and the spare row between entries: untouched by either store pattern
            assert bool((got[:, :, :, m:] == SENTINEL).all()) and bool((got[:, :, m] == SENTINEL).all()), where
            # the unmirrored launch writes nothing at j < i
            assert bool((plain.transpose(0, 1)[strict] == SENTINEL).all()), where


def test_refusals_launch_nothing():
    from quantum_systems_amd import kernels as K

    f64 = torch.float64

    def refused(dt, m, n, k, **kw):
        A = torch.zeros((m, k), dtype=dt, device=DEV)
        B = torch.zeros((2, 2, k, n), dtype=dt, device=DEV)
        out = torch.full((2, 2, m, n), SENTINEL, dtype=dt, device=DEV)
        with pytest.raises(ValueError):
            K.gemm_raw(dt, A, B, out, m, n, k, k, n, n, 0, 0, k * n, m * n, pairs=2, mirror=True, **kw)
        assert K.last_dispatch() == ""
        torch.cuda.synchronize()
        assert bool((out == SENTINEL).all())
        # the same product without the flag runs
        K.gemm_raw(dt, A, B, out, m, n, k, k, n, n, 0, 0, k * n, m * n, pairs=2, **kw)
        assert K.last_dispatch() != ""

    refused(f64, 128, 256, 16)                      # m != n
    refused(f64, 128, 128, 16, accumulate=True)
    refused(f64, 64, 64, 16)                        # no 128 x 128 tiles: a form without the mirrored epilogue
    refused(f64, 136, 136, 16)                      # an edge form
    refused(f64, 128, 128, 8)                       # k no whole k-stage
    refused(torch.complex128, 128, 128, 16)         # complex128: not built
    with K.tuning(gemm_fast=0):                     # the general kernel has no such epilogue
        refused(f64, 128, 128, 16)
    with pytest.raises(ValueError):
        K.gemm_raw(f64, torch.zeros(1, device=DEV, dtype=f64), torch.zeros(1, device=DEV, dtype=f64),
                   torch.zeros(1, device=DEV, dtype=f64), 128, 128, 16, 16, 128, 128, mirror=True)
