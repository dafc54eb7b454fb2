"""The triangular batch that takes the blocks below the block diagonal of its square A entries from the mirror pair
(``qs_matmul_pairs_lower``, include/qs_amd.h), driven through its C entry on the exchange route's d shape: a shared B
(``stride_b = 0``), A entries side x side at every flat index of the grid.

For every pair (i, j >= i) the launch may read the 16 x 16 blocks (G, J >= G) of entry (i, j) and the blocks (J, G), J < G,
of entry (j, i), and nothing else of A.  The stored tensor here is random; the full per-pair matrices are BUILT from exactly
those blocks for the NumPy reference; everything the launch must not read is NaN in the poisoned copy.

fp64 at side 64 (one 64-row tile), 128 (one 128-row tile), 192 (three 64-row tiles: row groups from 4 and 8) and 256 (two
128-row tiles: the second wave pair's row groups start at 4 and 12), grids of 1, 2 and 3, n = 128; a forced walk of three
tiles per workgroup, and a list of 1200 tiles, more than the resident workgroups take singly, so that the fetch cursor
crosses tile boundaries while it reads turned blocks and while it reads natural ones.  Parity within the project's
1e-10 * max|ref|; bit for bit against the fill followed by ``qs_matmul_pairs`` (the diagonal blocks of (i, j) and (j, i)
are each other's transposes here, as the route's second product leaves them to rounding)."""

import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BOUND = 1e-10
SENTINEL = -777.25
f64 = torch.float64


def _form(side):
    return f"qs::gemm_fast_kernel<false, {4 if side % 128 == 0 else 2}, 4, true, false>(qs::FastPairsLowerArgs)"


def _stored(side, grid, n, seed):
    """A random (grid, grid, side, side) tensor whose diagonal blocks (G, G) of entries (i, j) and (j, i) are each other's
    transposes, and the shared (side, n) matrix."""
    g = torch.Generator(device=DEV).manual_seed(seed)
    S = torch.randn((grid, grid, side, side), dtype=f64, device=DEV, generator=g)
    B = torch.randn((side, n), dtype=f64, device=DEV, generator=g)
    nb = side // 16
    S6 = S.view(grid, grid, nb, 16, nb, 16)
    below = torch.tril(torch.ones((grid, grid), dtype=torch.bool, device=DEV), diagonal=-1)[:, :, None, None]
    for G in range(nb):
        blk = S6[:, :, G, :, G, :]
        b = blk.clone()
        b = torch.where(below, b.permute(1, 0, 3, 2), b)
        for i in range(grid):
            b[i, i] = torch.triu(b[i, i]) + torch.triu(b[i, i], 1).T
        blk.copy_(b)
    return S, B


def _poisoned(S):
    """NaN wherever the launch must not read: every block below the block diagonal of every entry, and the diagonal blocks
    of the entries j < i."""
    grid, side = S.shape[0], S.shape[2]
    nb = side // 16
    P = S.clone()
    P6 = P.view(grid, grid, nb, 16, nb, 16)
    below = torch.tril(torch.ones((grid, grid), dtype=torch.bool, device=DEV), diagonal=-1)
    for G in range(nb):
        P6[:, :, G, :, :G, :] = float("nan")
        v = P6[:, :, G, :, G, :]
        v[below] = float("nan")
    return P


def _reference(S, B):
    """NumPy: the full matrix of every pair from the stored blocks, times B; (grid, grid, side, n), zero at j < i."""
    S_h, B_h = S.cpu().numpy(), B.cpu().numpy()
    grid, side = S_h.shape[0], S_h.shape[2]
    lower_blocks = np.kron(np.tril(np.ones((side // 16, side // 16)), -1), np.ones((16, 16))).astype(bool)
    ref = np.zeros((grid, grid, side, B_h.shape[1]))
    for i in range(grid):
        for j in range(i, grid):
            ref[i, j] = np.where(lower_blocks, S_h[j, i].T, S_h[i, j]) @ B_h
    return ref


def _launch(K, A, B, lower, **kw):
    grid, side, n = A.shape[0], A.shape[2], B.shape[1]
    out = torch.full((grid, grid, side, n), SENTINEL, dtype=f64, device=DEV)
    K.gemm_raw(f64, A, B, out, side, n, side, side, n, n, 0, side * side, 0, side * n, pairs=grid, lower=lower, **kw)
    return out, K.last_dispatch()


@functools.lru_cache(maxsize=None)
def _case(side, grid, n=128):
    """Operands, NumPy reference and fill-then-``qs_matmul_pairs`` result of one shape, computed once."""
    from quantum_systems_amd import kernels as K

    S, B = _stored(side, grid, n, seed=1000 * side + grid)
    ref = _reference(S, B)
    filled = K.exchange_mirror_lower_(S.clone())
    want, _ = _launch(K, filled, B, lower=False)
    return S, B, ref, want


def _check(K, side, grid, n=128, numpy_pairs=None):
    S, B, ref, want = _case(side, grid, n)
    upper = torch.triu(torch.ones((grid, grid), dtype=torch.bool, device=DEV))
    where = f"side={side} grid={grid} n={n}"
    got, dispatch = _launch(K, S, B, lower=True)
    assert dispatch == _form(side), (where, dispatch)
    got_h = got.cpu().numpy()
    up_h = upper.cpu().numpy()
    err = np.abs(got_h[up_h] - ref[up_h]).max() / np.abs(ref).max()
    print(f"matmul_pairs_lower {where}: vs NumPy {err:.2e}")
    assert err <= BOUND, where
    # bit for bit the fill followed by the plain triangular batch
    assert torch.equal(got[upper], want[upper]), where
    # nothing is written at the flat indices j < i
    assert bool((got[~upper] == SENTINEL).all()), where
    # NaN wherever the launch must not read: finite and unchanged
    poisoned, dispatch = _launch(K, _poisoned(S), B, lower=True)
    assert dispatch == _form(side), (where, dispatch)
    assert bool(torch.isfinite(poisoned).all()), where
    assert torch.equal(poisoned, got), where


@pytest.mark.parametrize("grid", [1, 2, 3])
@pytest.mark.parametrize("side", [64, 128, 192, 256])
def test_lower_blocks_from_the_mirror_pair(side, grid):
    from quantum_systems_amd import kernels as K

    _check(K, side, grid)


def test_forced_walk_of_three_tiles():
    from quantum_systems_amd import kernels as K

    with K.tuning(gemm_fast_persist=3):
        _check(K, 256, 3)


def test_long_tile_list():
    """Grid 24, side 256, n = 256: 300 pairs x 2 x 2 tiles, two or three per resident workgroup."""
    from quantum_systems_amd import kernels as K

    _check(K, 256, 24, n=256)


def test_refusals_launch_nothing():
    from quantum_systems_amd import kernels as K

    def refused(dt, m, n, k, **kw):
        A = torch.zeros((2, 2, m, k), dtype=dt, device=DEV)
        B = torch.zeros((k, n), dtype=dt, device=DEV)
        out = torch.full((2, 2, m, n), SENTINEL, dtype=dt, device=DEV)
        with pytest.raises(ValueError):
            K.gemm_raw(dt, A, B, out, m, n, k, k, n, n, 0, m * k, 0, m * n, pairs=2, lower=True, **kw)
        assert K.last_dispatch() == ""
        torch.cuda.synchronize()
        assert bool((out == SENTINEL).all())
        # the same product without the flag runs
        K.gemm_raw(dt, A, B, out, m, n, k, k, n, n, 0, m * k, 0, m * n, pairs=2, **kw)
        assert K.last_dispatch() != ""

    refused(torch.complex128, 128, 128, 128)        # complex128: not built
    refused(f64, 128, 128, 128, accumulate=True)
    refused(f64, 40, 128, 40)                       # side no multiple of 16 or of a row tile
    refused(f64, 128, 128, 64)                      # m != k
    refused(f64, 64, 128, 128)
    refused(f64, 128, 64, 128)                      # n no whole 128-column tile
    with K.tuning(gemm_fast=0):                     # the general kernel fetches no mirror blocks
        refused(f64, 128, 128, 128)
    with pytest.raises(ValueError):
        K.gemm_raw(f64, torch.zeros(1, device=DEV, dtype=f64), torch.zeros(1, device=DEV, dtype=f64),
                   torch.zeros(1, device=DEV, dtype=f64), 128, 128, 128, 128, 128, 128, lower=True)
