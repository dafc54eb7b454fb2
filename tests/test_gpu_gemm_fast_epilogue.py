"""The tile epilogue and the stage loop of the exact fp64 DMA forms of ``gemm_fast_kernel`` (qs_gemm_fast_body.h), all five
overloads: which lane stores which column, where a tile's rows and columns land in memory, what the column triangle and the
mirror make of them, and that a tile's stores leave the next tile alone.

Every stored element is compared for equal bits with ``torch.matmul`` in fp64 on the same operands; nothing expected comes
from the library.  The operands are whole numbers small enough that every product and every partial sum is a whole number
below 2^53: the sums are exact in any order, so equal bits hold whatever order the reference sums in, and a misplaced
element (another row, column, tile, pair or batch entry) still shows, the values being spread over millions.  Every output
starts as NaN: what a launch must not write is NaN afterwards, and operands are NaN wherever a launch must not read."""

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
f64 = torch.float64
TILED = dict(gemm_strip=0, gemm_stream=0, gemm_skinny=0, gemm_fit=0)
NAN = float("nan")


def _form(m, args=""):
    return f"qs::gemm_fast_kernel<false, {4 if m % 128 == 0 else 2}, 4, true, false>" + (f"(qs::{args})" if args else "")


def _ints(shape, seed, span=1 << 12):
    """Whole numbers in [-span, span) as fp64 (k <= 256: |sum| < 2^8 * 2^24, far below 2^53)."""
    g = torch.Generator(device=DEV).manual_seed(seed)
    return torch.randint(-span, span, shape, device=DEV, generator=g).to(f64)


def _plain(K, m, n, k, batch, seed, ldc=None, accumulate=False):
    ldc = n if ldc is None else ldc
    A, B = _ints((m, k), seed), _ints((batch, k, n), seed + 1)
    want = torch.matmul(A, B)
    out = torch.full((batch, m + 1, ldc), NAN, dtype=f64, device=DEV)
    if accumulate:
        start = _ints((batch, m, n), seed + 2, span=1 << 30)
        out[:, :m, :n] = start
        want = want + start
    with K.tuning(**TILED):
        K.gemm_raw(f64, A, B, out, m, n, k, k, n, ldc, batch, 0, k * n, (m + 1) * ldc, accumulate=accumulate)
        dispatch = K.last_dispatch()
    where = f"m={m} n={n} k={k} batch={batch} ldc={ldc} accumulate={accumulate}"
    assert dispatch == _form(m), (where, dispatch)
    assert torch.equal(out[:, :m, :n], want), where
    assert bool(torch.isnan(out[:, :, n:]).all()) and bool(torch.isnan(out[:, m]).all()), where


@pytest.mark.parametrize("k", [16, 32])
def test_one_tile_of_one_and_two_stages(k):
    """k = 16: the tile's first stage is its last."""
    from quantum_systems_amd import kernels as K

    _plain(K, 128, 128, k, 1, seed=10 + k)


def test_more_tiles_than_one_workgroup_takes():
    """2 x 3 tiles x batch 3 under a walk of three tiles per workgroup: an epilogue is followed by a next tile; and the
    64-row form on the same columns."""
    from quantum_systems_amd import kernels as K

    with K.tuning(gemm_fast_persist=3):
        _plain(K, 256, 384, 256, 3, seed=20)
    _plain(K, 256, 384, 256, 3, seed=21)
    _plain(K, 64, 384, 48, 3, seed=22)


def test_output_pitch_larger_than_n():
    from quantum_systems_amd import kernels as K

    _plain(K, 128, 256, 32, 2, seed=30, ldc=256 + 24)


def test_accumulate_on_a_plain_product():
    from quantum_systems_amd import kernels as K

    _plain(K, 128, 256, 48, 2, seed=40, accumulate=True)
    _plain(K, 64, 128, 16, 1, seed=41, accumulate=True, ldc=128 + 8)


@pytest.mark.parametrize("mirror", [False, True])
def test_triangular_batch_and_its_mirror(mirror):
    """Grid 3, L = M = 128: pair (i, j >= i) is A[i, j] @ B; mirrored, pair (j, i) is its transpose; plain, j < i stays."""
    from quantum_systems_amd import kernels as K

    grid, L = 3, 128
    A, B = _ints((grid, grid, L, L), 50), _ints((L, L), 51)
    A[torch.tril(torch.ones((grid, grid), dtype=torch.bool, device=DEV), -1)] = NAN        # entries j < i are not read
    out = torch.full((grid, grid, L, L), NAN, dtype=f64, device=DEV)
    K.gemm_raw(f64, A, B, out, L, L, L, L, L, L, 0, L * L, 0, L * L, pairs=grid, mirror=mirror)
    # (the record names the mirror's overload; the plain triangular batch is recorded like the plain batch)
    assert K.last_dispatch() == _form(L, "FastPairsMirrorArgs" if mirror else "")
    for i in range(grid):
        for j in range(grid):
            if j >= i:
                assert torch.equal(out[i, j], torch.matmul(A[i, j], B)), (i, j)
            elif mirror:
                assert torch.equal(out[i, j], torch.matmul(A[j, i], B).T.contiguous()), (i, j)
            else:
                assert bool(torch.isnan(out[i, j]).all()), (i, j)


def _kept(side, S=16):
    """(side, side) bool: the blocks of R = 128 / S rows c and S columns d whose last column >= their first row."""
    R = 128 // S
    first_row = (torch.arange(side, device=DEV) // R) * R
    last_col = (torch.arange(side, device=DEV) // S) * S + S - 1
    return last_col[None, :] >= first_row[:, None]


@pytest.mark.parametrize("L", [64, 128])
def test_column_triangle_on_the_route_shapes(L):
    """The exchange route's two leading products at L = M: b' (m = M, k = L, columns (c, d), batch a, ldb = L^2) and a'
    (m = M, k = L, columns (q, c, d), ldb = M L^2).  Kept blocks are the product's bits, everything else is untouched; the
    second operand is NaN outside the kept blocks."""
    from quantum_systems_amd import kernels as K

    M = L
    kept1 = _kept(L).reshape(-1)
    Ct = _ints((M, L), 60 + L)
    for name, batch, stack in (("b'", L, 1), ("a'", 1, M)):
        n = stack * L * L
        kept = kept1.repeat(stack)
        clean = _ints((batch, L, n), 61 + L + stack)
        want = torch.matmul(Ct, clean)
        src = torch.where(kept, clean, torch.full_like(clean, NAN))
        del clean
        out = torch.full((batch, M, n), NAN, dtype=f64, device=DEV)
        K.matmul_upper(f64, Ct, src, out, M, L, stack, L, L, n, n, batch, 0, L * n, M * n)
        assert K.last_dispatch() == _form(M, "FastUpperArgs"), (name, K.last_dispatch())
        assert torch.equal(out[:, :, kept], want[:, :, kept]), name
        assert bool(torch.isnan(out[:, :, ~kept]).all()), name
        del want, src, out


def test_lower_blocks_from_the_mirror_pair():
    """Grid 3, L = M = 128: the blocks (G, J < G) of pair (i, j) come from the blocks (J, G) of entry (j, i), turned; every
    block below the block diagonal, and the diagonal blocks of the entries j < i, are NaN."""
    from quantum_systems_amd import kernels as K

    grid, L, nb = 3, 128, 8
    S, B = _ints((grid, grid, L, L), 70), _ints((L, L), 71)
    lower_blocks = torch.kron(torch.tril(torch.ones((nb, nb), device=DEV), -1), torch.ones((16, 16), device=DEV)).bool()
    diag_blocks = torch.kron(torch.eye(nb, device=DEV), torch.ones((16, 16), device=DEV)).bool()
    P = torch.where(lower_blocks, torch.full_like(S, NAN), S)
    for i in range(grid):
        for j in range(i):
            P[i, j] = torch.where(diag_blocks, torch.full_like(P[i, j], NAN), P[i, j])
    out = torch.full((grid, grid, L, L), NAN, dtype=f64, device=DEV)
    K.gemm_raw(f64, P, B, out, L, L, L, L, L, L, 0, L * L, 0, L * L, pairs=grid, lower=True)
    assert K.last_dispatch() == _form(L, "FastPairsLowerArgs")
    for i in range(grid):
        for j in range(grid):
            if j >= i:
                full = torch.where(lower_blocks, S[j, i].T, S[i, j])
                assert torch.equal(out[i, j], torch.matmul(full, B)), (i, j)
            else:
                assert bool(torch.isnan(out[i, j]).all()), (i, j)
