"""The triangular batch of the products (``qs_matmul_pairs``: entry t of the batch is the t-th pair (i, j >= i) of an
n x n grid, its operands at the flat index i n + j) on both tiled kernels, at grids n = 1, 2, 5, 9.

The tuning knobs of tests/test_gpu_fast_walk.py select the instantiation, which is asserted from the dispatch: the exact
fp64 forms <4, 4> (128 x 128 and 256 x 128) and <2, 4> (64 x 128), an fp64 edge form with 16-byte items (even and odd
strides) and with 8-byte items (odd strides) at m = 40, n = 36, k = 20, a complex128 exact and edge form, and the general
kernel (``gemm_fast=0``).  Each runs with a shared A (``stride_a = 0``, the shape of the exchange route's c contraction)
and with a shared B (``stride_b = 0``, its d contraction), and with ``gemm_fast_persist`` 0, 3 and 9: grid 5 with two
tiles per pair is 30 tiles on 8 workgroups, so one workgroup's walk crosses pair rows (the remap is in the tile decode
that both the load cursor and the epilogue use).

Every case asserts
1. ``torch.equal`` (the whole output buffer) with a loop of plain ``qs_matmul`` calls, one per row i over its entries
   j >= i, under the same knobs;
2. error / bound <= 1 against the numpy.longdouble product, the bound gamma_(k+2) |A| |B| of an inner product of length
   k in any order (times 2 sqrt 2 for complex products), as tests/test_gpu_fast_walk.py and tests/_blocks_ref.py derive it;
3. no stray reads or writes: the entries j < i of the non-shared operands are NaN (like every padding element of the
   operands), the entries j < i of the output and all of its padding (columns n ... ldc-1, the row between two entries)
   hold a sentinel; no NaN reaches an output and every sentinel is intact."""

import numpy as np
import pytest
import torch

from _blocks_ref import gamma

pytestmark = pytest.mark.gpu

OTHER_ROUTES_OFF = dict(gemm_strip=0, gemm_stream=0, gemm_skinny=0, gemm_fit=0)
SENTINEL = -7777.25
GRIDS = [1, 2, 5, 9]


def fast(cx, tm, tn, vec, edge):
    b = {True: "true", False: "false"}
    return f"qs::gemm_fast_kernel<{b[cx]}, {tm}, {tn}, {b[vec]}, {b[edge]}>"


class Config:
    def __init__(self, cid, cx, m, n, k, lds, knobs, kernel, persists=(0, 3, 9)):
        self.id, self.cx, self.m, self.n, self.k, self.lds = cid, cx, m, n, k, lds
        self.knobs, self.kernel, self.persists = dict(OTHER_ROUTES_OFF, **knobs), kernel, persists


def _exact(cid, cx, m, n, k, kernel):
    return Config(f"{cid}-{m}x{n}-k{k}", cx, m, n, k, (k + 2, n + 2, n + 4), dict(gemm_fast=1), kernel)


EDGE = dict(m=40, n=36, k=20)
CONFIGS = (
    [_exact("f64-exact44", False, m, 128, k, fast(False, 4, 4, True, False)) for m in (128, 256) for k in (16, 32)] +
    [_exact("f64-exact24", False, 64, 128, k, fast(False, 2, 4, True, False)) for k in (16, 32)] +
    [Config("f64-edge22-v16-even", False, **EDGE, lds=(22, 38, 40), knobs=dict(gemm_fast=3, gemm_fast_shape=4),
            kernel=fast(False, 2, 2, True, True)),
     Config("f64-edge22-v16-odd", False, **EDGE, lds=(21, 37, 39), knobs=dict(gemm_fast=3, gemm_fast_shape=4),
            kernel=fast(False, 2, 2, True, True)),
     Config("f64-edge22-v8-odd", False, **EDGE, lds=(21, 37, 39),
            knobs=dict(gemm_fast=3, gemm_fast_shape=4, gemm_fast_unaligned=0), kernel=fast(False, 2, 2, False, True))] +
    [_exact("c128-exact22", True, 64, 64, k, fast(True, 2, 2, True, False)) for k in (8, 16)] +
    [Config("c128-edge22", True, **EDGE, lds=(21, 37, 39), knobs=dict(gemm_fast=3, gemm_fast_shape=3),
            kernel=fast(True, 2, 2, True, True)),
     Config("f64-general", False, **EDGE, lds=(21, 37, 39), knobs=dict(gemm_fast=0), kernel="qs::gemm_kernel<", persists=(1,)),
     Config("c128-general", True, **EDGE, lds=(21, 37, 39), knobs=dict(gemm_fast=0), kernel="qs::gemm_kernel<", persists=(1,))]
)


class Case:
    """Operands of one pairs product on an n x n grid of entries: NaN in every padding element and in the entries j < i
    of the operand that is not shared, the sentinel in C outside the stored elements of the pairs j >= i."""

    def __init__(self, cfg, grid, shared, seed):
        cx, m, n, k = cfg.cx, cfg.m, cfg.n, cfg.k
        lda, ldb, ldc = cfg.lds
        rng = np.random.default_rng(seed)
        dt = np.complex128 if cx else np.float64

        def rnd(*shape):
            x = rng.standard_normal(shape)
            return x + 1j * rng.standard_normal(shape) if cx else x

        self.cfg, self.grid, self.shared = cfg, grid, shared
        nn = grid * grid
        ii, jj = np.divmod(np.arange(nn), grid)
        self.upper = jj >= ii
        na, nb = (1, nn) if shared == "A" else (nn, 1)
        self.A = np.full((na, m, lda), np.nan, dtype=dt)
        self.A[:, :, :k] = rnd(na, m, k)
        self.B = np.full((nb, k + 1, ldb), np.nan, dtype=dt)
        self.B[:, :k, :n] = rnd(nb, k, n)
        if shared == "A":
            self.B[~self.upper] = np.nan
        else:
            self.A[~self.upper] = np.nan
        self.C0 = np.full((nn, m + 1, ldc), SENTINEL, dtype=dt)
        self.sa = 0 if shared == "A" else m * lda
        self.sb = 0 if shared == "B" else (k + 1) * ldb
        self.sc = (m + 1) * ldc
        self.dt = torch.complex128 if cx else torch.float64
        self.dA, self.dB, self.dC0 = (torch.from_numpy(x).cuda() for x in (self.A, self.B, self.C0))
        ld = np.clongdouble if cx else np.longdouble
        a = self.A[:, :, :k] if shared == "A" else self.A[self.upper][:, :, :k]
        b = self.B[:, :k, :n] if shared == "B" else self.B[self.upper][:, :k, :n]
        self.prod = np.matmul(a.astype(ld), b.astype(ld))              # (pairs, m, n), the shared operand broadcast
        self.abs_prod = np.matmul(np.abs(a), np.abs(b))

    def args(self):
        c = self.cfg
        return (self.dt, self.dA, self.dB), (c.m, c.n, c.k, *c.lds)

    def run_pairs(self, K):
        out = self.dC0.clone()
        (dt, A, B), ext = self.args()
        K.gemm_raw(dt, A, B, out, *ext, 0, self.sa, self.sb, self.sc, pairs=self.grid)
        return out, K.last_dispatch()

    def run_rows(self, K):
        """One plain batched product per row i: its entries j >= i are contiguous in the flat index from i n + i."""
        out = self.dC0.clone()
        (dt, A, B), ext = self.args()
        g = self.grid
        for i in range(g):
            f = i * g + i
            K.gemm_raw(dt, A, B, out, *ext, g - i, self.sa, self.sb, self.sc,
                       a_off=f * self.sa, b_off=f * self.sb, c_off=f * self.sc)
        return out

    def ratio(self, out):
        got = out.cpu().numpy()
        m, n = self.cfg.m, self.cfg.n
        assert np.array_equal(got[~self.upper], self.C0[~self.upper]), "an entry j < i of the output was written"
        assert np.array_equal(got[:, m:, :], self.C0[:, m:, :]) and np.array_equal(got[:, :, n:], self.C0[:, :, n:]), \
            "the sentinel around C was overwritten"
        stored = got[self.upper][:, :m, :n]
        assert not np.isnan(stored.real).any() and not np.isnan(stored.imag).any(), "a NaN reached the output"
        bound = gamma(self.cfg.k + 2) * self.abs_prod * (2.0 * np.sqrt(2.0) if self.cfg.cx else 1.0)
        return float((np.abs(stored - self.prod) / bound).max())


@pytest.fixture(scope="module")
def K():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    from quantum_systems_amd import kernels

    return kernels


@pytest.mark.parametrize("grid", GRIDS)
@pytest.mark.parametrize("cfg", CONFIGS, ids=[c.id for c in CONFIGS])
def test_pairs_product(K, cfg, grid):
    for shared in ("A", "B"):
        case = Case(cfg, grid, shared, seed=1000 * grid + cfg.m + cfg.k + (shared == "A"))
        assert int(case.upper.sum()) == grid * (grid + 1) // 2
        for persist in cfg.persists:
            with K.tuning(**cfg.knobs, gemm_fast_persist=persist):
                out, ran = case.run_pairs(K)
                rows = case.run_rows(K)
            torch.cuda.synchronize()
            name = ran.split(" x")[0]
            assert ";" not in ran and (name == cfg.kernel or (cfg.kernel.endswith("<") and name.startswith(cfg.kernel))), \
                (cfg.id, grid, shared, persist, ran)
            assert torch.equal(out, rows), (cfg.id, grid, shared, persist, "bits differ from the per-row launches")
            r = case.ratio(out)
            print(f"pairs product {cfg.id} grid={grid} shared{shared} persist={persist}: max error / bound = {r:.4f}")
            assert r <= 1.0, (cfg.id, grid, shared, persist, r)

