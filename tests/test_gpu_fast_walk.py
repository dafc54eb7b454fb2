"""The tile walk of the VALU-free product kernel (qs_gemm_fast.hip) at sizes of a few hundred kilobytes.

A persistent workgroup of ``gemm_fast_kernel`` walks its tiles as ONE flat stream of stages: the load cursor runs three
stages (register-staged forms) or two (LDS-DMA forms) ahead of the multiplication, crosses into the next tile -- with a
short K into the second or third tile after it -- while the current tile still multiplies; the edge forms zero the K tail
by a stage counter of their own that has to stay in step with that cursor, and the DMA forms count the previous tile's
epilogue stores in their wait for the next stage.  On the device the host launches min(2 CUs, tiles) workgroups for any
tile list of at most 4096 tiles, so a product small enough for a test runs one tile per workgroup and never walks.  The
tuning key ``gemm_fast_persist >= 3`` sets the tiles per workgroup instead (P = ceil(total / N) workgroups, rounded up
to a multiple of 8 and capped at total; workgroup b takes ceil((total - b) / P) tiles): 30 tiles then walk on 8
workgroups.

All 26 instantiations (21 edge forms under ``gemm_fast=3``: the nine fp64 shapes with 16-byte and with 8-byte items and
the three complex128 shapes; 5 exact forms under ``gemm_fast=1``) walk here, at nk = 1 ... 4 stages per tile, plain and
accumulating, with a shared A (tiles grouped along m) and with one A per batch entry (grouped along n), the instantiation
asserted from the dispatch log.  Every case asserts

1. error / bound <= 1 on every element against the numpy.longdouble product of the same strided views, the bound
   gamma_(k+2) (|A| |B| + |C0|) of an inner product of length k in any order plus the accumulation (C0 only when the
   call accumulates; times 2 sqrt 2 for complex products) -- derived as tests/_blocks_ref.py, not tuned;
2. ``torch.equal`` with the general kernel (``gemm_fast=0``): the same MFMA order along k, the documented promise;
3. ``torch.equal`` between all ``gemm_fast_persist`` settings: one tile per workgroup, 2, 4 and 9 tiles;
4. the sentinel of the padding columns of C (ldc = n + 3; n + 4 where every stride has to be even) and of the row
   between two batch slices is unchanged.

The padding of the operands is NaN throughout: the columns k ... lda-1 of A and the row below every B[t] are what the K
tail of a tile's last stage loads, the columns n ... ldb-1 of B and the rows of the NEXT entry of A are what a border
tile loads; none of it may reach a stored element.

The worst error / bound per instantiation is printed and, when QS_FAST_WALK_OUT names a file, appended there with the
dispatch string (profiles/r15_fast_walk.txt holds the figures measured on the MI355X)."""

import os

import numpy as np
import pytest
import torch
from hypothesis import HealthCheck, given, settings
from hypothesis import strategies as st

from _blocks_ref import gamma

pytestmark = pytest.mark.gpu

OTHER_ROUTES_OFF = dict(gemm_strip=0, gemm_stream=0, gemm_skinny=0, gemm_fit=0)
SENTINEL = -7777.25
F64_SHAPES = {1: (4, 4), 2: (2, 4), 3: (4, 2), 4: (2, 2), 5: (3, 4), 6: (5, 2), 7: (6, 2), 8: (7, 2), 9: (3, 2)}
C128_SHAPES = {1: (4, 2), 2: (2, 4), 3: (2, 2)}


class Form:
    """One instantiation gemm_fast_kernel<CX, TM, TN, VEC, EDGE> and the tuning keys that select it."""

    def __init__(self, cx, tm, tn, vec, edge, shape=0):
        self.cx, self.tm, self.tn, self.vec, self.edge, self.shape = cx, tm, tn, vec, edge, shape
        self.bm, self.bn, self.kt = 32 * tm, 32 * tn, 8 if cx else 16
        self.id = f"{'c128' if cx else 'f64'}-{tm}x{tn}-{'v16' if vec else 'v8'}-{'edge' if edge else 'exact'}"

    def knobs(self):
        keys = dict(OTHER_ROUTES_OFF, gemm_fast=3 if self.edge else 1)
        if self.edge:
            keys["gemm_fast_shape"] = self.shape
        if not self.vec:
            keys["gemm_fast_unaligned"] = 0
        return keys


def kernel_name(cx, tm, tn, vec, edge):
    b = {True: "true", False: "false"}
    return f"qs::gemm_fast_kernel<{b[cx]}, {tm}, {tn}, {b[vec]}, {b[edge]}>"


FORMS = ([Form(False, *F64_SHAPES[s], True, True, s) for s in range(1, 10)] +
         [Form(False, *F64_SHAPES[s], False, True, s) for s in range(1, 10)] +
         [Form(True, *C128_SHAPES[s], True, True, s) for s in range(1, 4)] +
         [Form(False, 4, 4, True, False), Form(False, 2, 4, True, False),
          Form(True, 4, 2, True, False), Form(True, 2, 4, True, False), Form(True, 2, 2, True, False)])
assert len(FORMS) == 26 and len({f.id for f in FORMS}) == 26


def expected_kernel(form, m, n, k, even):
    """The instantiation gemm_fast_try launches under ``form.knobs()`` (its rule restated): whole-tile extents take an
    exact form first, whatever shape is forced; ``even`` = every stride and n even (the bases of a test are aligned)."""
    cx = form.cx
    vec = cx or even or form.vec
    if not cx and vec and k % 16 == 0:
        if m % 128 == 0 and n % 128 == 0:
            return kernel_name(False, 4, 4, True, False)
        if m % 64 == 0 and n % 128 == 0:
            return kernel_name(False, 2, 4, True, False)
    if cx and k % 8 == 0:
        if m >= n and m % 128 == 0 and n % 64 == 0:
            return kernel_name(True, 4, 2, True, False)
        if m % 64 == 0 and n % 128 == 0:
            return kernel_name(True, 2, 4, True, False)
        if m % 128 == 0 and n % 64 == 0:
            return kernel_name(True, 4, 2, True, False)
        if m % 64 == 0 and n % 64 == 0:
            return kernel_name(True, 2, 2, True, False)
    if not form.edge:
        return None          # (not a whole number of any exact form's tiles: no test here draws such extents)
    return kernel_name(cx, form.tm, form.tn, vec, True)


def walk(total, persist):
    """(workgroups, most and fewest tiles of one workgroup) of launch_fast for ``gemm_fast_persist`` = 0 or >= 3 and a
    tile list far below the device's 2 CUs x 8."""
    if persist == 0:
        return total, 1, 1
    p = min(total, (-(-total // persist) + 7) // 8 * 8)
    return p, -(-total // p), total // p


def test_walk_geometry_of_the_designed_cases():
    # 30 tiles: 4 per workgroup -> 8 workgroups, six with 4 tiles and two with 3; 3 -> 16 workgroups, fourteen with 2 and
    # two with 1; 72 tiles at 9 per workgroup -> 8 workgroups with 9 each
    assert walk(30, 4) == (8, 4, 3) and [-(-(30 - b) // 8) for b in range(8)] == [4] * 6 + [3] * 2
    assert walk(30, 3) == (16, 2, 1) and [-(-(30 - b) // 16) for b in range(16)] == [2] * 14 + [1] * 2
    assert walk(72, 9) == (8, 9, 9) and walk(30, 0) == (30, 1, 1)


class Case:
    """Operands of one product on the host (padding NaN, sentinel in C's padding) and its long-double reference."""

    def __init__(self, cx, m, n, k, batch, lda, ldb, ldc, shared_a, seed, poison=False):
        self.cx, self.m, self.n, self.k, self.batch = cx, m, n, k, batch
        self.lda, self.ldb, self.ldc, self.shared_a = lda, ldb, ldc, shared_a
        rng = np.random.default_rng(seed)

        def rnd(*shape):
            x = rng.standard_normal(shape)
            return x + 1j * rng.standard_normal(shape) if cx else x

        na = 1 if shared_a else batch
        # A: (na, m, lda) packed, so the rows >= m of a border tile are the next entry's; B and C: one row between slices
        self.A = np.full((na, m, lda), np.nan, dtype=np.complex128 if cx else np.float64)
        self.A[:, :, :k] = rnd(na, m, k)
        self.B = np.full((batch, k + 1, ldb), np.nan, dtype=self.A.dtype)
        self.B[:, :k, :n] = rnd(batch, k, n)
        self.C0 = np.full((batch, m + 1, ldc), SENTINEL, dtype=self.A.dtype)
        self.C0[:, :m, :n] = rnd(batch, m, n)
        if poison:
            self.A[1 % na, 0, k // 2] = np.nan
            self.B[:, :k, n:] = np.inf
        self.sa, self.sb, self.sc = (0 if shared_a else m * lda), (k + 1) * ldb, (m + 1) * ldc
        self.even = not any(x & 1 for x in (lda, ldb, ldc, self.sa, self.sb, self.sc, n))
        self.dt = torch.complex128 if cx else torch.float64
        self.dA, self.dB, self.dC0 = (torch.from_numpy(x).cuda() for x in (self.A, self.B, self.C0))
        ld = np.clongdouble if cx else np.longdouble
        a, b = self.A[:, :, :k], self.B[:, :k, :n]
        with np.errstate(invalid="ignore"):
            self.prod = np.matmul(a.astype(ld), b.astype(ld))                       # (batch, m, n), A broadcast when shared
        self.abs_prod = np.matmul(np.abs(a), np.abs(b))

    def run(self, K, accumulate):
        out = self.dC0.clone()
        K.gemm_raw(self.dt, self.dA, self.dB, out, self.m, self.n, self.k, self.lda, self.ldb, self.ldc, self.batch,
                   self.sa, self.sb, self.sc, accumulate)
        return out

    def ratio(self, out, accumulate):
        """Largest error / bound of the stored elements; asserts that nothing else was written."""
        got = out.cpu().numpy()
        m, n = self.m, self.n
        assert np.array_equal(got[:, m:, :], self.C0[:, m:, :]) and np.array_equal(got[:, :, n:], self.C0[:, :, n:]), \
            "the sentinel around C was overwritten"
        c0 = self.C0[:, :m, :n]
        exact = self.prod + c0 if accumulate else self.prod
        bound = gamma(self.k + 2) * (self.abs_prod + (np.abs(c0) if accumulate else 0.0)) * (2.0 * np.sqrt(2.0) if self.cx else 1.0)
        err = np.abs(got[:, :m, :n] - exact)
        nan_ref = np.isnan(exact.real) | np.isnan(exact.imag)
        nan_got = np.isnan(got[:, :m, :n].real) | np.isnan(got[:, :m, :n].imag)
        assert np.array_equal(nan_got, nan_ref), "NaN pattern differs from the reference's"
        ok = ~nan_ref
        return float((err[ok] / bound[ok]).max())


@pytest.fixture(scope="module")
def K():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    from quantum_systems_amd import kernels

    return kernels


WORST = {}


def _note(form, ratio, ran):
    key = (form.id, ran)
    WORST[key] = max(WORST.get(key, 0.0), ratio)


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    lines = [f"fast walk {fid}: largest error / bound = {r:.4f}  [{ran}]" for (fid, ran), r in sorted(WORST.items())]
    print("\n" + "\n".join(lines))
    if os.environ.get("QS_FAST_WALK_OUT"):
        with open(os.environ["QS_FAST_WALK_OUT"], "a") as f:
            f.write("\n".join(lines) + "\n")


def fast_runs(K, form, case, persists, accumulate, name):
    outs = []
    for persist in persists:
        with K.tuning(**form.knobs(), gemm_fast_persist=persist):
            outs.append(case.run(K, accumulate))
            ran = K.last_dispatch()
        assert ran.split(" x")[0] == name, (form.id, persist, ran)
    return outs


def general_run(K, case, accumulate):
    with K.tuning(**OTHER_ROUTES_OFF, gemm_fast=0):
        out = case.run(K, accumulate)
        assert "qs::gemm_kernel<" in K.last_dispatch(), K.last_dispatch()
    return out


def check(K, form, case, persists, tag):
    name = expected_kernel(form, case.m, case.n, case.k, case.even)
    worst = 0.0
    for accumulate in (False, True):
        outs = fast_runs(K, form, case, persists, accumulate, name)
        general = general_run(K, case, accumulate)
        torch.cuda.synchronize()
        assert torch.equal(outs[-1], general), (form.id, tag, accumulate, "bits differ from the general kernel")
        for persist, out in zip(persists[:-1], outs[:-1]):
            assert torch.equal(out, outs[-1]), (form.id, tag, accumulate, f"gemm_fast_persist={persist} differs")
        r = case.ratio(outs[-1], accumulate)
        print(f"fast walk {form.id} {tag} accumulate={int(accumulate)}: max error / bound = {r:.4f}")
        assert r <= 1.0, (form.id, tag, accumulate, r)
        worst = max(worst, r)
    _note(form, worst, name)
    return name


def extents(form, twin, shared_a):
    """Smallest extents that still walk.  Edge forms: three tile rows, two tile columns, both borders partial (the even
    twin: even extents).  Exact forms: 3 x 2 tiles; where those extents select another instantiation (the 64-row forms
    with one A per entry need m >= n for the grouping along n, and 192 x 128 complex is a <2, 4> product) 5 x 2 or 3 x 3."""
    if form.edge:
        return (2 * form.bm + 5, form.bn + 3) if twin == "odd" else (2 * form.bm + 6, form.bn + 4)
    if form.cx and (form.tm, form.tn) == (2, 2):
        return 3 * form.bm, 3 * form.bn
    if (form.tm, form.tn) == (2, 4) and not shared_a:
        return 5 * form.bm, 2 * form.bn
    return 3 * form.bm, 2 * form.bn


def strides(form, twin, n, k):
    """(lda, ldb, ldc).  odd twin: odd lda and ldb, ldc = n + 3.  even twin: every stride even (16-byte rows), ldc = n + 4
    -- except in the 8-byte forms, which an even layout would not select: odd strides there too."""
    if twin == "odd" or not form.vec:
        return k + 1 + k % 2, n + 1 + n % 2, n + 3
    return k + 2 - k % 2, n + 2, n + 4


def k_values(form):
    kt = form.kt
    return [3, kt, kt + 1, 2 * kt, 3 * kt - 2, 3 * kt + 5] if form.edge else [kt, 2 * kt, 3 * kt]


@pytest.mark.parametrize("shared_a", [True, False], ids=["sharedA", "perEntryA"])
@pytest.mark.parametrize("form", FORMS, ids=[f.id for f in FORMS])
def test_walk_of_thirty_tiles(K, form, shared_a):
    for twin in ("odd", "even"):
        m, n = extents(form, twin, shared_a)
        for k in k_values(form):
            lda, ldb, ldc = strides(form, twin, n, k)
            case = Case(form.cx, m, n, k, 5, lda, ldb, ldc, shared_a, seed=1000 * form.bm + 10 * k + shared_a)
            tiles = -(-m // form.bm) * -(-n // form.bn) * 5
            assert walk(tiles, 4)[1] >= 3, tiles
            assert shared_a or m >= n                # one A per entry: the tiles are grouped along n
            name = check(K, form, case, [0, 3, 4], f"{twin} m={m} n={n} k={k}")
            assert name == kernel_name(form.cx, form.tm, form.tn, form.vec, form.edge), name


@pytest.mark.parametrize("form", FORMS, ids=[f.id for f in FORMS])
def test_walk_of_nine_tiles_per_workgroup(K, form):
    # 72 tiles (batch 12) on 8 workgroups; odd stage counts too (nk = 3: 27 stages)
    kt = form.kt
    m, n = extents(form, "odd", True)
    for k in ([kt + 1, 3 * kt - 2] if form.edge else [kt, 3 * kt]):
        lda, ldb, ldc = strides(form, "odd", n, k)
        case = Case(form.cx, m, n, k, 12, lda, ldb, ldc, True, seed=77 * form.bm + k)
        tiles = -(-m // form.bm) * -(-n // form.bn) * 12
        assert walk(tiles, 9)[2] >= 6, tiles       # (fewest tiles of a workgroup)
        check(K, form, case, [0, 9], f"long m={m} n={n} k={k}")


@pytest.mark.parametrize("form", [FORMS[0], FORMS[9], FORMS[18]], ids=lambda f: f.id)
def test_non_finite_neighbours_mid_walk(K, form):
    # One A per entry, packed (sa = m lda): the rows >= m of entry 0's border tiles are entry 1's first rows, and row 0 of
    # entry 1 holds a NaN; the columns >= n of B hold Inf.  Only row 0 of C[1] may be NaN -- as in the reference.
    m, n = extents(form, "odd", False)
    k = form.kt + 1
    lda, ldb, ldc = strides(form, "odd", n, k)
    case = Case(form.cx, m, n, k, 5, lda, ldb, ldc, False, seed=5, poison=True)
    name = expected_kernel(form, m, n, k, case.even)
    for accumulate in (False, True):
        outs = fast_runs(K, form, case, [0, 4], accumulate, name)
        for out in outs:
            r = case.ratio(out, accumulate)
            assert r <= 1.0, (form.id, accumulate, r)
        got = outs[-1][:, :m, :n]
        nan = torch.isnan(torch.view_as_real(got)).any(-1) if form.cx else torch.isnan(got)
        assert bool(nan[1, 0].all()) and int(nan.sum()) == n


@st.composite
def walk_case(draw):
    form = FORMS[draw(st.integers(0, len(FORMS) - 1))]
    persist = draw(st.sampled_from([0, 3, 4, 5, 9]))
    if form.edge:
        m, n, k = draw(st.integers(1, 3 * form.bm)), draw(st.integers(1, 3 * form.bn)), draw(st.integers(1, 70))
    else:
        m, n = form.bm * draw(st.integers(1, 3)), form.bn * draw(st.integers(1, 3))
        k = form.kt * draw(st.integers(1, 64 // form.kt))
    batch = draw(st.integers(1, 12))
    pads = draw(st.integers(0, 3)), draw(st.integers(0, 3)), draw(st.integers(0, 3))
    return form, persist, m, n, k, batch, pads, draw(st.booleans()), draw(st.booleans()), draw(st.integers(0, 2**31 - 1))


@given(walk_case())
@settings(max_examples=int(os.environ.get("QS_HYP_EXAMPLES", "60")), deadline=None, suppress_health_check=list(HealthCheck))
def test_random_walks_match_long_double_and_the_general_kernel(case):
    from quantum_systems_amd import kernels as K

    form, persist, m, n, k, batch, (pa, pb, pc), shared_a, accumulate, seed = case
    c = Case(form.cx, m, n, k, batch, k + pa, n + pb, n + pc, shared_a, seed)
    name = expected_kernel(form, m, n, k, c.even)
    with K.tuning(**form.knobs(), gemm_fast_persist=persist):
        out = c.run(K, accumulate)
        ran = K.last_dispatch()
    assert name is not None and ran.split(" x")[0] == name, (form.id, m, n, k, ran)
    general = general_run(K, c, accumulate)
    torch.cuda.synchronize()
    assert torch.equal(out, general), (form.id, persist, m, n, k, batch, shared_a, accumulate)
    r = c.ratio(out, accumulate)
    assert r <= 1.0, (form.id, persist, m, n, k, batch, shared_a, accumulate, r)
