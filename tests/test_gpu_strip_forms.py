"""Every instantiation of the strip kernel (qs_gemm_strip.hip) at sizes of a few hundred kilobytes, its tile walk included.

``gemm_strip_kernel<CX, FORM, T, WN, SETS>`` is compiled 68 times: fp64 FORM 0 / 1 with T = 1 ... 16 blocks of 16 along
the small extent at WN = 1 (tiles of 128 along the big extent) and T = 1 ... 10 again at WN = 2 (tiles of 256, FORM 0
with the paired-column loads and 16-byte stores of ``kPair``), complex128 FORM 0 / 1 with T = 1 ... 8.  The host selects
the 256-wide form by itself only from 4 x CUs such tiles (262144 rows or virtual columns), and a workgroup walks to a
second tile only past one tile per CU.  Two tuning keys bring both down to a test's size: ``gemm_strip_wide`` (1 never,
2 wherever the form exists) and ``gemm_strip_wgs`` (at most that many workgroups: 3 workgroups walk two tiles each of
six).  The instantiation is asserted from the dispatch log, SETS = ((CX ? 2 : 1) T WN <= 12 ? 2 : 1) included.

Layout of every case but the aligned ones: bases one element past the allocation (fp64: 8-byte but not 16-byte
aligned), odd lda, ldb, ldc and odd batch strides (complex128: padded ones).  Everything the kernel may over-read is NaN:
the columns k ... lda-1 of A and the slack behind it, the columns n ... ldb-1 of B (the dummy virtual column of an odd
segment reads B[row, W]), one row below each B[t] (the K tail of a tile's last stage) and the gap between batch slices.
Everything of C that must not be written holds a sentinel: the columns n ... ldc-1, one extra row per entry, the gaps
between entries and the element before the base.

Every case asserts
1. error / bound <= 1 on every stored element against the numpy.longdouble product of the same strided views, the bound
   gamma_(k+2) |A| |B| of an inner product of length k in any order (times 2 sqrt 2 for complex products) -- derived as
   tests/_blocks_ref.py and tests/test_gpu_fast_walk.py, not tuned;
2. ``torch.equal`` on the WHOLE C buffer with the general kernel (every other route off): the same MFMA order along k,
   the documented promise;
3. ``torch.equal`` between all ``gemm_strip_wgs`` settings and between WN = 1 and WN = 2 of the same product;
4. no NaN in a stored element, every sentinel intact.

The worst error / bound per instantiation is printed and, when QS_STRIP_FORMS_OUT names a file, appended there with the
dispatch string (profiles/strip_forms.txt holds the figures measured on the MI355X)."""

import functools
import os

import numpy as np
import pytest
import torch
from hypothesis import HealthCheck, given, settings
from hypothesis import strategies as st

from _product_case import Case, cdiv, even_layout, odd_layout

pytestmark = pytest.mark.gpu

STRIP = dict(gemm_strip=2, gemm_fast=0, gemm_stream=0, gemm_skinny=0, gemm_fit=0)
GENERAL = dict(gemm_strip=0, gemm_fast=0, gemm_stream=0, gemm_skinny=0, gemm_fit=0)
MAX_T = {False: 16, True: 8}
WIDE_MAX_T = 10


def kernel_name(cx, form, t, wn):
    sets = 2 if (2 if cx else 1) * t * wn <= 12 else 1
    return f"qs::gemm_strip_kernel<{'true' if cx else 'false'}, {form}, {t}, {wn}, {sets}>"


ALL_NAMES = ({kernel_name(False, f, t, 1) for f in (0, 1) for t in range(1, 17)} |
             {kernel_name(False, f, t, 2) for f in (0, 1) for t in range(1, 11)} |
             {kernel_name(True, f, t, 1) for f in (0, 1) for t in range(1, 9)})
assert len(ALL_NAMES) == 68


def blocks_and_tiles(cx, small):
    """(T, tiles along the small extent) of gemm_strip_try, its rule restated: the fewest tiles of at most 16 (complex128
    8) blocks, equally high; fp64 with an even number of 12 ... 16 blocks: two tiles of half the height."""
    t = cdiv(small, 16)
    ns = cdiv(t, MAX_T[cx])
    if not cx and ns == 1 and t >= 12 and t % 2 == 0:
        ns = 2
    return cdiv(t, ns), ns


def form_of(m, n, batch):
    """FORM of gemm_strip_try for a shared A (stride_a = 0)."""
    return 0 if batch > 1 or n >= m else 1


def small_of(cx, t):
    """Smallest extent with a partial last block that selects T = t directly; fp64 T = 12, 14, 16 exist only as two
    tiles (the second one with a partial last block)."""
    return 32 * t - 3 if (not cx and t in (12, 14, 16)) else 16 * t - 3


for _cx in (False, True):
    for _t in range(1, MAX_T[_cx] + 1):
        assert blocks_and_tiles(_cx, small_of(_cx, _t)) == (_t, 2 if (not _cx and _t in (12, 14, 16)) else 1)
assert blocks_and_tiles(False, 525) == (11, 3) and blocks_and_tiles(False, 1021) == (16, 4)
assert blocks_and_tiles(True, 200) == (7, 2) and blocks_and_tiles(True, 509) == (8, 4)


@functools.lru_cache(maxsize=4)
def make_case(cx, m, n, k, batch, even=False):
    """The case of a product, built (and its reference computed) once and shared by the tests that need it."""
    layout = (even_layout if even else odd_layout)(cx, m, n, k)
    return Case(cx, m, n, k, batch, layout, seed=(m * 1000003 + n * 1009 + k * 17 + batch) * 2 + cx)


@pytest.fixture(scope="module")
def K():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    from quantum_systems_amd import kernels

    return kernels


WORST = {}


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    lines = [f"strip forms {name}: largest error / bound = {r:.4f}" for name, r in sorted(WORST.items())]
    print("\n" + "\n".join(lines) + f"\nstrip forms: {len(WORST)} instantiations")
    if os.environ.get("QS_STRIP_FORMS_OUT"):
        with open(os.environ["QS_STRIP_FORMS_OUT"], "a") as f:
            f.write("\n".join(lines) + "\n")


def expected(case, wide):
    """The instantiation gemm_strip_try launches for ``case`` under ``gemm_strip_wide`` = wide (a test's tile list is far
    too short for the automatic rule to choose the 256-wide form)."""
    form = form_of(case.m, case.n, case.batch)
    t, ns = blocks_and_tiles(case.cx, case.n if form else case.m)
    wn = 2 if (wide == 2 and not case.cx and t <= WIDE_MAX_T) else 1
    return kernel_name(case.cx, form, t, wn), form, t, wn, ns


def tiles_of(case, wide):
    _, form, _, wn, ns = expected(case, wide)
    wp = case.n + (case.n & 1 if not case.cx else 0)
    return cdiv(case.m if form else wp * case.batch, 128 * wn) * ns


def general_run(K, case):
    with K.tuning(**GENERAL):
        out = case.run(K)
        assert K.last_dispatch().startswith("qs::gemm_kernel<"), K.last_dispatch()
    return out


def check(K, case, wides, wgss, tag, general=None):
    """Assertions 1 - 4 for every (gemm_strip_wide, gemm_strip_wgs) of the lists; the names that ran."""
    if general is None:
        general = general_run(K, case)
    names = []
    judged, r = None, 0.0
    for wide in wides:
        name = expected(case, wide)[0]
        for wgs in wgss:
            with K.tuning(**STRIP, gemm_strip_wide=wide, gemm_strip_wgs=wgs):
                out = case.run(K)
                ran = K.last_dispatch()
            what = (tag, name, f"wide={wide}", f"wgs={wgs}", f"tiles={tiles_of(case, wide)}")
            assert ran.split(" x")[0] == name, (*what, ran)
            torch.cuda.synchronize()
            if judged is None or not torch.equal(out, judged):      # (a buffer with the bits of a judged one: the same verdict)
                r = case.ratio(out)
                judged = out
            print(f"strip forms {name} {tag} wide={wide} wgs={wgs}: max error / bound = {r:.4f}")
            assert r <= 1.0, (*what, r)
            assert torch.equal(out, general), (*what, "bits differ from the general kernel")
            WORST[name] = max(WORST.get(name, 0.0), r)
        names.append(name)
    return names


def wides_of(cx, t):
    return [1, 2] if (not cx and t <= WIDE_MAX_T) else [1]


# ---- every instantiation at its smallest shape

INSTANCES = [(cx, form, t) for cx in (False, True) for form in (0, 1) for t in range(1, MAX_T[cx] + 1)]
assert {kernel_name(cx, f, t, wn) for cx, f, t in INSTANCES for wn in ((1, 2) if wides_of(cx, t) == [1, 2] else (1,))} == ALL_NAMES


def instance_id(inst):
    cx, form, t = inst
    return f"{'c128' if cx else 'f64'}-form{form}-T{t}"


@pytest.mark.parametrize("inst", INSTANCES, ids=instance_id)
def test_every_instantiation_at_its_smallest_shape(K, inst):
    cx, form, t = inst
    small, k = small_of(cx, t), 21          # fp64: two 16-deep stages, tail 5; complex128: three 8-deep stages, tail 5
    wides = wides_of(cx, t)
    if form == 0:
        # W = 45: segments of 46 virtual columns straddle every tile edge.  Batch 9: four 128-wide or two 256-wide tiles,
        # the last one partial -- one workgroup walks them all; batch 29: 11 or 6 tiles, two and more for each of three
        runs = [(make_case(cx, small, 45, k, 9), [0, 3, 1], (4, 2)), (make_case(cx, small, 45, k, 29), [0, 3], (11, 6))]
    else:
        # 5 tiles + 5 rows: 645 rows in tiles of 128, 1285 in tiles of 256 (and in tiles of 128: the same product on both)
        runs = [(make_case(cx, 645, small, k, 1), [0, 3], (6, 3))]
    ns = blocks_and_tiles(cx, small)[1]
    for case, wgss, (narrow, wide_tiles) in runs:
        assert tiles_of(case, 1) == narrow * ns and (len(wides) == 1 or form == 1 or tiles_of(case, 2) == wide_tiles * ns)
        names = check(K, case, wides if form == 0 else [1], wgss, f"m={case.m} n={case.n} k={k} batch={case.batch}")
        assert names[0] == kernel_name(cx, form, t, 1)
        assert form == 1 or len(wides) == 1 or names[1] == kernel_name(False, 0, t, 2)
    if form == 1 and len(wides) == 2:
        case = make_case(cx, 1285, small, k, 1)
        assert tiles_of(case, 2) == 6 * ns
        assert check(K, case, [1, 2], [0, 3], f"m=1285 n={small} k={k}") == [kernel_name(False, 1, t, 1), kernel_name(False, 1, t, 2)]


def test_all_68_instantiations_are_dispatched(K):
    """The collecting assertion, on its own feet (whatever part of the module was selected): the smallest product of
    every (dtype, FORM, T) under gemm_strip_wide = 1 and, where the form exists, 2 -- the dispatch log names all 68."""
    seen = set()
    for cx, form, t in INSTANCES:
        small = small_of(cx, t)
        case = make_case(cx, small, 45, 21, 9) if form == 0 else make_case(cx, 645, small, 21, 1)
        for wide in wides_of(cx, t):
            with K.tuning(**STRIP, gemm_strip_wide=wide, gemm_strip_wgs=3):
                case.run(K)
                seen.add(K.last_dispatch().split(" x")[0])
    torch.cuda.synchronize()
    assert seen == ALL_NAMES, (sorted(ALL_NAMES - seen), sorted(seen - ALL_NAMES))


# ---- the full grid on a representative subset

K_GRID = {False: [5, 16, 21, 48], True: [5, 8, 21, 24]}       # nk = 1 with and without a tail, whole stages only, a tail
W_GRID = [7, 45, 46, 128, 300]       # many segments per wave block, odd, even, exactly one tile, wider than a tile
WGS_GRID = [0, 1, 3, 8]
# (dtype, FORM, small extent): fp64 FORM 0 T = 1, 5, 10 (both WN), 11, 16; FORM 1 T = 2, 9 (both WN), 13; complex128
# T = 1, 5, 8 of both forms; two, three and four tiles along the small extent
GRID = ([(False, 0, small_of(False, t)) for t in (1, 5, 10, 11, 16)] + [(False, 0, 525), (False, 0, 1021)] +
        [(False, 1, small_of(False, t)) for t in (2, 9, 13)] + [(False, 1, 525), (False, 1, 1021)] +
        [(True, f, small_of(True, t)) for f in (0, 1) for t in (1, 5, 8)] + [(True, f, s) for f in (0, 1) for s in (200, 509)])


def grid_batch(cx, w):
    """Batch entries of a FORM 0 grid case: at least three tiles of the widest form that runs (256 fp64, 128 complex128)."""
    wp = w if cx else w + (w & 1)
    return cdiv(2 * (128 if cx else 256) + 1, wp) + 1


@pytest.mark.parametrize("k_index", range(4))
@pytest.mark.parametrize("spec", GRID, ids=[f"{'c128' if cx else 'f64'}-form{f}-small{s}" for cx, f, s in GRID])
def test_grid_of_k_segment_width_and_workgroups(K, spec, k_index):
    cx, form, small = spec
    k = K_GRID[cx][k_index]
    t, ns = blocks_and_tiles(cx, small)
    wides = wides_of(cx, t)
    if form == 0:
        cases = [make_case(cx, small, w, k, grid_batch(cx, w)) for w in W_GRID]
    else:
        cases = [make_case(cx, 1285 if not cx else 645, small, k, 1)]          # (more rows than columns: FORM 1)
    for case in cases:
        assert form_of(case.m, case.n, case.batch) == form and tiles_of(case, wides[-1]) >= 3 * ns
        names = check(K, case, wides, WGS_GRID, f"m={case.m} n={case.n} k={k} batch={case.batch}")
        assert names == [kernel_name(cx, form, t, wn) for wn in wides]


@pytest.mark.parametrize("cx,form,small,n_or_m", [(False, 0, 77, 45), (False, 0, 78, 46), (False, 1, 78, 646), (False, 1, 141, 1286),
                                                   (True, 0, 77, 45), (True, 1, 77, 645)])
def test_aligned_layout(K, cx, form, small, n_or_m):
    # 16-byte bases, every stride even (fp64 with an odd W too: the dummy column of a segment is then the padding column)
    case = make_case(cx, small, n_or_m, 21, 9, even=True) if form == 0 else make_case(cx, n_or_m, small, 21, 1, even=True)
    assert not any(x & 1 for x in (case.lda, case.ldb, case.ldc, case.sb, case.sc)) and case.offs == (0, 0, 0)
    check(K, case, wides_of(cx, blocks_and_tiles(cx, small)[0]), [0, 3], f"aligned m={case.m} n={case.n}")


# ---- random products

@st.composite
def strip_case(draw):
    cx = draw(st.booleans())
    form = draw(st.integers(0, 1))
    small, k = draw(st.integers(1, 260)), draw(st.integers(1, 70))
    if form == 0:
        m, n, batch = small, draw(st.integers(1, 300)), draw(st.integers(2, 6))
    else:
        m, n, batch = small + draw(st.integers(1, 700)), small, 1
    pads = [draw(st.integers(0, 3)) for _ in range(5)]
    offs = tuple(draw(st.integers(0, 3)) for _ in range(3))
    wide, wgs = draw(st.sampled_from([0, 1, 2])), draw(st.sampled_from([0, 1, 2, 3, 5, 8, 4096]))
    return cx, m, n, k, batch, pads, offs, wide, wgs, draw(st.integers(0, 2**31 - 1))


@given(strip_case())
@settings(max_examples=int(os.environ.get("QS_HYP_EXAMPLES", "40")), deadline=None, derandomize=True,
          suppress_health_check=list(HealthCheck))
def test_random_products_match_long_double_and_the_general_kernel(spec):
    from quantum_systems_amd import kernels as K

    cx, m, n, k, batch, (pa, pb, pc, gb, gc), offs, wide, wgs, seed = spec
    case = Case(cx, m, n, k, batch, (k + pa, n + pb, n + pc, gb, gc, 0), seed, offs=offs)
    assert form_of(m, n, batch) == (0 if batch > 1 else 1)
    names = check(K, case, [wide], [wgs], f"random m={m} n={n} k={k} batch={batch} lds={case.lda},{case.ldb},{case.ldc} offs={offs}")
    assert names[0] in ALL_NAMES


# ---- what the strip kernels do not take

@pytest.mark.parametrize("fast,kernel", [(0, "qs::gemm_kernel<"), (3, "qs::gemm_fast_kernel<")], ids=["general", "fast"])
@pytest.mark.parametrize("what", ["accumulate", "pairs"])
@pytest.mark.parametrize("cx", [False, True], ids=["f64", "c128"])
def test_accumulate_and_pairs_hand_over_to_the_tiled_kernels(K, cx, what, fast, kernel):
    # gemm_strip = 2 with both new keys set: an accumulating product and a triangular batch (grid 3: the pairs j >= i of
    # the nine entries) still run on the other tiled kernels, and nothing but the pairs' entries is written
    grid = 3
    case = Case(cx, 77, 45, 21, grid * grid, odd_layout(cx, 77, 45, 21), seed=5 + cx, accumulate=what == "accumulate")
    upper = np.array([j >= i for i in range(grid) for j in range(grid)])
    with K.tuning(**dict(STRIP, gemm_fast=fast), gemm_strip_wide=2, gemm_strip_wgs=3):
        out = case.run(K, pairs=grid) if what == "pairs" else case.run(K)
        ran = K.last_dispatch()
    assert ran.startswith(kernel) and "gemm_strip" not in ran, ran
    torch.cuda.synchronize()
    r = case.ratio(out, upper if what == "pairs" else None)
    assert r <= 1.0, (what, ran, r)
    with K.tuning(**STRIP, gemm_strip_wide=2, gemm_strip_wgs=3):         # the plain product of the same operands: the strip kernel
        case.accumulate = False
        case.run(K)
        assert K.last_dispatch().split(" x")[0] == kernel_name(cx, 0, 5, 1 if cx else 2), K.last_dispatch()
