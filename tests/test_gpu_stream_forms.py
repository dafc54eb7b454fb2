"""Every reachable instantiation of the stream kernels (qs_gemm_stream.hip), their block walk and their gates; the ring of
the skinny kernel (qs_gemm_skinny.hip).

``gemm_stream_try`` chooses between 44 compiled kernels.  fp64: ``gemm_stream_left_kernel<TMW, SPLIT, KQ, 2, VEC>`` with
(TMW, SPLIT) = (1, 1), (2, 1) for one and two blocks of 16 rows, (2, 2) from three blocks up -- (4, 1) there under
``gemm_stream`` = 2 --, KQ = ceil(k / 16) = 1 ... 4 and VEC = 16-byte accesses: 32, all reachable.  complex128:
``gemm_stream_left_cx_kernel<TMW, SPLIT, KQ>`` with (1, 1), (2, 1), (2, 2); k > 48 is refused, so the three KQ = 4
kernels are compiled and never launched (the hand-over test below documents it): 9 reachable, 41 in all.

All edge handling of these kernels is address arithmetic: buffer range checks for the K tail and the row tail, a clamped
column for the lanes past n, a marker bit that parks their stores, one host-side gate for the 32-bit offsets, and
persistent waves that walk a block list across batch slices.  ``gemm_stream_wgs`` caps the workgroups of a launch: with
1 and 3 every wave of the smallest eligible shape walks hundreds of blocks and crosses batch slices, with 3 the waves have
unequal trip counts.

Cases are tests/_product_case.py's: flat host buffers, NaN around A and B (the gap below each B[t] and between batch
slices included), a sentinel around C.  Every case asserts
1. error / bound <= 1 on every stored element against the numpy.longdouble (clongdouble) product of the same strided
   views, the bound gamma_(k+2) |A| |B| (times 2 sqrt 2 for complex products) -- derived, not tuned;
2. ``torch.equal`` on the WHOLE C buffer with the general kernel (every other route off): the documented "same k order";
3. ``torch.equal`` between all ``gemm_stream_wgs`` settings of the same product;
4. no NaN in a stored element, every sentinel intact;
5. the dispatch log names the exact instantiation, computed by a restatement of the selection rule.

The worst error / bound per instantiation is printed and, when QS_STREAM_FORMS_OUT names a file, appended there
(profiles/stream_forms.txt holds the figures measured on the MI355X).

The skinny kernel: m = 16, 32 are the reachable row counts (m > 32 is refused: ``gemm_skinny_kernel<CX, 3>`` and
``<CX, 4>`` are compiled and never launched); its eight-deep ring is run at one k-step, not yet full, exactly full, one
step into the second round, and two rounds and a tail."""

import functools
import os

import numpy as np
import pytest
import torch
from numpy.lib.stride_tricks import as_strided

from _blocks_ref import gamma
from _product_case import SENTINEL, Case, cdiv, even_layout, odd_layout

pytestmark = pytest.mark.gpu

OTHERS_OFF = dict(gemm_strip=0, gemm_fast=0, gemm_skinny=0, gemm_fit=0)
GENERAL = dict(OTHERS_OFF, gemm_stream=0)
GATE = {False: 1 << 15, True: 1 << 16}          # least n * batch
K_MAX = {False: 64, True: 48}


def fp64_name(tmw, split, kq, vec):
    return f"qs::gemm_stream_left_kernel<{tmw}, {split}, {kq}, 2, {'true' if vec else 'false'}>"


def cx_name(tmw, split, kq):
    return f"qs::gemm_stream_left_cx_kernel<{tmw}, {split}, {kq}>"


ALL_NAMES = ({fp64_name(tmw, split, kq, vec) for tmw, split in ((1, 1), (2, 1), (2, 2), (4, 1)) for kq in (1, 2, 3, 4)
              for vec in (False, True)} |
             {cx_name(tmw, split, kq) for tmw, split in ((1, 1), (2, 1), (2, 2)) for kq in (1, 2, 3)})
assert len(ALL_NAMES) == 41


def rows_of(cx, m, knob):
    """(TMW, SPLIT) of gemm_stream_try."""
    tm = cdiv(m, 16)
    if tm <= 2:
        return tm, 1
    return (4, 1) if (not cx and knob == 2) else (2, 2)


def vec_conditions(case):
    """The seven conditions of the fp64 kernels' 16-byte accesses (the bases of the device buffers are 16-byte aligned)."""
    one = case.batch == 1
    return (case.offs[1] % 2 == 0, case.offs[2] % 2 == 0, case.ldb % 2 == 0, case.ldc % 2 == 0,
            one or case.sb % 2 == 0, one or case.sc % 2 == 0, case.n % 2 == 0)


def eligible(case):
    """gemm_stream_try's gates for a case, restated (the 32-bit offset gate on the 16 KQ rows the ring addresses)."""
    cx, m, n, k, batch = case.cx, case.m, case.n, case.k, case.batch
    esz = 16 if cx else 8
    if case.accumulate or (batch > 1 and case.sa) or m > 64 or k > K_MAX[cx] or n * batch < GATE[cx]:
        return False
    if (16 * cdiv(k, 16) * case.ldb + n) * esz >= 1 << 31 or ((m + 63) * case.ldc + n) * esz >= 1 << 31:
        return False
    return cx or not (m % 64 == 0 and n % 128 == 0 and k % 16 == 0)


def expected(case, knob):
    """The instantiation gemm_stream_try launches for an eligible case under ``gemm_stream`` = knob."""
    assert eligible(case)
    tmw, split = rows_of(case.cx, case.m, knob)
    kq = cdiv(case.k, 16)
    return cx_name(tmw, split, kq) if case.cx else fp64_name(tmw, split, kq, all(vec_conditions(case)))


def seed_of(cx, m, n, k, batch):
    return (m * 1000003 + n * 1009 + k * 17 + batch) * 2 + cx


@functools.lru_cache(maxsize=4)
def make_case(cx, m, n, k, batch, even=False):
    """The case of a product, built (and its reference computed) once and shared by the tests that need it."""
    layout = (even_layout if even else odd_layout)(cx, m, n, k)
    return Case(cx, m, n, k, batch, layout, seed=seed_of(cx, m, n, k, batch))


@pytest.fixture(scope="module")
def K():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    from quantum_systems_amd import kernels

    return kernels


WORST = {}


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    lines = [f"stream forms {name}: largest error / bound = {r:.4f}" for name, r in sorted(WORST.items())]
    print("\n" + "\n".join(lines) + f"\nstream forms: {len(WORST)} instantiations")
    if os.environ.get("QS_STREAM_FORMS_OUT"):
        with open(os.environ["QS_STREAM_FORMS_OUT"], "a") as f:
            f.write("\n".join(lines) + "\n")


def ran_name(K):
    return K.last_dispatch().split(" x")[0]


def general_run(K, case):
    with K.tuning(**GENERAL):
        out = case.run(K)
        assert K.last_dispatch().startswith("qs::gemm_kernel<"), K.last_dispatch()
    return out


def check(K, case, knobs, wgss, tag):
    """Assertions 1 - 5 for every (gemm_stream, gemm_stream_wgs) of the lists; the names that ran."""
    assert all(t.data_ptr() % 16 == 0 for t in (case.dA, case.dB, case.dC0))
    general = general_run(K, case)
    names = []
    judged, r = None, 0.0
    for knob in knobs:
        name = expected(case, knob)
        first = None
        for wgs in wgss:
            with K.tuning(**OTHERS_OFF, gemm_stream=knob, gemm_stream_wgs=wgs):
                out = case.run(K)
                ran = ran_name(K)
            what = (tag, name, f"gemm_stream={knob}", f"wgs={wgs}")
            assert ran == name, (*what, ran)
            torch.cuda.synchronize()
            if judged is None or not torch.equal(out, judged):      # (a buffer with the bits of a judged one: the same verdict)
                r = case.ratio(out)
                judged = out
            print(f"stream forms {name} {tag} gemm_stream={knob} wgs={wgs}: max error / bound = {r:.4f}")
            assert r <= 1.0, (*what, r)
            assert torch.equal(out, general), (*what, "bits differ from the general kernel")
            if first is None:
                first = out
            assert torch.equal(out, first), (*what, f"bits differ from gemm_stream_wgs={wgss[0]}")
            WORST[name] = max(WORST.get(name, 0.0), r)
        names.append(name)
    return names


def knobs_of(cx, m):
    """The ``gemm_stream`` values that select different kernels for m rows."""
    return [1, 2] if (not cx and m > 32) else [1]


def smallest(cx, even):
    """(n, batch) just above the length gate: two blocks per slice, one or two live columns in the second."""
    if cx:
        return 33, 1986
    return (34, 964) if even else (33, 993)


for _cx, _even in ((False, False), (False, True), (True, False)):
    _n, _batch = smallest(_cx, _even)
    assert GATE[_cx] <= _n * _batch < GATE[_cx] + _n and cdiv(_n, 32) == 2


# ---- every instantiation at its smallest shape

INSTANCES = ([(False, tm, kq, vec) for tm in (1, 2, 3) for kq in (1, 2, 3, 4) for vec in (False, True)] +
             [(True, tm, kq, False) for tm in (1, 2, 3) for kq in (1, 2, 3)])


def instance_id(inst):
    cx, tm, kq, vec = inst
    return f"{'c128' if cx else 'f64'}-tm{tm}-kq{kq}" + ("" if cx else f"-vec{int(vec)}")


def instance_names(inst):
    cx, tm, kq, vec = inst
    if cx:
        return [cx_name(*rows_of(True, 16 * tm, 1), kq)]
    return [fp64_name(*rows_of(False, 16 * tm, knob), kq, vec) for knob in knobs_of(False, 16 * tm)]


assert {name for inst in INSTANCES for name in instance_names(inst)} == ALL_NAMES


def instance_shape(inst):
    cx, tm, kq, vec = inst
    n, batch = smallest(cx, vec)
    # a partial last row block; a k tail that is no multiple of 4: zero fragments of A and rows of B past the records
    return cx, 16 * tm - 3, n, 16 * kq - 3, batch, vec


@pytest.mark.parametrize("inst", INSTANCES, ids=instance_id)
def test_every_instantiation_at_its_smallest_shape(K, inst):
    case = make_case(*instance_shape(inst))
    assert all(vec_conditions(case)) == inst[3] or case.cx
    names = check(K, case, knobs_of(case.cx, case.m), [0, 1, 3], f"m={case.m} n={case.n} k={case.k} batch={case.batch}")
    assert names == instance_names(inst)


def test_all_41_instantiations_are_dispatched(K):
    """The collecting assertion, on its own feet (whatever part of the module was selected): the smallest product of
    every instantiation, launched without a reference -- the dispatch log names all 41."""
    seen = set()
    for inst in INSTANCES:
        cx, m, n, k, batch, even = instance_shape(inst)
        case = Case(cx, m, n, k, batch, (even_layout if even else odd_layout)(cx, m, n, k), seed=1, reference=False)
        for knob in knobs_of(cx, m):
            with K.tuning(**OTHERS_OFF, gemm_stream=knob, gemm_stream_wgs=3):
                case.run(K)
                seen.add(ran_name(K))
            assert expected(case, knob) in seen
    torch.cuda.synchronize()
    assert seen == ALL_NAMES, (sorted(ALL_NAMES - seen), sorted(seen - ALL_NAMES))


# ---- extents at the edges, on one instantiation per (TMW, SPLIT) and dtype (fp64 tm = 3: both of its kernels)

def edge_cases():
    out = []
    for cx in (False, True):
        kmax, gate = K_MAX[cx], GATE[cx]
        for tm in (1, 2, 3):
            m = 16 * tm - 3
            n0, batch0 = smallest(cx, True)                      # (fp64: the even layout, 16-byte accesses)
            for k in (1, 32, 17, kmax):                           # one element, 16 kq, 16 (kq - 1) + 1, the largest
                out.append((cx, m, n0, k, batch0))
            for n in (1, 2, 31, 32, 63):                          # one lane, one pair, one short of a block, a block, two short of two
                out.append((cx, m, n, 29, cdiv(gate, n)))
            out.append((cx, m, gate + 1, 29, 1))                  # one slice: 1025 / 2049 blocks, the last with one column
        out.append((cx, 1, 33, 29, cdiv(gate, 33)))
        out.append((cx, 64, 33, 29, cdiv(gate, 33)))              # (fp64: n no multiple of 128, else the whole-tile rule takes it)
    return out


EDGES = edge_cases()


@pytest.mark.parametrize("spec", EDGES, ids=[f"{'c128' if s[0] else 'f64'}-m{s[1]}-n{s[2]}-k{s[3]}-batch{s[4]}" for s in EDGES])
def test_extents_at_the_edges(K, spec):
    cx, m, n, k, batch = spec
    case = make_case(cx, m, n, k, batch, even=n % 2 == 0)        # even n: 16-byte accesses; odd n: the odd layout
    assert cx or all(vec_conditions(case)) == (n % 2 == 0)
    check(K, case, knobs_of(cx, m), [0, 3], f"m={m} n={n} k={k} batch={batch}")


# ---- each condition of the 16-byte accesses alone

def vec_variants():
    m, k = 29, 29                                                # (k + 1 and m + 1 even: the parity of sb, sc is the gap's)
    lda, ldb, ldc, gb, gc, _ = even_layout(False, m, 34, k)
    return {
        "all-met": (34, 964, (lda, ldb, ldc, gb, gc, 0), (0, 0, 0), None),
        "odd-ldb": (34, 964, (lda, ldb + 1, ldc, gb, gc, 0), (0, 0, 0), 2),
        "odd-ldc": (34, 964, (lda, ldb, ldc + 1, gb, gc, 0), (0, 0, 0), 3),
        "odd-sb": (34, 964, (lda, ldb, ldc, gb + 1, gc, 0), (0, 0, 0), 4),
        "odd-sc": (34, 964, (lda, ldb, ldc, gb, gc + 1, 0), (0, 0, 0), 5),
        "B-8-byte-aligned": (34, 964, (lda, ldb, ldc, gb, gc, 0), (0, 1, 0), 0),
        "C-8-byte-aligned": (34, 964, (lda, ldb, ldc, gb, gc, 0), (0, 0, 1), 1),
        "odd-n": (33, 993, (lda, ldb, ldc, gb, gc, 0), (0, 0, 0), 6),
    }


@pytest.mark.parametrize("which", list(vec_variants()))
def test_each_condition_of_the_16_byte_accesses_alone(K, which):
    n, batch, layout, offs, broken = vec_variants()[which]
    case = Case(False, 29, n, 29, batch, layout, seed=seed_of(False, 29, n, 29, batch), offs=offs)
    assert [i for i, met in enumerate(vec_conditions(case)) if not met] == ([] if broken is None else [broken])
    names = check(K, case, [1], [0, 3], which)
    assert names == [fp64_name(2, 1, 2, broken is None)]


# ---- non-finite values stay in their columns

NON_FINITE = [(False, tm, vec) for tm in (1, 2, 3) for vec in (False, True)] + [(True, tm, False) for tm in (1, 2, 3)]


@pytest.mark.parametrize("cx,tm,vec", NON_FINITE,
                         ids=[f"{'c128' if cx else 'f64'}-tm{tm}" + ("" if cx else f"-vec{int(vec)}") for cx, tm, vec in NON_FINITE])
def test_non_finite_values_stay_in_their_columns(K, cx, tm, vec):
    m, k = 16 * tm - 3, 29
    n, batch = smallest(cx, vec)
    case = Case(cx, m, n, k, batch, (even_layout if vec else odd_layout)(cx, m, n, k), seed=11 + tm, reference=False)
    # (slice, row of B, column, value): the first block, the partial last block, and both blocks of the last slice
    plants = [(0, 0, 5, np.nan), (batch // 2, k - 1, n - 1, np.inf), (batch - 1, 3, 17, np.nan), (batch - 1, k - 1, n - 1, np.inf)]
    es = case.B.dtype.itemsize
    poisoned = case.B.copy()
    b = as_strided(poisoned[case.offs[1]:], (batch, k, n), (case.sb * es, case.ldb * es, es))
    hit = np.zeros(case.C0.size, dtype=bool)
    for t, row, col, value in plants:
        b[t, row, col] = value
        as_strided(hit[case.offs[2]:], (batch, m, n), (case.sc, case.ldc, 1))[t, :, col] = True
    clean_b, poisoned_b = case.dB, torch.from_numpy(poisoned).cuda()
    for knob in knobs_of(cx, m):
        name = expected(case, knob)
        assert name == (cx_name(*rows_of(True, m, 1), 2) if cx else fp64_name(*rows_of(False, m, knob), 2, vec))
        for wgs in (0, 3):
            outs = []
            for operand in (clean_b, poisoned_b):
                case.dB = operand
                with K.tuning(**OTHERS_OFF, gemm_stream=knob, gemm_stream_wgs=wgs):
                    outs.append(case.run(K))
                    assert ran_name(K) == name, (name, ran_name(K))
            case.dB = clean_b
            torch.cuda.synchronize()
            clean, got = (o.cpu().numpy() for o in outs)
            assert np.isfinite(clean[case.stored]).all() and np.array_equal(clean[~case.stored], case.C0[~case.stored])
            assert not np.isfinite(got[hit]).any(), (name, wgs, "a planted column came out finite in some row")
            assert np.array_equal(got[~hit].view(np.int64), clean[~hit].view(np.int64)), \
                (name, wgs, "a non-finite value left its column")


# ---- what the stream kernels do not take

HAND_OVERS = {
    # name: (m, n per dtype, k, batch per dtype, layout, Case keywords, dtypes)
    "accumulate": (29, (33, 33), 29, (993, 1986), odd_layout, dict(accumulate=True), (False, True)),
    "per-entry-A": (29, (33, 33), 29, (993, 1986), odd_layout, dict(per_entry_a=True), (False, True)),
    "m65": (65, (33, 33), 29, (993, 1986), odd_layout, {}, (False, True)),
    "k65": (29, (33, 33), 65, (993, 1986), odd_layout, {}, (False, True)),
    "k49": (29, (33, 33), 49, (993, 1986), odd_layout, {}, (True,)),      # complex128 KQ = 4 is never launched:
    "k64": (29, (33, 33), 64, (993, 1986), odd_layout, {}, (True,)),      # k > 48 goes to the tiled kernels
    "one-below-the-gate": (29, (31, 51), 29, (1057, 1285), odd_layout, {}, (False, True)),
    "whole-tile": (64, (128, 128), 16, (256, 256), even_layout, {}, (False,)),
}
assert 31 * 1057 == GATE[False] - 1 and 51 * 1285 == GATE[True] - 1

HAND_OVER_PARAMS = [(what, cx) for what, spec in HAND_OVERS.items() for cx in spec[6]]


@pytest.mark.parametrize("what,cx", HAND_OVER_PARAMS, ids=[f"{w}-{'c128' if cx else 'f64'}" for w, cx in HAND_OVER_PARAMS])
def test_hand_overs_name_another_kernel_and_are_right(K, what, cx):
    m, ns, k, batches, layout, kw, _ = HAND_OVERS[what]
    n, batch = ns[cx], batches[cx]
    case = Case(cx, m, n, k, batch, layout(cx, m, n, k), seed=seed_of(cx, m, n, k, batch), **kw)
    assert not eligible(case)
    for knob in (1, 2):
        with K.tuning(**OTHERS_OFF, gemm_stream=knob, gemm_stream_wgs=3):
            out = case.run(K)
            ran = K.last_dispatch()
        assert ran.startswith("qs::gemm_kernel<") and "gemm_stream" not in ran, (what, ran)
        torch.cuda.synchronize()
        r = case.ratio(out)
        print(f"stream forms hand-over {what} {'c128' if cx else 'f64'} gemm_stream={knob}: {ran}, max error / bound = {r:.4f}")
        assert r <= 1.0, (what, ran, r)


def test_complex_operands_on_8_byte_addresses_are_refused_before_any_kernel(K):
    # gemm_stream_try hands complex operands that are not 16-byte aligned to the other kernels; through the C ABI no such
    # product arrives there: qs_matmul refuses a pointer that is not aligned to its element.  Nothing runs, C is untouched.
    case = Case(True, 29, 33, 29, 1986, odd_layout(True, 29, 33, 29), seed=3, reference=False)
    out = case.dC0.clone()
    for shifted in range(3):
        operands = [case.dA, case.dB, out]
        operands[shifted] = torch.view_as_real(operands[shifted]).reshape(-1)[1:]        # the same storage, 8 bytes on
        assert operands[shifted].data_ptr() % 16 == 8
        with K.tuning(**OTHERS_OFF, gemm_stream=1):
            with pytest.raises(ValueError, match="aligned"):
                K.gemm_raw(case.dt, *operands, case.m, case.n, case.k, case.lda, case.ldb, case.ldc, case.batch,
                           0, case.sb, case.sc, False, a_off=1, b_off=1, c_off=1)
            assert "kernel" not in K.last_dispatch(), K.last_dispatch()
    torch.cuda.synchronize()
    assert torch.equal(out, case.dC0)


# ---- the 32-bit offsets of the ring

class FarRows:
    """C = A B for one slice whose rows of B lie ``ldb`` elements apart, hundreds of megabytes: B is filled with NaN on
    the device, then its k rows are written.  A with lda = k + 1 (NaN in the padding), C with ldc = n + 4 and one extra
    row, the sentinel around it."""

    def __init__(self, cx, m, n, k, ldb, seed):
        self.cx, self.m, self.n, self.k, self.ldb = cx, m, n, k, ldb
        self.lda, self.ldc = k + 1, n + 4
        dt = np.complex128 if cx else np.float64
        self.dt = torch.complex128 if cx else torch.float64
        rng = np.random.default_rng(seed)

        def rnd(*shape):
            x = rng.standard_normal(shape)
            return x + 1j * rng.standard_normal(shape) if cx else x

        a, b = rnd(m, k), rnd(k, n)
        A = np.full(m * self.lda + 8, np.nan, dtype=dt)
        A[:m * self.lda].reshape(m, self.lda)[:, :k] = a
        self.dA = torch.from_numpy(A).cuda()
        self.dB = torch.full(((k - 1) * ldb + n + 8,), complex(np.nan, np.nan) if cx else np.nan, dtype=self.dt, device="cuda")
        self.dB.as_strided((k, n), (ldb, 1)).copy_(torch.from_numpy(b).cuda())
        self.C0 = np.full((m + 1) * self.ldc, SENTINEL, dtype=dt)
        self.dC0 = torch.from_numpy(self.C0).cuda()
        ld = np.clongdouble if cx else np.longdouble
        self.prod = np.matmul(a.astype(ld), b.astype(ld))
        self.bound = gamma(k + 2) * np.matmul(np.abs(a), np.abs(b)) * (2.0 * np.sqrt(2.0) if cx else 1.0)

    def run(self, K):
        out = self.dC0.clone()
        K.gemm_raw(self.dt, self.dA, self.dB, out, self.m, self.n, self.k, self.lda, self.ldb, self.ldc)
        return out

    def ratio(self, out):
        got = out.cpu().numpy().reshape(self.m + 1, self.ldc)
        ref = self.C0.reshape(self.m + 1, self.ldc)
        assert np.array_equal(got[:, self.n:], ref[:, self.n:]) and np.array_equal(got[self.m], ref[self.m]), \
            "a sentinel around C was overwritten"
        c = got[:self.m, :self.n]
        assert not np.isnan(c.real).any() and not np.isnan(c.imag).any(), "a NaN reached a stored element"
        return float((np.abs(c - self.prod) / self.bound).max())


# (dtype, n, ldb, stream kernel or None = whichever kernel the dispatcher picks).  k = 4: one k-step of records, and the
# ring of KQ = 1 addresses rows 0 ... 15.  At ldb = 38 343 240 (fp64) row 15 starts 15 ldb 8 = 2^32 + 306 221 504 bytes
# into the slice: in 32-bit arithmetic that is element 38 277 688 of row 0, inside the slice's records, in the NaN padding
# between the rows, and A's zero fragment times that NaN is NaN in every column.  A gate on the rows the ring addresses
# keeps such a slice away from the stream kernels; just under that gate they still run.
FAR = [
    ("f64-row-15-past-2^32", False, 32768, 38343240, None),
    # (the same bytes per row; with n = 32768 complex columns it is below the length gate and, by n's own 16 bytes per
    # element, past the offset gate as well: the tiled kernels' product at this ldb)
    ("c128-twin-at-half-the-ldb", True, 32768, 19171620, None),
    ("c128-row-15-past-2^32-long-enough-to-stream", True, 65536, 19164598, None),
    ("f64-just-under-the-gate", False, 32768, 16775166, fp64_name(1, 1, 1, True)),
    ("c128-just-under-the-gate", True, 65536, 8384510, cx_name(1, 1, 1)),
]
for _tag, _cx, _n, _ldb, _name in FAR:
    _esz = 16 if _cx else 8
    if "twin" not in _tag:
        assert _n >= GATE[_cx] and ((4 + 3) * _ldb + _n) * _esz < 1 << 31           # long enough, and inside a gate on k + 3 rows;
    assert ((16 * _ldb + _n) * _esz < 1 << 31) == (_name is not None)               # inside the gate on 16 rows: only the last two;
    assert (15 * _ldb * _esz >= 1 << 32) == (_name is None)                         # row 15 of the others wraps
    assert _name is not None or _n < (15 * _ldb * _esz) % (1 << 32) // _esz < _ldb  # into the padding of row 0
    assert _name is None or ((16 * (_ldb + 2) + _n) * _esz >= 1 << 31)              # (just under: the next even ldb is refused)


@pytest.mark.parametrize("tag,cx,n,ldb,name", FAR, ids=[f[0] for f in FAR])
def test_rows_of_the_ring_past_32_bit_offsets(K, tag, cx, n, ldb, name):
    case = FarRows(cx, 13, n, 4, ldb, seed=ldb % 1000 + cx)
    with K.tuning(**OTHERS_OFF, gemm_stream=1):
        out = case.run(K)
        ran = ran_name(K)
    torch.cuda.synchronize()
    nans = int(torch.isnan(torch.view_as_real(out) if cx else out).sum())
    print(f"stream forms far rows {tag}: {ran}, NaN in the C buffer: {nans}")
    r = case.ratio(out)
    print(f"stream forms far rows {tag}: max error / bound = {r:.4f}")
    assert r <= 1.0, (tag, ran, r)
    assert name is None or ran == name, (tag, ran)


# ---- the skinny kernel's ring

SKINNY = dict(gemm_strip=0, gemm_fast=0, gemm_stream=0, gemm_fit=0, gemm_skinny=1)
SKINNY_N = {False: (65536, 65792), True: (65536, 65664)}          # the least n, and one workgroup strip (256 / 128) more


def skinny_name(cx, tms):
    return f"qs::gemm_skinny_kernel<{'true' if cx else 'false'}, {tms}>"


def skinny_case(cx, m, n, k, batch=1, ldb=None, reference=True):
    return Case(cx, m, n, k, batch, (k + 1, ldb or n + 2, n + 4, 2, 2, 0), seed=seed_of(cx, m, n, k, batch), reference=reference)


@pytest.mark.parametrize("k", [4, 28, 32, 36, 68])   # one k-step; 7 of 8 slots; exactly full; one step into round two; two rounds and one
@pytest.mark.parametrize("tms", [1, 2])
@pytest.mark.parametrize("cx", [False, True], ids=["f64", "c128"])
def test_skinny_ring_depths(K, cx, tms, k):
    for n in SKINNY_N[cx]:
        case = skinny_case(cx, 16 * tms, n, k)
        with K.tuning(**SKINNY):
            out = case.run(K)
            ran = ran_name(K)
        assert ran == skinny_name(cx, tms), ran
        torch.cuda.synchronize()
        r = case.ratio(out)
        print(f"stream forms {ran} n={n} k={k}: max error / bound = {r:.4f}")
        assert r <= 1.0, (ran, n, k, r)
        WORST[f"{ran} k={k}"] = max(WORST.get(f"{ran} k={k}", 0.0), r)


SKINNY_HAND_OVERS = [(cx, what) for cx in (False, True) for what in ("n-not-a-strip-multiple", "odd-ldb", "m48", "batch2")
                     if not (cx and what == "odd-ldb")]      # (complex128 elements are 16 bytes at any ldb: the condition is fp64's)


@pytest.mark.parametrize("cx,what", SKINNY_HAND_OVERS, ids=[f"{'c128' if cx else 'f64'}-{what}" for cx, what in SKINNY_HAND_OVERS])
def test_skinny_hand_overs(K, cx, what):
    case = {"n-not-a-strip-multiple": lambda: skinny_case(cx, 16, 65536 + 64, 28),
            "odd-ldb": lambda: skinny_case(cx, 16, 65536, 28, ldb=65536 + 3),
            "m48": lambda: skinny_case(cx, 48, 65536, 28),
            "batch2": lambda: skinny_case(cx, 16, 65536, 28, batch=2)}[what]()
    with K.tuning(**SKINNY):
        out = case.run(K)
        ran = K.last_dispatch()
    assert ran.startswith("qs::gemm_kernel<") and "gemm_skinny" not in ran, (what, ran)
    torch.cuda.synchronize()
    r = case.ratio(out)
    assert r <= 1.0, (what, ran, r)
    if what != "batch2":              # the same product with the one condition met: the skinny kernel
        twin = {"n-not-a-strip-multiple": lambda: skinny_case(cx, 16, 65536, 28, reference=False),
                "odd-ldb": lambda: skinny_case(cx, 16, 65536, 28, ldb=65536 + 2, reference=False),
                "m48": lambda: skinny_case(cx, 32, 65536, 28, reference=False)}[what]()
        with K.tuning(**SKINNY):
            twin.run(K)
            assert ran_name(K).startswith("qs::gemm_skinny_kernel<"), K.last_dispatch()
