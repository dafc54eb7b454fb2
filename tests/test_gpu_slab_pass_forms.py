"""Every instantiation of the slab-pair kernels (qs_slab_pair.hip), their persistent slab walk and their gates; the
sandwich slab pass (qs_sandwich4.hip, qs_sandwich4b.hip) on partial slabs, its tail split included.

The slab pass is the fused (d, c) contraction T2[a, b] = C^T . u[a, b] . C on the ``rows * L`` contiguous L x L slabs of
``rows`` leading-index rows; the b contraction (a tiled product) follows, so an entry computes
v[a,q,r,s] = sum_bcd Ct[q,b] C[c,r] C[d,s] u[a,b,c,d] and a row a of v depends on row a of u alone.

``slab_pair_try`` takes fp64 with L, M <= 64 from 256 slabs on and chooses between 24 kernels: TL = ceil(L / 16) row tiles
and k-step quads of X, TM = ceil(M / 16) column tiles; ``slab_pair_kernel<TL, TM>`` (16; one wave per slab, four slabs per
workgroup) and, for an even TM unless ``slab_pair`` = 2, ``slab_pair_split_kernel<TL, TM>`` (8; two waves per slab, two
slabs per workgroup).  Both walk: at most n_cu / 2 n_cu workgroups are launched, so one trip takes 4 n_cu slabs, and a
wave goes on to slab s + 4 n_cu with the X fragments of that slab already on their way (the split kernel through a ring
of four k-steps that runs across the slab boundary).  All edge handling is address arithmetic: a buffer descriptor per
slab whose range check zeroes rows >= L of X and drops rows >= M of Z, a select for the k tail, parked stores for columns
>= M.  TL = 1 is reachable at L = 16 only: rows <= L and rows * L >= 256 leave no other size up to 16.

``sandwich4_try`` takes the slab pass ahead of it for equal quad counts ceil(L / 4) = ceil(M / 4) from 1024 slabs on,
under the default knobs for ceil(L / 4) in {9, 10, 12, 13, 14, 15, 16} (11 loses with slabs in and slabs out).  Four slabs
make one item quad; ``sandwich4b_kernel`` splits the quads of a partly filled last round over all workgroups ("+tail").

Cases: u is a view into a NaN-filled buffer with 64 doubles of NaN in front and behind, ``out=`` likewise.  Every case
asserts
1. error / bound <= 1 on every checked element against the numpy.longdouble evaluation of the three contractions, the bound
   gamma_(3L+6) A with A the same contractions on absolute values -- tests/_blocks_ref.py's rule for three chained inner
   products, derived, not tuned (a plain fp64 numpy chain stays below 0.006 of it).  From L = 49 on the longdouble sums are
   taken on rows {0, 1, rows // 2, rows - 1} of the slab; assertion 2 covers every row;
2. the bits of the WHOLE output buffer equal those of the same call on the two tiled products (``slab_pair`` = 0,
   ``sandwich`` = 0): the documented "same chains of fused multiply-adds";
3. the bits of ``slab_pair`` = 1 and 2 are equal wherever both kernels exist (an even TM);
4. no NaN in the result, every NaN around u and around the result intact;
5. the dispatch log names the exact instantiation, computed by a restatement of the selection rule.

The worst error / bound per instantiation and per part is printed and, when QS_SLAB_FORMS_OUT names a file, appended there
(profiles/slab_pass_forms.txt holds the figures measured on the MI355X)."""

import functools
import os

import numpy as np
import pytest
import torch

from _blocks_ref import gamma
from test_gpu_kernels import _sandwich_launches

pytestmark = pytest.mark.gpu

PAD = 64                                            # doubles of NaN in front of and behind u and the result
FUSED_OFF = dict(slab_pair=0, sandwich=0)           # the two tiled products
PAIR_ONLY = dict(sandwich=0, quad4s=0, small4=0)    # nothing ahead of the slab-pair kernels


def cdiv(a, b):
    return -(-a // b)


# ---- the selection rules, restated

def pair_name(L, M, knob=1):
    """The instantiation launch_slab_pair picks under ``slab_pair`` = knob."""
    tl, tm = min(cdiv(L, 16), 4), min(cdiv(M, 16), 4)
    split = tm % 2 == 0 and knob != 2
    return f"qs::slab_pair_{'split_' if split else ''}kernel<{tl}, {tm}>"


def pair_takes(L, M, rows):
    """slab_pair_try's gates (fp64): otherwise the two tiled products."""
    return rows * L >= 256 and L <= 64 and M <= 64


ALL_NAMES = ({f"qs::slab_pair_kernel<{tl}, {tm}>" for tl in (1, 2, 3, 4) for tm in (1, 2, 3, 4)} |
             {f"qs::slab_pair_split_kernel<{tl}, {tm}>" for tl in (1, 2, 3, 4) for tm in (2, 4)})
assert len(ALL_NAMES) == 24


def tail_quads(nquads, M, n_cu, knob=1):
    """sandwich4b_tail_quads: the quads of a partly filled last round, if one task per workgroup covers them."""
    wgs = n_cu - n_cu % 8
    if not knob or wgs < 8 or nquads <= wgs:
        return 0
    ntail, parts = nquads % wgs, cdiv(cdiv(M, 4), 4)
    return ntail if ntail * parts <= wgs else 0


def sandwich_name(L, M, rows, n_cu, forced, tail_knob=1):
    """The kernel sandwich4_try launches for the slab pass of a partial call (slabs in, slabs out), None where it refuses;
    ``forced``: ``sandwich`` = 4."""
    n4 = cdiv(L, 4)
    if L > 64 or M > 64 or n4 != cdiv(M, 4) or rows * L < 1024:
        return None
    tail = tail_quads(cdiv(rows * L, 4), M, n_cu, tail_knob)
    v2 = n4 in (10, 12, 14, 16) and (not (L % 4 == 0 and n4 in (10, 14)) or tail > 0)
    n4k = n4
    if n4 % 2 and n4 >= 9 and (n4 in (11, 15) or (n4 == 9 and tail >= 48)):
        v2, n4k = True, n4 + 1
    if not forced and (n4 < 9 or n4 == 11):         # (12 and 15 run on the balanced kernel under the default knobs)
        return None
    if not 6 <= n4 <= 16:
        return None
    return f"qs::sandwich4b_kernel<{n4k}>" + ("+tail" if tail else "") if v2 else f"qs::sandwich4_kernel<{n4}>"


def default_name(L, M, rows, n_cu, **knobs):
    """First kernel of a partial fp64 call under the default knobs: sandwich, slab pair, or None (a tiled product)."""
    name = sandwich_name(L, M, rows, n_cu, False, knobs.get("sandwich_tail", 1))
    if name is None and pair_takes(L, M, rows):
        name = pair_name(L, M, knobs.get("slab_pair", 1))
    return name


# ---- a problem, its reference, and one run

def contract(x, C, Ct):
    """v[a,q,r,s] = sum_bcd Ct[q,b] C[c,r] C[d,s] x[a,b,c,d], in the dtype of the operands."""
    n, L, M = x.shape[0], C.shape[0], C.shape[1]
    t = np.matmul(x, C)                                          # d -> s: (n, L, L, M)
    t = np.matmul(C.T, t)                                        # c -> r: (n, L, M, M)
    return np.matmul(Ct, t.reshape(n, L, M * M)).reshape(n, M, M, M)


class Problem:
    """u for ``rows`` leading rows, C, Ct on the host; the reference of a row is computed when first asked for and kept."""

    def __init__(self, L, M, rows, cplx=False):
        self.L, self.M, self.rows, self.cplx = L, M, rows, cplx
        rng = np.random.default_rng((L * 1009 + M) * 1009 + rows)

        def rnd(*shape):
            x = rng.standard_normal(shape)
            return x + 1j * rng.standard_normal(shape) if cplx else x

        self.u = rnd(rows, L, L, L)
        self.C = rnd(L, M) / np.sqrt(L)
        self.Ct = rnd(M, L) / np.sqrt(L)
        self.dC, self.dCt = torch.from_numpy(self.C).cuda(), torch.from_numpy(self.Ct).cuda()
        self._ref = {}

    def reference(self, idx):
        new = [a for a in idx if a not in self._ref]
        if new:
            ld = np.clongdouble if self.cplx else np.longdouble
            exact = contract(self.u[new].astype(ld), self.C.astype(ld), self.Ct.astype(ld))
            bound = gamma(3 * self.L + 6) * contract(np.abs(self.u[new]), np.abs(self.C), np.abs(self.Ct))
            if self.cplx:
                bound = bound * 2.0 * np.sqrt(2.0)
            for i, a in enumerate(new):
                self._ref[a] = (exact[i], bound[i])
        return np.stack([self._ref[a][0] for a in idx]), np.stack([self._ref[a][1] for a in idx])

    def checked_rows(self, rows):
        return sorted({0, 1, rows // 2, rows - 1} & set(range(rows))) if self.L >= 49 else list(range(rows))

    def ratio(self, got, rows):
        idx = self.checked_rows(rows)
        exact, bound = self.reference(idx)
        return float((np.abs(got[idx] - exact) / bound).max())


@functools.lru_cache(maxsize=2)
def problem(L, M, rows):
    return Problem(L, M, rows)


def bits(t):
    return t.view(torch.int64)


class Slab:
    """The first ``rows`` rows of a problem's u on the device, NaN in front and behind; ``run`` gives the whole result buffer
    (NaN around the result) and the dispatch record."""

    def __init__(self, prob, rows, u=None):
        self.prob, self.rows = prob, rows
        n = rows * prob.L ** 3
        self.buf = torch.full((n + 2 * PAD,), float("nan"), dtype=torch.float64, device="cuda")
        self.view = self.buf[PAD:PAD + n].view(rows, prob.L, prob.L, prob.L)
        self.view.copy_(torch.from_numpy(prob.u[:rows] if u is None else u))
        self.pristine = self.buf.clone()

    def run(self, K, **knobs):
        M, n = self.prob.M, self.rows * self.prob.M ** 3
        obuf = torch.full((n + 2 * PAD,), float("nan"), dtype=torch.float64, device="cuda")
        with K.tuning(**knobs):
            K.transform_two_body_partial(self.view, self.prob.dC, self.prob.dCt, out=obuf[PAD:PAD + n].view(self.rows, M, M, M))
            ran = K.last_dispatch()
        torch.cuda.synchronize()
        assert torch.isnan(obuf[:PAD]).all() and torch.isnan(obuf[PAD + n:]).all(), (knobs, ran, "a NaN around the result was overwritten")
        assert torch.equal(bits(self.buf), bits(self.pristine)), (knobs, ran, "u or the NaN around it changed")
        return obuf, ran

    def result(self, obuf):
        M = self.prob.M
        return obuf[PAD:PAD + self.rows * M ** 3].view(self.rows, M, M, M).cpu().numpy()


def first_kernel(ran):
    return ran.split(";")[0].split(" x")[0]


@pytest.fixture(scope="module")
def K():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    from quantum_systems_amd import kernels

    return kernels


@pytest.fixture(scope="module")
def n_cu():
    return torch.cuda.get_device_properties(0).multi_processor_count


WORST = {}


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    lines = [f"slab pass forms {key}: largest error / bound = {r:.4f}" for key, r in sorted(WORST.items())]
    print("\n" + "\n".join(lines) + f"\nslab pass forms: {len(WORST)} figures")
    if os.environ.get("QS_SLAB_FORMS_OUT"):
        with open(os.environ["QS_SLAB_FORMS_OUT"], "a") as f:
            f.write("\n".join(lines) + "\n")


def check(K, prob, rows, settings, part):
    """Assertions 1 - 5 for one slab: ``settings`` is a list of (knobs, expected first kernel or None = a tiled product);
    the results of all of them carry the bits of the tiled route.  Returns the names that ran."""
    slab = Slab(prob, rows)
    tag = f"L={prob.L} M={prob.M} rows={rows}"
    tiled, ran = slab.run(K, **FUSED_OFF)
    assert "slab_pair" not in ran and "sandwich4" not in ran, (tag, ran)
    judged, r, names = None, 0.0, []
    for knobs, name in settings:
        out, ran = slab.run(K, **knobs)
        what = (part, tag, knobs, name)
        if name is None:
            assert "slab_pair" not in ran and "sandwich4" not in ran, (*what, ran)
        else:
            assert first_kernel(ran) == name, (*what, ran)
            if "sandwich4" in name:
                assert _sandwich_launches(ran.split(";")[0], cdiv(prob.L, 4)) == 1, (*what, ran)
        if judged is None or not torch.equal(bits(out), bits(judged)):       # (the bits of a judged buffer: the same verdict)
            got = slab.result(out)
            assert not np.isnan(got).any(), (*what, "a NaN reached the result")
            r = prob.ratio(got, rows)
            judged = out
        print(f"slab pass forms {part} {name or ran} {tag} {knobs}: max error / bound = {r:.4f}")
        assert r <= 1.0, (*what, r)
        assert torch.equal(bits(out), bits(tiled)), (*what, "bits differ from the two tiled products")
        key = f"{part} {name or 'tiled products'}"
        WORST[key] = max(WORST.get(key, 0.0), r)
        names.append(first_kernel(ran))
    return names


def pair_settings(L, M):
    """``slab_pair`` = 2 and, where it selects the other kernel, 1: both with nothing ahead of them."""
    knobs = [2, 1] if pair_name(L, M, 1) != pair_name(L, M, 2) else [2]
    return [(dict(PAIR_ONLY, slab_pair=k), pair_name(L, M, k)) for k in knobs]


# ---- (a) every instantiation

# per TL: one row and one live k in the last tile; L % 4 != 0, a partly live k-step; whole tiles
L_OF = {1: (16,), 2: (17, 23, 32), 3: (33, 42, 48), 4: (49, 55, 64)}
M_OF = {1: (1, 9, 16), 2: (17, 26, 32), 3: (33, 39, 48), 4: (49, 61, 64)}


def rows_of(L):
    """ceil(256 / L) and the next three: the slab count takes every residue mod 4 that L allows -- last workgroups with
    1, 2 and 3 live waves, and for the split kernel a last workgroup with one slab."""
    r0 = cdiv(256, L)
    return [r for r in range(r0, r0 + 4) if r <= L]


def instances():
    out = []
    for tl in (1, 2, 3, 4):
        for tm in (1, 2, 3, 4):
            ls, ms = L_OF[tl], M_OF[tm]
            for i in range(3):                                   # in rotation; TL = 1: its one L with all three M
                out.append((tl, tm, ls[i % len(ls)], ms[(i + tl + tm) % 3]))
    return out


INSTANCES = instances()
assert len(INSTANCES) == 48 and len(set(INSTANCES)) == 48
assert {pair_name(L, M, k) for _, _, L, M in INSTANCES for k in (1, 2)} == ALL_NAMES
assert all(pair_takes(L, M, r) for _, _, L, M in INSTANCES for r in rows_of(L))
assert {r * L % 4 for _, _, L, _ in INSTANCES if L % 2 for r in rows_of(L)} == {0, 1, 2, 3}


@pytest.mark.parametrize("tl,tm,L,M", INSTANCES, ids=[f"tl{tl}-tm{tm}-L{L}-M{M}" for tl, tm, L, M in INSTANCES])
def test_every_instantiation(K, tl, tm, L, M):
    assert (min(cdiv(L, 16), 4), min(cdiv(M, 16), 4)) == (tl, tm)
    rows = rows_of(L)
    prob = problem(L, M, rows[-1])
    for r in rows:
        names = check(K, prob, r, pair_settings(L, M), "instances")
        assert names == ([f"qs::slab_pair_kernel<{tl}, {tm}>"] +
                         ([f"qs::slab_pair_split_kernel<{tl}, {tm}>"] if tm % 2 == 0 else []))


def test_all_24_instantiations_are_dispatched(K):
    """The collecting assertion, on its own feet (whatever part of the module was selected): the smallest slab of every
    (TL, TM), launched without a reference -- the dispatch log names all 24."""
    seen = set()
    for tl in (1, 2, 3, 4):
        for tm in (1, 2, 3, 4):
            L, M = L_OF[tl][0], M_OF[tm][0]
            g = torch.Generator(device="cuda").manual_seed(16 * tl + tm)
            u = torch.randn(cdiv(256, L), L, L, L, dtype=torch.float64, device="cuda", generator=g)
            C = torch.randn(L, M, dtype=torch.float64, device="cuda", generator=g)
            for knob in (1, 2):
                with K.tuning(**PAIR_ONLY, slab_pair=knob):
                    K.transform_two_body_partial(u, C)
                    seen.add(first_kernel(K.last_dispatch()))
                assert pair_name(L, M, knob) in seen
    torch.cuda.synchronize()
    assert seen == ALL_NAMES, (sorted(ALL_NAMES - seen), sorted(seen - ALL_NAMES))


# ---- (b) the slab walk

def factor(n, ls=range(16, 65)):
    """(L, rows) with rows * L == n and rows <= L <= 64, the smallest L; None if there is none."""
    for L in ls:
        if n % L == 0 and n // L <= L:
            return L, n // L
    return None


def first_count(lo, hi, pred=lambda n: True):
    for n in range(lo, min(hi, 64 * 64 + 1)):
        if pred(n) and factor(n):
            return factor(n)
    return None


def walk_case(kind, n_cu):
    """(L, rows) of a walk case on a device of n_cu CUs; one trip of either kernel takes cap = 4 n_cu slabs."""
    cap = 4 * n_cu
    if kind == "one-full-trip":
        return factor(cap)
    if kind == "one-wave-takes-a-second-trip":                    # the smallest reachable count past one trip
        return first_count(cap + 1, 2 * cap)
    if kind == "eight-workgroups-take-a-second-trip":             # 32 slabs past one trip (16 workgroups of the split kernel)
        return first_count(cap + 32, 2 * cap)
    if kind == "between-two-and-three-trips":                     # an odd count if one is reachable, else no multiple of 4
        return first_count(2 * cap + 1, 3 * cap, lambda n: n % 2 == 1) or first_count(2 * cap + 1, 3 * cap, lambda n: n % 4 != 0)
    assert kind == "four-full-trips"
    return factor(4 * cap)


WALK_M = {"one-full-trip": 30, "one-wave-takes-a-second-trip": 20, "eight-workgroups-take-a-second-trip": 64,
          "between-two-and-three-trips": 49, "four-full-trips": 33}
assert walk_case("one-full-trip", 256) == (32, 32) and walk_case("one-wave-takes-a-second-trip", 256) == (41, 25)
assert walk_case("eight-workgroups-take-a-second-trip", 256) == (33, 32) and walk_case("four-full-trips", 256) == (64, 64)
assert all(walk_case(kind, 256) for kind in WALK_M)


@pytest.mark.parametrize("kind", list(WALK_M))
def test_slab_walk(K, n_cu, kind):
    case = walk_case(kind, n_cu)
    if case is None:
        pytest.skip(f"{kind}: no rows <= L <= 64 gives the slab count on {n_cu} CUs")
    L, rows = case
    M = WALK_M[kind]
    cap = 4 * n_cu
    print(f"slab pass forms walk {kind}: {rows} x {L} = {rows * L} slabs, one trip = {cap}")
    check(K, problem(L, M, rows), rows, pair_settings(L, M), f"walk {kind}")


# ---- (c) non-finite values stay in their slab

def second_trip_pair(L, n_cu):
    """(rows, a): slab s = a L + L - 1, the last of row a, is one a wave reaches on its second trip, and even, so that in
    the split kernel s + 1 -- the first slab of row a + 1 -- belongs to the other wave pair of its workgroup."""
    a = cdiv(max(4 * n_cu - (L - 1), 0), L)
    a += (a * L + L - 1) % 2
    return (a + 2, a) if a + 2 <= L else None


@pytest.mark.parametrize("L,second_trip", [(23, False), (49, True)], ids=["L23", "L49-second-trip"])
def test_non_finite_values_stay_in_their_slab(K, n_cu, L, second_trip):
    M = L                                                         # (an even TM: both kernels)
    if second_trip:
        found = second_trip_pair(L, n_cu)
        if found is None:
            pytest.skip(f"no slab of L = {L} lies on a second trip on {n_cu} CUs")
        rows, a = found
        assert a * L + L - 1 >= 4 * n_cu
    else:
        rows, a = L, 4
    s = a * L + L - 1
    assert s % 2 == 0 and a + 1 < rows and pair_takes(L, M, rows)
    prob = Problem(L, M, rows)
    poisoned = prob.u.copy()
    poisoned[a, L - 1, L - 1, L - 1] = np.nan                     # the last element of slab s
    poisoned[a + 1, 0, 0, 0] = np.inf                             # the first element of slab s + 1
    clean_slab, poisoned_slab = Slab(prob, rows), Slab(prob, rows, u=poisoned)
    others = [i for i in range(rows) if i not in (a, a + 1)]
    for knobs, name in pair_settings(L, M):
        outs = []
        for slab in (clean_slab, poisoned_slab):
            out, ran = slab.run(K, **knobs)
            assert first_kernel(ran) == name, (name, ran)
            outs.append(slab.result(out))
        clean, got = outs
        assert np.isfinite(clean).all()
        assert not np.isfinite(got[[a, a + 1]]).any(), (name, "an element of a row that owns a planted slab came out finite")
        assert np.array_equal(got[others].view(np.int64), clean[others].view(np.int64)), (name, "a non-finite value left its slab")


# ---- (d) gates and hand-over

# (partial calls: only the sandwich and the slab-pair kernels stand ahead of the tiled products, and the sandwich ones take
# no slab pass below 1024 slabs, so M = 20 meets none of them whatever its quad count)
GATE = [(17, 15), (17, 16), (51, 5), (51, 6), (64, 3), (64, 4)]
assert [L * rows for L, rows in GATE] == [255, 272, 255, 306, 192, 256]


@pytest.mark.parametrize("L,rows", GATE, ids=[f"{L}x{rows}" for L, rows in GATE])
def test_the_256_slab_gate(K, n_cu, L, rows):
    M = 20
    name = default_name(L, M, rows, n_cu)
    assert (name is not None) == (rows * L >= 256) and (name is None or name == pair_name(L, M))
    check(K, problem(L, M, rows), rows, [({}, name)], "gate")


@pytest.mark.parametrize("what", ["L65", "M65", "complex128", "real-u-complex-C"])
def test_sizes_and_types_the_slab_pair_kernels_refuse(K, what):
    L, M, rows = {"L65": (65, 20, 4), "M65": (64, 65, 4), "complex128": (17, 20, 16), "real-u-complex-C": (17, 9, 17)}[what]
    assert rows * L >= 256
    prob = Problem(L, M, rows, cplx=what in ("complex128", "real-u-complex-C"))
    if what == "real-u-complex-C":                               # (a whole transform: the partial entry has no mixed form)
        un = prob.u.real.copy()
        got = K.transform_two_body(torch.from_numpy(un).cuda(), prob.dC, prob.dCt)
        ran = K.last_dispatch()
        ld = np.clongdouble
        v = contract(un.astype(ld), prob.C.astype(ld), prob.Ct.astype(ld))
        exact = np.matmul(prob.Ct.astype(ld), v.reshape(L, M ** 3)).reshape(M, M, M, M)
        A = contract(np.abs(un), np.abs(prob.C), np.abs(prob.Ct))
        bound = gamma(4 * L + 8) * np.matmul(np.abs(prob.Ct), A.reshape(L, M ** 3)).reshape(M, M, M, M) * 2.0 * np.sqrt(2.0)
        r = float((np.abs(got.cpu().numpy() - exact) / bound).max())
    else:
        got = K.transform_two_body_partial(torch.from_numpy(prob.u).cuda(), prob.dC, prob.dCt)
        ran = K.last_dispatch()
        r = prob.ratio(got.cpu().numpy(), rows)
    print(f"slab pass forms refused {what}: {ran}, max error / bound = {r:.4f}")
    assert "slab_pair" not in ran and "sandwich4" not in ran, (what, ran)
    assert r <= 1.0, (what, ran, r)


# (L, M) per quad count that the sandwich kernels take under the default knobs; rows just below and at 1024 slabs
HAND_OVER = [(33, 33), (40, 38), (47, 48), (49, 52), (55, 53), (64, 61)]
assert [cdiv(L, 4) for L, _ in HAND_OVER] == [9, 10, 12, 13, 14, 16] and all(cdiv(L, 4) == cdiv(M, 4) for L, M in HAND_OVER)
assert (1023 // 33) * 33 == 1023 and cdiv(1024, 64) * 64 == 1024              # 33 x 31 is one slab short, 64 x 16 exact


@pytest.mark.parametrize("L,M", HAND_OVER, ids=[f"L{L}-M{M}" for L, M in HAND_OVER])
def test_hand_over_to_the_sandwich_kernels_at_1024_slabs(K, n_cu, L, M):
    below, at = 1023 // L, cdiv(1024, L)
    assert 256 <= below * L < 1024 <= at * L and at <= L
    prob = problem(L, M, at)
    assert default_name(L, M, below, n_cu) == pair_name(L, M)
    check(K, prob, below, [({}, pair_name(L, M))], "hand-over")
    name = default_name(L, M, at, n_cu)
    assert name.startswith("qs::sandwich4")
    check(K, prob, at, [({}, name)], "hand-over")


def test_sandwich4_kernel_6_and_7_are_never_launched(K):
    # ceil(L / 4) = 6, 7: a whole transform has M^2 <= 28^2 < 1024 columns, a partial call rows * L <= 28^2 slabs -- no entry
    # reaches the two instantiations, whatever the knobs; the slab-pair kernel takes the slab pass
    for L in (24, 28):
        prob = problem(L, L, L)
        du = torch.from_numpy(prob.u).cuda()
        for knobs in (dict(sandwich=4), dict(sandwich=4, quad4s=0, small4=0), {}):
            with K.tuning(**knobs):
                K.transform_two_body(du, prob.dC, prob.dCt)
                whole = K.last_dispatch()
                K.transform_two_body_partial(du, prob.dC, prob.dCt)
                part = K.last_dispatch()
            assert "sandwich4" not in whole and "sandwich4" not in part, (L, knobs, whole, part)
            assert first_kernel(part) == pair_name(L, L), (L, knobs, part)
        check(K, prob, L, [(dict(sandwich=4), pair_name(L, L))], "hand-over")


# ---- (e) the sandwich slab pass on partial slabs

def sandwich_settings(L, M, rows, n_cu):
    """Forced and automatic, each with and without the tail split; what the defaults hand to the slab-pair kernel (quad count
    11) is named as that."""
    return [(dict(sandwich=4), sandwich_name(L, M, rows, n_cu, True)),
            (dict(sandwich=4, sandwich_tail=0), sandwich_name(L, M, rows, n_cu, True, 0)),
            ({}, default_name(L, M, rows, n_cu)),
            (dict(sandwich_tail=0), default_name(L, M, rows, n_cu, sandwich_tail=0))]


def residue_rows(L):
    """From ceil(1024 / L) up: one row count per residue 1, 2, 3 (mod 4) of the item count that L allows."""
    r0 = cdiv(1024, L)
    return [r for r in range(r0, r0 + 4) if r * L % 4]


ITEM_L = {9: 35, 10: 39, 11: 43, 12: 47, 13: 51, 14: 55, 15: 59, 16: 63}          # odd: every residue is reachable
ITEM_CASES = [(L, M) for L in ITEM_L.values() for M in (L, L - 1)]
assert all(cdiv(L, 4) == n4 for n4, L in ITEM_L.items()) and all(cdiv(L, 4) == cdiv(M, 4) for L, M in ITEM_CASES)
assert all(sorted(r * L % 4 for r in residue_rows(L)) == [1, 2, 3] and residue_rows(L)[-1] <= L for L in ITEM_L.values())


@pytest.mark.parametrize("L,M", ITEM_CASES, ids=[f"L{L}-M{M}" for L, M in ITEM_CASES])
def test_sandwich_item_counts_off_the_quad_grid(K, n_cu, L, M):
    rows = residue_rows(L)
    prob = problem(L, M, rows[-1])
    for r in rows:
        settings = sandwich_settings(L, M, r, n_cu)
        assert settings[0][1].startswith("qs::sandwich4")
        assert settings[2][1].startswith("qs::slab_pair" if cdiv(L, 4) == 11 else "qs::sandwich4")
        check(K, prob, r, settings, f"items = {r * L % 4} (mod 4)")


def test_sandwich_on_a_23_row_slab_of_53(K, n_cu):
    # (the 7-row slabs of 53 orbitals on 8 ranks are 371 items, below the kernels' 1024; 53 x 23 = 1219 = 3 (mod 4))
    check(K, problem(53, 53, 23), 23, sandwich_settings(53, 53, 23, n_cu), "items = 3 (mod 4)")


def tail_case(kind, n_cu):
    """(L, rows), M = L, of a tail case on n_cu CUs; None if no rows <= L gives it."""
    wgs = n_cu - n_cu % 8

    def scan(ls, pred, key=None):
        found = [(L, r) for L in ls for r in range(cdiv(1024, L), L + 1) if pred(L, r, cdiv(r * L, 4))]
        if not found:
            return None
        return min(found, key=key) if key else found[0]

    def tail(L, nq):
        return tail_quads(nq, L, n_cu)

    def past(L, nq):                                             # a partly filled last round too long to split
        return wgs >= 8 and nq > wgs and nq % wgs * cdiv(cdiv(L, 4), 4) > wgs

    if kind == "tail-of-one-quad":                               # (also: one quad more than the grid)
        return scan([L for L in range(37, 65) if cdiv(L, 4) in (10, 12, 14, 15, 16)], lambda L, r, nq: tail(L, nq) == 1)
    if kind.startswith("last-quad-holds-"):
        k = int(kind[-1])
        return scan([55], lambda L, r, nq: tail(L, nq) and r * L % 4 == k)
    if kind == "largest-tail-that-splits":
        return scan([55], lambda L, r, nq: tail(L, nq), key=lambda c: -tail(c[0], cdiv(c[0] * c[1], 4)))
    if kind == "first-count-past-the-largest-tail":
        return scan([55], lambda L, r, nq: past(L, nq), key=lambda c: cdiv(c[0] * c[1], 4) % wgs)
    if kind in ("odd-quad-count-57", "odd-quad-count-58"):       # ceil(L / 4) = 15 on the instantiation for 16
        return scan([int(kind[-2:])], lambda L, r, nq: tail(L, nq))
    if kind == "quad-count-9-on-the-instantiation-for-10":       # its rule: a tail of 48 quads or more
        return scan([35, 36, 34, 33], lambda L, r, nq: tail(L, nq) >= 48)
    assert kind == "exactly-the-grid"                            # as many quads as workgroups: no tail
    return scan(range(33, 65), lambda L, r, nq: r * L == 4 * wgs)


TAIL_KINDS = ["tail-of-one-quad", "last-quad-holds-1", "last-quad-holds-2", "last-quad-holds-3", "largest-tail-that-splits",
              "first-count-past-the-largest-tail", "odd-quad-count-57", "odd-quad-count-58", "quad-count-9-on-the-instantiation-for-10",
              "exactly-the-grid"]
# 256 CUs.  (1028 items, 257 whole quads, have no rows <= L <= 64; 38 x 27 = 54 x 19 = 1026 items are 257 quads too)
assert tail_case("tail-of-one-quad", 256) == (38, 27) and tail_case("exactly-the-grid", 256) == (64, 16)
assert [tail_case(f"last-quad-holds-{k}", 256) for k in (1, 2, 3)] == [(55, 19), (55, 22), (55, 21)]
assert tail_case("odd-quad-count-57", 256) == (57, 18) and tail_case("odd-quad-count-58", 256) == (58, 18)
assert all(tail_case(kind, 256) for kind in TAIL_KINDS)


@pytest.mark.parametrize("kind", TAIL_KINDS)
def test_sandwich_tail_on_partial_slabs(K, n_cu, kind):
    case = tail_case(kind, n_cu)
    if case is None:
        pytest.skip(f"{kind}: no rows <= L <= 64 gives the quad count on {n_cu} CUs")
    L, rows = case
    settings = sandwich_settings(L, L, rows, n_cu)
    nq, wgs = cdiv(rows * L, 4), n_cu - n_cu % 8
    print(f"slab pass forms tail {kind}: {rows} x {L} = {rows * L} items, {nq} quads on {wgs} workgroups: {settings[0][1]}")
    splits = kind not in ("first-count-past-the-largest-tail", "exactly-the-grid")
    for i, (_, name) in enumerate(settings):
        assert name.startswith("qs::sandwich4") and name.endswith("+tail") == (splits and i % 2 == 0), (kind, name)
    check(K, problem(L, L, rows), rows, settings, f"tail {kind}")
