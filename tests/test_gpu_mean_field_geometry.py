"""``kernels.mean_field`` (qs_mean_field.hip) in every launch geometry up to L = 1024.

The host picks a geometry from (L, R, dtypes): the column threads CT of a tile, the column and row blocks (ncb, nrb),
two waves per tile row when CT = 128, and a chunk length Rc that the LDS room for D caps at large L.
tests/test_gpu_mean_field.py stops at L = 96 and reaches 7 of the 16 tile classes of each form; this file runs the case
table of tests/_mean_field_cases.py, which tests/test_mean_field_cabi.py proves complete against the library's own
``qs_mean_field_plan``.  The tests here read their geometry from the same hook, not from a copy of its arithmetic.

Parity uses the bound of test_gpu_mean_field.py unchanged (it holds for ANY summation order, so for any geometry):
|W - W_exact| <= gamma_(2 R L + 2) * A, times 2 sqrt 2 for complex results, W_exact in numpy.longdouble.  The largest
error / bound per form is printed and, when QS_MEAN_FIELD_PARITY_OUT names a file, appended there."""

import ctypes
import os

import numpy as np
import pytest
import torch

import _mean_field_cases as cases
import _mean_field_ref as ref

pytestmark = pytest.mark.gpu
FORMS = list(cases.FORMS)
FORM_INDEX = {"fp64": 0, "complex128": 1, "mixed": 2}
# (cj, ck) -> the <DOJ, DOK> instantiation that must run
WEIGHTS = [((1.0, -0.5), "true, true"), ((1.0, 0.0), "true, false"), ((0.0, 1.0), "false, true")]


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def bits(t):
    return t.contiguous().view(torch.float64).view(torch.int64)


def plan_of(form, L, P, R):
    from quantum_systems_amd import _lib

    u_dtype, d_dtype = cases.FORMS[form][:2]
    out = (ctypes.c_int64 * 7)()
    assert _lib.load().qs_mean_field_plan(u_dtype, d_dtype, L, P, R, ctypes.cast(out, ctypes.c_void_p), 7) == 0
    return dict(zip(cases.PLAN_FIELDS, out))


def slab_operands(form, L, P, R, seed):
    """The seeded generator of test_gpu_mean_field.operands, drawing a (P, R, L, L) slab instead of the whole tensor."""
    rng = np.random.default_rng(seed)
    u = rng.standard_normal((P, R, L, L))
    D = rng.standard_normal((L, L))
    if form == "complex128":
        u = u + 1j * rng.standard_normal((P, R, L, L))
    if form != "fp64":
        D = D + 1j * rng.standard_normal((L, L))
    return u, D


def fill(shape, dtype, seed):
    """Seeded normal numbers drawn on the device (tools/mean_field_bench.py): a whole tensor never crosses the bus."""
    gen = torch.Generator(device="cuda").manual_seed(seed)
    t = torch.empty(shape, dtype=dtype, device="cuda")
    flat = torch.view_as_real(t).reshape(-1) if t.is_complex() else t.reshape(-1)
    step = 1 << 28
    for i in range(0, flat.numel(), step):
        flat[i:i + step].normal_(generator=gen)
    return t


@pytest.fixture(scope="module")
def worst():
    seen = {}
    yield seen
    path = os.environ.get("QS_MEAN_FIELD_PARITY_OUT")
    for form in FORMS:
        if form in seen:
            line = f"{form}: largest |W - W_exact| / bound = {seen[form]:.3e} (geometry cases, L <= 1024)"
            print(line)
            if path:
                with open(path, "a") as fh:
                    fh.write(line + "\n")


@pytest.mark.parametrize("case", cases.CASES, ids=cases.case_id)
def test_parity_within_the_summation_bound(case, worst):
    from quantum_systems_amd import kernels

    form, L, P, p_lo, R, r_lo = case
    u, D = slab_operands(form, L, P, R, 100000 + 1031 * L + 7 * p_lo + R)
    J, K = ref.jk(u, D, r_lo, extended=True)
    aJ, aK = ref.jk(np.abs(u), np.abs(D), r_lo)
    scale = ref.gamma(2 * R * L + 2) * (1.0 if form == "fp64" else 2.0 * np.sqrt(2.0))
    d_u, d_D = dev(u), dev(D)
    del u
    for (cj, ck), inst in WEIGHTS:
        W = kernels.mean_field(d_u, d_D, cj=cj, ck=ck, r_lo=r_lo)
        assert kernels.last_dispatch().count(f"qs::mean_field_kernel<{FORM_INDEX[form]}, {inst}>") == 1
        assert W.dtype == (torch.float64 if form == "fp64" else torch.complex128) and tuple(W.shape) == (P, L)
        err = np.abs(W.cpu().numpy().astype(J.dtype) - (cj * J + ck * K)).astype(np.float64)
        ratio = float((err / (scale * (abs(cj) * aJ + abs(ck) * aK))).max())
        print(f"{cases.case_id(case)} cj={cj} ck={ck}: error / bound = {ratio:.3e}")
        worst[form] = max(worst.get(form, 0.0), ratio)
        assert ratio <= 1.0, (case, cj, ck, ratio, plan_of(form, L, P, R))


# (form, L, which geometry the case is there for): odd L, so that in the forms with two columns per item the 16-byte
# item of a row's last element reaches into the next row
CONTAINMENT = [("fp64", 145, "blocks"), ("complex128", 129, "blocks"), ("mixed", 145, "blocks"),
               ("complex128", 449, "ct8"), ("fp64", 255, "wpr2")]


@pytest.mark.parametrize("form,L,why", CONTAINMENT)
def test_non_finite_values_stay_in_their_row(form, L, why):
    from quantum_systems_amd import kernels

    P, R, r_lo, p0 = 3, cases.cdiv(4096, L) + 2, 2, 1        # the shortest R with chunks of two r
    plan = plan_of(form, L, P, R)
    cpi = cases.FORMS[form][2]
    CT = 1 << plan["ct_log"]
    RB, cols = 8 * (256 // CT), CT * cpi
    if why == "blocks":
        assert plan["ncb"] > 1 and plan["nrb"] > 1, plan
    elif why == "ct8":
        assert CT == 8 and plan["ncb"] > 1 and plan["nrb"] > 1, plan
    else:
        assert CT == 128 and L > 64 * cpi, plan         # the second wave of a tile row holds real columns
        cols = 64 * cpi                                 # ... and the seam is between the two waves
    assert plan["Rc"] > 1 and cols < L and RB < L, plan
    u, D = slab_operands(form, L, P, R, 4242 + L)
    clean = kernels.mean_field(dev(u), dev(D), cj=1.0, ck=-0.5, r_lo=r_lo)
    assert torch.isfinite(clean.abs()).all()
    # (r, a, b, value): the last column of a column block (of the first wave), the first of the next, the last row of
    # a row block and the first of the next, the last element of an odd row and the first of the row after it (the
    # two halves of one straddling item), the slab's last element
    poison = [(0, 3, cols - 1, np.nan), (1, 5, cols, np.inf), (2, RB - 1, 7, -np.inf), (3, RB, 9, np.nan),
              (4, L - 2, L - 1, np.inf), (5, 4, 0, -np.inf), (R - 1, L - 1, L - 1, -np.inf)]
    d_D = dev(D)
    for r, a, b, value in poison:
        bad = u.copy()
        bad[p0, r, a, b] = value
        got = kernels.mean_field(dev(bad), d_D, cj=1.0, ck=-0.5, r_lo=r_lo)
        where = (form, L, r, a, b, value, plan)
        assert torch.equal(bits(got[[0, 2]]), bits(clean[[0, 2]])), where
        # u[p0, r, a, b] enters J[p0, a] and K[p0, b], and nothing else
        hit = sorted({a, b})
        rest = [q for q in range(L) if q not in hit]
        assert not torch.isfinite(got[p0, hit].abs()).any(), where
        assert torch.equal(bits(got[p0, rest]), bits(clean[p0, rest])), where
    bad = u.copy()
    for r, a, b, value in poison:
        bad[p0, r, a, b] = value
    got = kernels.mean_field(dev(bad), d_D, cj=1.0, ck=-0.5, r_lo=r_lo)
    assert torch.equal(bits(got[[0, 2]]), bits(clean[[0, 2]]))
    assert not torch.isfinite(got[p0].abs()).all()


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("L", [129, 257, 513, 1023])
def test_padding_contributes_nothing(form, L):
    # constant u = c, D = 1: every element of W is (cj + ck) c R L, exactly (multiples of 1/8 far below 2^53) --
    # padding columns, padding rows and the far half of an odd row's last item add nothing
    from quantum_systems_amd import kernels

    P, R, r_lo = 2, 7, 3
    c = 0.5 + 0.25j if form == "complex128" else 0.5
    cu = np.full((P, R, L, L), c)
    cD = np.ones((L, L), dtype=np.float64 if form == "fp64" else np.complex128)
    d_u, d_D = dev(cu), dev(cD)
    for (cj, ck), _ in WEIGHTS:
        W = kernels.mean_field(d_u, d_D, cj=cj, ck=ck, r_lo=r_lo).cpu().numpy()
        assert (W == (cj + ck) * c * R * L).all(), (form, L, cj, ck, plan_of(form, L, P, R))


# one L per form with more than one column block whose whole tensor fits comfortably (3.6 GB, 4.6 GB, 3.6 GB)
WHOLE = {"fp64": 146, "complex128": 130, "mixed": 146}


@pytest.mark.parametrize("form", FORMS)
def test_rows_are_bit_identical_and_bits_repeat_on_a_whole_tensor(form):
    from quantum_systems_amd import kernels

    L = WHOLE[form]
    plan = plan_of(form, L, L, L)
    assert plan["ncb"] > 1 and plan["Rc"] > 1, plan
    cplx = torch.complex128
    u = fill((L, L, L, L), cplx if form == "complex128" else torch.float64, 11)
    D = fill((L, L), torch.float64 if form == "fp64" else cplx, 12)
    h_D = D.cpu().numpy()
    SLABS = [(0, 1), (L // 4, 3), (L - 2, 2)]
    exact = {}
    for p_lo, P in SLABS:
        h_u = u[p_lo:p_lo + P].cpu().numpy()
        exact[p_lo] = ref.jk(h_u, h_D, 0, extended=True) + ref.jk(np.abs(h_u), np.abs(h_D), 0)
    scale = ref.gamma(2 * L * L + 2) * (1.0 if form == "fp64" else 2.0 * np.sqrt(2.0))
    for (cj, ck), _ in WEIGHTS:
        full = kernels.mean_field(u, D, cj=cj, ck=ck)
        again = kernels.mean_field(u, D, cj=cj, ck=ck)
        assert torch.equal(bits(full), bits(again)), (form, cj, ck)
        for p_lo, P in SLABS:
            rows = kernels.mean_field(u[p_lo:p_lo + P], D, cj=cj, ck=ck)
            assert torch.equal(bits(rows), bits(full[p_lo:p_lo + P])), (form, cj, ck, p_lo, P)
            assert torch.equal(bits(kernels.mean_field(u[p_lo:p_lo + P], D, cj=cj, ck=ck)), bits(rows))
            J, K, aJ, aK = exact[p_lo]
            err = np.abs(rows.cpu().numpy().astype(J.dtype) - (cj * J + ck * K)).astype(np.float64)
            ratio = float((err / (scale * (abs(cj) * aJ + abs(ck) * aK))).max())
            print(f"{form} L={L} rows [{p_lo}, {p_lo + P}) cj={cj} ck={ck}: error / bound = {ratio:.3e}")
            assert ratio <= 1.0, (form, cj, ck, p_lo, P, ratio)


def test_out_aliases_are_refused_at_large_sizes():
    from quantum_systems_amd import kernels

    form, L, P, R, r_lo = "fp64", 450, 2, 11, 5
    assert plan_of(form, L, P, R)["ncb"] > 1
    u, D = slab_operands(form, L, P, R, 5)
    d_u, d_D = dev(u), dev(D)
    good = kernels.mean_field(d_u, d_D, cj=1.0, ck=-0.5, r_lo=r_lo)
    flat = d_u.view(-1)
    for out in (flat[:P * L].view(P, L), flat[-P * L:].view(P, L), d_D[:P], d_D[L - P:]):
        with pytest.raises(ValueError, match="aliases"):
            kernels.mean_field(d_u, d_D, cj=1.0, ck=-0.5, r_lo=r_lo, out=out)
    # nothing was written by the refused calls
    assert torch.equal(d_u.cpu(), torch.from_numpy(u)) and torch.equal(d_D.cpu(), torch.from_numpy(D))
    out = torch.empty_like(good)
    assert kernels.mean_field(d_u, d_D, cj=1.0, ck=-0.5, r_lo=r_lo, out=out) is out
    assert torch.equal(bits(out), bits(good))
