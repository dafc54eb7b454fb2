"""``kernels.mean_field_batch`` (qs_mean_field_batch.hip) on the GPU: parity of every ``W_k`` against the
numpy.longdouble evaluation under the any-order bound of tests/_mean_field_ref.py (|W - W_exact| <= gamma_(2RL+2) A, A
the formula on absolute values, a further 2 sqrt 2 for complex results -- derived there, not tuned), independence of
the batch bit for bit, padding and leakage, the number of streaming launches, and one smallest and one largest L of
every tile class of ``qs_mean_field_batch_plan`` up to L = 1024.

Host cost: numpy's longdouble products run at a few 10^8 multiply-adds a second, and the exact sums of 16 densities
over a whole L = 96 slab are 10^10 of them.  So the exact sums of the ND_MAX densities of an (L, slab) are taken once
(every batch size uses a prefix of those densities), as ``numpy.inner`` on contiguous rows, and from L = 55 on for
``checked_rows`` of the slab only (the first two, the middle one and the last).  The kernel still runs the whole
slab for every batch size, and ALL its rows are then held against the fp64 evaluation of the same sums by torch on the
GPU: that one obeys the same any-order bound, so the two differ by at most twice the bound."""

import ctypes
import os

import numpy as np
import pytest
import torch

import _mean_field_ref as ref

pytestmark = pytest.mark.gpu
F64, C128 = 0, 1
FORMS = {"fp64": (F64, F64, 2, 1), "complex128": (C128, C128, 1, 2), "mixed": (F64, C128, 2, 2)}
FORM_INDEX = {"fp64": 0, "complex128": 1, "mixed": 2}
SIZES = [1, 2, 5, 16, 31, 55, 64, 65, 96]
BATCHES = [1, 2, 3, 4, 5, 8, 9, 16]
ROWS_FROM = 55                  # from this L on the longdouble sums are taken for ``checked_rows`` of a slab
WEIGHTS = [(1.0, 0.0), (0.0, 1.0), (1.0, -0.5), (2.0, -1.0), (1.0, -1.0), (0.0, -1.0), (0.5, 0.25)]
PLAN_FIELDS = ("G", "passes", "Rc", "nchunk", "ct_log", "ncb", "nrb", "lds_bytes", "grid")


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def bits(t):
    return t.contiguous().view(torch.float64).view(torch.int64)


def plan_of(form, L, P, R, ND=1):
    from quantum_systems_amd import _lib

    u_dtype, d_dtype = FORMS[form][:2]
    out = (ctypes.c_int64 * 9)()
    assert _lib.load().qs_mean_field_batch_plan(u_dtype, d_dtype, L, P, R, ND, ctypes.cast(out, ctypes.c_void_p), 9) == 0
    return dict(zip(PLAN_FIELDS, out))


def streaming_launches(entry):
    """Launches of the streaming kernel in one ``last_dispatch`` entry (repeats of a name are logged as ``name xN``)."""
    import re

    total = 0
    for part in entry.split(";"):
        if "qs::mean_field_batch_kernel<" in part:
            m = re.search(r" x(\d+)$", part.strip())
            total += int(m.group(1)) if m else 1
    return total


def weights_for(nd, shift=0):
    w = [WEIGHTS[(k + shift) % len(WEIGHTS)] for k in range(nd)]
    return [a for a, _ in w], [b for _, b in w]


def operands(form, shape, nd, seed):
    """A (P, R, L, L) slab and nd densities, seeded."""
    rng = np.random.default_rng(seed)
    L = shape[-1]

    def draw(shp, is_complex, sample):                 # complex: both parts in one pass, no temporaries of u's size
        return sample(shp + (2,)).view(np.complex128).reshape(shp) if is_complex else sample(shp)

    u = draw(tuple(shape), form == "complex128", rng.random)            # uniform: a third of the time of a normal draw
    u -= 0.5 + 0.5j if form == "complex128" else 0.5
    D = draw((nd, L, L), form != "fp64", rng.standard_normal)
    return u, D


def extended_inner(A, Bt):
    """``A @ Bt.T`` in numpy.longdouble (``inner`` runs over contiguous rows: several times faster than ``@`` there);
    a real ``A`` with a complex ``Bt`` as two real products."""
    A = A.astype(np.clongdouble if np.iscomplexobj(A) else np.longdouble)
    if np.iscomplexobj(Bt) and not np.iscomplexobj(A):
        return np.inner(A, Bt.real.astype(np.longdouble)) + 1j * np.inner(A, Bt.imag.astype(np.longdouble))
    return np.inner(A, Bt.astype(np.clongdouble if np.iscomplexobj(Bt) else np.longdouble))


def jk_batch(slab, D, r_lo, extended=False):
    """(J, K), each (ND, P, L): ``ref.jk`` for every density, as two matrix products over (r, s)."""
    P, R, L = slab.shape[0], slab.shape[1], slab.shape[3]
    Bt = np.ascontiguousarray(D[:, :, r_lo:r_lo + R].transpose(0, 2, 1)).reshape(-1, R * L)      # [k, (r, s)]
    product = extended_inner if extended else (lambda A, Bt: A @ Bt.T)
    J = product(slab.transpose(0, 2, 1, 3).reshape(P * L, R * L), Bt)    # u[p, r, q, s] -> [(p, q), (r, s)]
    K = product(slab.transpose(0, 3, 1, 2).reshape(P * L, R * L), Bt)    # u[p, r, s, q] -> [(p, q), (r, s)]
    return J.reshape(P, L, -1).transpose(2, 0, 1), K.reshape(P, L, -1).transpose(2, 0, 1)


def jk_device(d_slab, d_D, r_lo):
    """(J, K) of every density in fp64 by torch on the GPU: any order of summation, the same bound."""
    Dr = d_D[:, :, r_lo:r_lo + d_slab.shape[1]]
    if Dr.is_complex() and not d_slab.is_complex():
        parts = [jk_device(d_slab, x.contiguous(), 0) for x in (Dr.real, Dr.imag)]
        return tuple(torch.complex(re, im) for re, im in zip(*parts))
    return torch.einsum("prqs,ksr->kpq", d_slab, Dr), torch.einsum("prsq,ksr->kpq", d_slab, Dr)


def checked_rows(P):
    return sorted({0, 1, P // 2, P - 1} & set(range(P)))


def slabs(u, L):
    p_lo, P = L // 4, max(1, L // 3)
    r_lo = L // 3 if L > 2 else L - 1
    return [("full", u, 0), ("rows", u[p_lo:p_lo + P], 0), ("second", np.ascontiguousarray(u[:, r_lo:]), r_lo)]


def check_parity(form, slab, D, r_lo, batches, what, rows=None):
    """Every W_k of every batch size against the longdouble sums (on ``rows`` of the slab when given: then every row
    is also held to twice the bound against ``jk_device``); returns the largest error / bound."""
    from quantum_systems_amd import kernels

    L, R = slab.shape[3], slab.shape[1]
    some = rows is not None
    rows = list(range(slab.shape[0])) if rows is None else rows
    J, K = jk_batch(slab[rows], D, r_lo, extended=True)
    aJ, aK = jk_batch(np.abs(slab[rows]), np.abs(D), r_lo)
    scale = ref.gamma(2 * R * L + 2) * (1.0 if form == "fp64" else 2.0 * np.sqrt(2.0))
    d_slab, d_D = dev(slab), dev(D)
    if some:
        tJ, tK = jk_device(d_slab, d_D, r_lo)
        taJ, taK = jk_device(d_slab.abs(), d_D.abs(), r_lo)
    worst = 0.0
    for nd in batches:
        cj, ck = weights_for(nd, shift=nd)
        W = kernels.mean_field_batch(d_slab, d_D[:nd], cj=cj, ck=ck, r_lo=r_lo)
        assert W.dtype == (torch.float64 if form == "fp64" else torch.complex128)
        assert tuple(W.shape) == (nd, slab.shape[0], L)
        if some:
            wj, wk = (torch.tensor(w, dtype=torch.float64, device="cuda")[:, None, None] for w in (cj, ck))
            apart = (W - (wj * tJ[:nd] + wk * tK[:nd])).abs()
            assert bool((apart <= 2.0 * scale * (wj.abs() * taJ[:nd] + wk.abs() * taK[:nd])).all()), (form, what, nd)
        W = W[:, rows].cpu().numpy()
        for k in range(nd):
            err = np.abs(W[k].astype(J.dtype) - (cj[k] * J[k] + ck[k] * K[k])).astype(np.float64)
            bound = scale * (abs(cj[k]) * aJ[k] + abs(ck[k]) * aK[k])
            ratio = float((err / bound).max())
            worst = max(worst, ratio)
            assert ratio <= 1.0, (form, what, nd, k, cj[k], ck[k], ratio)
    return worst


def report(line):
    print(line)
    path = os.environ.get("QS_MEAN_FIELD_PARITY_OUT")
    if path:
        with open(path, "a") as fh:
            fh.write(line + "\n")


def test_the_bound_used_here_is_the_reference_bound():
    u, D = operands("mixed", (3, 4, 5, 5), 2, 1)
    slab = np.ascontiguousarray(u[:, 1:])
    aJ, aK = jk_batch(np.abs(slab), np.abs(D), 1)
    mine = ref.gamma(2 * 3 * 5 + 2) * 2.0 * np.sqrt(2.0) * (1.0 * aJ[1] + 0.5 * aK[1])
    np.testing.assert_allclose(mine, ref.error_bound(slab, D[1], 1.0, -0.5, r_lo=1), rtol=1e-13)


@pytest.mark.parametrize("form", list(FORMS))
def test_parity_within_the_summation_bound(form):
    worst = 0.0
    for L in SIZES:
        u, D = operands(form, (L, L, L, L), max(BATCHES), 3000 + L)
        for name, slab, r_lo in slabs(u, L):
            rows = checked_rows(slab.shape[0]) if L >= ROWS_FROM else None
            worst = max(worst, check_parity(form, slab, D, r_lo, BATCHES, (L, name), rows))
    report(f"{form}: largest |W_k - W_exact| / bound = {worst:.3e} (batch, L <= 96)")


@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("L", [5, 31, 64, 65])
def test_results_do_not_depend_on_the_batch(form, L):
    from quantum_systems_amd import kernels

    G = plan_of(form, L, L, L)["G"]
    nmax = 2 * G + 1
    u, D = operands(form, (L, L, L, L), nmax, 17 + L)
    d_u, d_D = dev(u), dev(D)
    cj, ck = weights_for(nmax)
    alone = [kernels.mean_field_batch(d_u, d_D[k:k + 1], cj=cj[k], ck=ck[k])[0] for k in range(nmax)]
    for nd in sorted({max(1, G - 1), G, G + 1, 2 * G + 1}):
        for pos in sorted({0, nd // 2, nd - 1}):
            # density 0 at position `pos` of a batch of nd (the others in their own order behind / before it)
            order = list(range(1, nd))
            order.insert(pos, 0)
            W = kernels.mean_field_batch(d_u, d_D[order], cj=[cj[i] for i in order], ck=[ck[i] for i in order])
            again = kernels.mean_field_batch(d_u, d_D[order], cj=[cj[i] for i in order], ck=[ck[i] for i in order])
            assert torch.equal(bits(W), bits(again)), (nd, pos)
            for j, i in enumerate(order):
                assert torch.equal(bits(W[j]), bits(alone[i])), (nd, pos, j, i)
    full = kernels.mean_field_batch(d_u, d_D[:G + 1], cj=cj[:G + 1], ck=ck[:G + 1])
    for p_lo, P in [(0, 1), (L // 4, max(1, L // 3)), (L - 2, 2)]:
        rows = kernels.mean_field_batch(d_u[p_lo:p_lo + P], d_D[:G + 1], cj=cj[:G + 1], ck=ck[:G + 1])
        assert torch.equal(bits(rows), bits(full[:, p_lo:p_lo + P])), (p_lo, P)
    out = torch.empty_like(full)
    assert kernels.mean_field_batch(d_u, d_D[:G + 1], cj=cj[:G + 1], ck=ck[:G + 1], out=out) is out
    assert torch.equal(bits(out), bits(full))


@pytest.mark.parametrize("form", list(FORMS))
def test_no_leakage_across_rows_or_densities_and_padding_contributes_nothing(form):
    from quantum_systems_amd import kernels

    L, p0 = 31, 7
    G = plan_of(form, L, L, L)["G"]
    nd = G + 1
    u, D = operands(form, (L, L, L, L), nd, 99)
    cj, ck = weights_for(nd)
    clean = kernels.mean_field_batch(dev(u), dev(D), cj=cj, ck=ck)
    bad = u.copy()
    bad[p0, 3, 30, 30] = np.nan          # last element of an odd row: its 16-byte item straddles the next row
    bad[p0, L - 1, L - 1, L - 1] = np.inf
    bad[p0, 0, 0, 0] = -np.inf
    got = kernels.mean_field_batch(dev(bad), dev(D), cj=cj, ck=ck)
    keep = [p for p in range(L) if p != p0]
    assert torch.equal(bits(got[:, keep]), bits(clean[:, keep]))
    for k in range(nd):
        assert not torch.isfinite(got[k, p0].abs()).all(), k
    # a NaN in one density stays in its own result, wherever it sits in its group
    for k_bad in sorted({0, 1, G - 1, G}):
        Db = D.copy()
        Db[k_bad, 4, 5] = np.nan
        Db[k_bad, L - 1, L - 1] = np.inf
        got = kernels.mean_field_batch(dev(u), dev(Db), cj=cj, ck=ck)
        others = [k for k in range(nd) if k != k_bad]
        assert torch.equal(bits(got[others]), bits(clean[others])), k_bad
        assert not torch.isfinite(got[k_bad].abs()).all()
    # odd L, constant u, D_k = k + 1: every element of W_k is (cj + ck) c (k + 1) L^2 exactly -- padding adds nothing
    for L in (1, 5, 31, 65):
        c = 0.5
        cu = np.full((L, L, L, L), c) if form != "complex128" else np.full((L, L, L, L), c + 0.25j)
        cD = np.stack([np.full((L, L), k + 1.0) for k in range(nd)])
        cD = cD if form == "fp64" else cD * (1.0 + 0j)
        W = kernels.mean_field_batch(dev(cu), dev(cD), cj=1.0, ck=-0.5).cpu().numpy()
        for k in range(nd):
            assert (W[k] == 0.5 * cu[0, 0, 0, 0] * (k + 1) * L * L).all(), (form, L, k)


@pytest.mark.parametrize("form", list(FORMS))
def test_one_pass_per_group(form):
    from quantum_systems_amd import kernels

    L = 16
    G = plan_of(form, L, L, L)["G"]
    u, D = operands(form, (L, L, L, L), 2 * G + 1, 5)
    d_u, d_D = dev(u), dev(D)
    for nd in (1, G, G + 1, 2 * G + 1):
        kernels.mean_field_batch(d_u, d_D[:nd], cj=1.0, ck=-0.5)
        log = kernels.last_dispatch()
        assert streaming_launches(log) == -(-nd // G), (nd, log)
        assert log.count("qs::mean_field_close_kernel") == 1 and "qs::mean_field_kernel" not in log, log
        assert f"qs::mean_field_batch_kernel<{FORM_INDEX[form]}, " in log


def test_wrapper_validates_its_arguments():
    from quantum_systems_amd import kernels

    u = torch.zeros(4, 4, 4, 4, dtype=torch.float64, device="cuda")
    D = torch.zeros(3, 4, 4, dtype=torch.float64, device="cuda")
    with pytest.raises(ValueError):
        kernels.mean_field_batch(u, D[0])
    with pytest.raises(ValueError):
        kernels.mean_field_batch(u, D[:, :3])
    with pytest.raises(ValueError):
        kernels.mean_field_batch(u, D, cj=[1.0, 2.0])
    with pytest.raises(ValueError):
        kernels.mean_field_batch(u[:, :2].contiguous(), D, r_lo=3)
    with pytest.raises(ValueError):
        kernels.mean_field_batch(u, D, out=torch.empty(3, 4, 4, dtype=torch.complex128, device="cuda"))
    assert tuple(kernels.mean_field_batch(u, D, cj=[1.0, 0.0, 2.0], ck=-0.5).shape) == (3, 4, 4)


def tile_class(plan, L):
    return (plan["ct_log"], plan["ncb"] > 1, plan["nrb"] > 1, L % 2 == 1, plan["G"])


@pytest.mark.parametrize("form", list(FORMS))
def test_every_tile_class_up_to_1024(form):
    classes = {}
    for L in range(1, 1025):
        classes.setdefault(tile_class(plan_of(form, L, 1, 1), L), []).append(L)
    sizes = sorted({L for Ls in classes.values() for L in (min(Ls), max(Ls)) if L > 96})
    assert 1023 in sizes or 1024 in sizes
    worst, P = 0.0, 3
    for L in sizes:
        R = min(L, -(-4096 // L) + 3)                  # chunks of more than one r wherever the LDS leaves room, a short last one
        r_lo = (L - R) // 2
        plan = plan_of(form, L, P, R)
        nd = plan["G"] + 1
        u, D = operands(form, (P, R, L, L), nd, 50000 + L)
        ratio = check_parity(form, u, D, r_lo, [nd], (L, plan))
        print(f"{form} L={L} {plan}: error / bound = {ratio:.3e}")
        worst = max(worst, ratio)
    report(f"{form}: largest |W_k - W_exact| / bound = {worst:.3e} (batch, {len(sizes)} sizes of {len(classes)} tile classes, "
           f"L <= 1024)")
