"""The determinant kernels past what the Jordan-Wigner oracle reaches (m <= 8, 70 determinants): several workgroups
and a ragged tail, the density's loop over more than one trip and its upper waves, orbital indices up to 62 compared
element by element, and rows of ``c`` with padding between them (``ldc > K``) through the C entry.

The reference at (m, N) = (11, 5), 462 determinants, is ``_det_ci_ref.string_hamiltonian`` / ``string_density``: the
operator strings applied to the list of masks term by term in ``numpy.longdouble`` (no Slater-Condon rule; pinned
against the Jordan-Wigner matrices in tests/test_det_ci_ref_host.py).  It is built once per form and never modified;
the Hamiltonian of a sub-list is the sub-matrix of the full one (the projection the oracle has by construction).

Tolerances are those of tests/test_gpu_det_ci.py, for the shapes used here:
  * sigma: gamma_(n+2) (|H| |c|), n = ``terms(m, N)``.  For the (8, 4) problem placed on eight scattered orbitals of a
    larger m the count is that of (8, 4): a target that is not in the list adds no operation to a sum;
  * the diagonal: gamma_(N + C(N,2)) times the moduli of its terms;
  * the density: gamma_(dim+2) |c|^2 with dim the length of the list; entries no determinant of the list connects are
    sums of nothing and must be exactly zero.
Every comparison prints its worst ratio to the bound before it asserts."""

import functools
from math import comb

import numpy as np
import pytest
import torch

import _det_ci_ref as ref
import test_gpu_det_ci as base
from test_gpu_det_ci import FORMS, H, dev, vectors

pytestmark = pytest.mark.gpu
M, N, DIM = 11, 5, 462


@functools.lru_cache(maxsize=None)
def big(cplx):
    """(ht, ut, masks, H fp64, H longdouble) at (11, 5) from the string oracle; computed once, never modified."""
    ht, ut = ref.random_hamiltonian(M, 100 * M + N, cplx)
    dets = ref.sector(M, N)
    Hx = ref.string_hamiltonian(ht, ut, dets)
    out = ht, ut, dets, Hx.astype(np.complex128 if cplx else np.float64), Hx
    for a in out:
        a.setflags(write=False)
    return out


# positions in the 462 list: dims at the edges of the 64-thread workgroups of sigma and of the 256-thread loop of the
# density, one list with holes (most searches of its excitations miss), and everything
LISTS = {f"first{n}": np.arange(n) for n in (63, 64, 65, 255, 256, 257)}
LISTS["holes300"] = np.sort(np.random.default_rng(300).permutation(DIM)[:300])
LISTS["full462"] = np.arange(DIM)


def unit(dim, cplx, seed):
    v = vectors(1, dim, cplx, seed)[0]
    return v / np.linalg.norm(v)


def logged_sigma(ht, ut, dets, n, c):
    """(sigma, launches of the sigma kernel)."""
    from quantum_systems_amd import kernels

    kernels.dispatch_log = log = []
    try:
        got = base.run_sigma(ht, ut, dets, n, c)
    finally:
        kernels.dispatch_log = None
    return got, base.launches([e for e in log if "det_ci_sigma" in e][-1])


def check_diagonal(D, ht, ut, dets, n, exact, what):
    m = ht.shape[0]
    assert D.dtype == np.float64 and D.shape == (len(dets),)
    occ = [[p for p in range(m) if x >> p & 1] for x in dets.tolist()]
    moduli = np.array([sum(abs(ht[p, p].real) for p in o) + sum(abs(ut[p, q, p, q].real) for p in o for q in o if p < q)
                       for o in occ])
    bound = ref.gamma(n + comb(n, 2)) * moduli
    err = np.abs(D - exact).astype(np.float64)
    print(f"{what}: worst |D - exact| / bound = {(err / bound).max():.3f}")
    assert (err <= bound).all(), what


def check_density(rho, exact, v, m, n, what):
    bound = ref.density_bound(v, m, n)
    err = float(np.abs(rho - exact).max())
    print(f"{what}: worst |rho - exact| / bound = {err / bound:.3f}")
    assert rho.shape == (m, m) and err <= bound, what
    assert abs(np.trace(rho) - n) <= m * bound and np.abs(rho - rho.conj().T).max() <= 2 * bound, what


@pytest.mark.parametrize("name", list(LISTS))
@pytest.mark.parametrize("form", list(FORMS))
def test_diagonal_and_sigma_across_workgroups(form, name):
    from quantum_systems_amd import kernels

    cplx = FORMS[form]
    ht, ut, full, Hd, Hx = big(cplx)
    keep = LISTS[name]
    dets = full[keep]
    sub, subx = Hd[np.ix_(keep, keep)], Hx[np.ix_(keep, keep)]
    D = H(kernels.det_ci_diagonal(dev(ht), dev(ut), dev(dets), N))
    check_diagonal(D, ht, ut, dets, N, np.diag(subx).real, f"{form} {name}")
    G = base.shipped_group(cplx)
    for K in (1, G + 1):
        c = vectors(K, len(keep), cplx, 2000 + K)
        got, count = logged_sigma(ht, ut, dets, N, c)
        assert got.shape == (K, len(keep)) and got.dtype == (np.complex128 if cplx else np.float64)
        base.check_sigma(got, subx, sub, c, M, N, f"{form} {name} K={K}")
        assert count == -(-K // G)


@pytest.mark.parametrize("name", ["first255", "first256", "first257", "holes300", "full462"])
@pytest.mark.parametrize("form", list(FORMS))
def test_density_over_several_trips_and_on_a_subset(form, name):
    from quantum_systems_amd import kernels

    cplx = FORMS[form]
    _, _, full, _, _ = big(cplx)
    keep = LISTS[name]
    v = unit(len(keep), cplx, 11)
    padded = np.zeros(DIM, dtype=v.dtype)
    padded[keep] = v
    rho = H(kernels.det_ci_density1(dev(full[keep]), dev(v), M, N))
    check_density(rho, ref.string_density(padded, full, M), v, M, N, f"{form} {name}")


@pytest.mark.parametrize("form", list(FORMS))
def test_density_of_a_vector_held_by_the_upper_waves(form):
    """Non-zeros only at list positions i >= 128 with i mod 256 >= 128: every one of them is read as ``c[i]`` by a
    thread of waves 2 and 3 of the 256-thread workgroup, so the trace is N only if the closing sum takes all four."""
    from quantum_systems_amd import kernels

    cplx = FORMS[form]
    _, _, full, _, _ = big(cplx)
    where = np.nonzero(np.arange(DIM) % 256 >= 128)[0]
    assert where.min() == 128 and (where % 256 >= 192).sum() > 64
    v = np.zeros(DIM, dtype=np.complex128 if cplx else np.float64)
    v[where] = unit(len(where), cplx, 12)
    rho = H(kernels.det_ci_density1(dev(full), dev(v), M, N))
    check_density(rho, ref.string_density(v, full, M), v, M, N, f"{form} upper waves")


@pytest.mark.parametrize("form", list(FORMS))
def test_bits_do_not_depend_on_the_group_on_many_workgroups(form):
    from quantum_systems_amd import kernels

    cplx = FORMS[form]
    ht, ut, dets, _, _ = big(cplx)
    c = vectors(11, DIM, cplx, 5)
    shipped = base.run_sigma(ht, ut, dets, N, c)
    for g in (1, 2, 4, 8):
        with kernels.tuning(det_ci_g=g):
            got, count = logged_sigma(ht, ut, dets, N, c)
        assert np.array_equal(got, shipped), g
        assert count == -(-11 // g)


# ---- high orbital indices, element by element ------------------------------------------------------------------------
# The (8, 4) problem of the Jordan-Wigner oracle on eight scattered orbitals of a larger m.  The placement preserves
# the order of the orbitals, hence every "occupied below" count: the compact oracle's H IS the answer on the 70 placed
# determinants.  Everything outside the where x where (x where x where) blocks is random and non-zero and cannot enter
# an element of H between determinants of the list: a mis-indexed read shows up instead of meeting a zero.
# m = 32 and 33 are the edges of the mask 2^m - 1; complex128 at m = 63 is the largest dynamic-LDS copy of ht, 63 504 B.
WHERE = {32: [0, 3, 9, 15, 16, 24, 30, 31], 33: [0, 7, 15, 16, 29, 30, 31, 32], 63: [0, 15, 31, 32, 33, 47, 61, 62]}


def placed(m, cplx):
    """Device ht (m, m) Hermitian, ut (m, m, m, m) and the 70 placed masks; generated on the device (252 MB at m = 63
    complex128), seeded."""
    where = np.array(WHERE[m])
    ht8, ut8, dets8, _, _ = base.problem(8, 4, cplx)
    gen = torch.Generator(device="cuda").manual_seed(6300 + m)

    def draw(*shape):
        if not cplx:
            return torch.randn(*shape, dtype=torch.float64, device="cuda", generator=gen)
        return torch.view_as_complex(torch.randn(*shape, 2, dtype=torch.float64, device="cuda", generator=gen))

    a = draw(m, m)
    ht = (0.5 * (a + a.conj().T)).contiguous()
    ut = draw(m, m, m, m)
    assert bool((ut != 0).all())
    w = torch.from_numpy(where).cuda()
    ht[w[:, None], w[None, :]] = dev(ht8)
    ut[w[:, None, None, None], w[None, :, None, None], w[None, None, :, None], w[None, None, None, :]] = dev(ut8)
    dets = np.array([sum(1 << int(where[i]) for i in range(8) if x >> i & 1) for x in dets8.tolist()], dtype=np.int64)
    assert (np.diff(dets) > 0).all() and int(dets.max()) >> (m - 1) == 1
    return ht, ut, dets


@pytest.mark.parametrize("m", list(WHERE))
@pytest.mark.parametrize("form", list(FORMS))
def test_scattered_orbitals_up_to_the_last_bit(form, m):
    from quantum_systems_amd import kernels

    cplx = FORMS[form]
    where = WHERE[m]
    ht8, ut8, dets8, Hd, Hx = base.problem(8, 4, cplx)
    ht, ut, dets = placed(m, cplx)
    d_dets = dev(dets)
    what = f"{form} m={m}"

    D = kernels.det_ci_diagonal(ht, ut, d_dets, 4)
    check_diagonal(H(D), ht8, ut8, dets8, 4, np.diag(Hx).real, what)

    G = base.shipped_group(cplx)
    for K in (1, G + 1):
        c = vectors(K, 70, cplx, 3000 + K)
        got = H(kernels.det_ci_sigma(ht, ut, d_dets, 4, D, dev(c)))
        base.check_sigma(got, Hx, Hd, c, 8, 4, f"{what} K={K}")

    keep = np.sort(np.random.default_rng(m).permutation(70)[:35])                  # misses at high bits
    c = vectors(3, 35, cplx, 3100)
    d_half = dev(dets[keep])
    got = H(kernels.det_ci_sigma(ht, ut, d_half, 4, kernels.det_ci_diagonal(ht, ut, d_half, 4), dev(c)))
    base.check_sigma(got, Hx[np.ix_(keep, keep)], Hd[np.ix_(keep, keep)], c, 8, 4, f"{what} half of the list")

    v = unit(70, cplx, 13)
    rho = H(kernels.det_ci_density1(d_dets, dev(v), m, 4))
    assert rho.shape == (m, m)
    inside = rho[np.ix_(where, where)]
    check_density(inside, ref.one_body_density(v, 8, 4), v, 8, 4, what)
    outside = rho.copy()
    outside[np.ix_(where, where)] = 0
    assert not outside.any(), f"{what}: {np.count_nonzero(outside)} density entries off the placed orbitals are not zero"


# ---- ldc > K through the C entry ------------------------------------------------------------------------------------


@pytest.mark.parametrize("case", ["m8_N4-fp64", "m8_N4-complex128", "m11_N5-fp64"])
def test_rows_of_c_with_padding_between_them(case):
    """``c`` stored as (dim, ldc) with ldc = K + 3 and NaN in the three padding columns, K = 11 > G: the second group
    starts at ``c + G`` elements and every row is ``ldc`` apart.  The wrapper always passes ldc = K; the same vectors
    through it give the bits to compare with."""
    from quantum_systems_amd import _lib, kernels

    shape, form = case.split("-")
    cplx = FORMS[form]
    ht, ut, dets, _, _ = base.problem(8, 4, cplx) if shape == "m8_N4" else big(cplx)
    m, n, dim = ht.shape[0], (4 if shape == "m8_N4" else N), len(dets)
    K, ldc = 11, 14
    assert base.shipped_group(cplx) < K
    dt = torch.complex128 if cplx else torch.float64
    d_ht, d_ut, d_dets = dev(ht), dev(ut), dev(dets)
    D = kernels.det_ci_diagonal(d_ht, d_ut, d_dets, n)
    c = dev(vectors(K, dim, cplx, 17))
    want = H(kernels.det_ci_sigma(d_ht, d_ut, d_dets, n, D, c))
    store = torch.full((dim, ldc), complex(np.nan, np.nan) if cplx else np.nan, dtype=dt, device="cuda")
    store[:, :K] = c.T
    before = H(store).tobytes()
    out = torch.zeros(K, dim, dtype=dt, device="cuda")
    code = _lib.QS_C128 if cplx else _lib.QS_F64
    rc = _lib.load().qs_det_ci_sigma(code, code, d_ht.data_ptr(), d_ut.data_ptr(), d_dets.data_ptr(), D.data_ptr(),
                                     store.data_ptr(), out.data_ptr(), m, n, dim, K, ldc, None, 0,
                                     torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert rc == 0                                                                  # QS_OK
    got = H(out)
    assert not np.isnan(got).any()
    assert np.array_equal(got, want)
    assert H(store).tobytes() == before
