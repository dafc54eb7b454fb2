"""``kernels.det_ci_density2`` and ``kernels.det_ci_transition_density1`` on the GPU, fp64 and complex128, against the
oracles of tests/_det_ci_density_ref.py: the Jordan-Wigner matrices for m <= 8 and operator strings applied to the list
of masks past that (no Slater-Condon rule and no count between two orbitals is shared with the kernels).

Tolerance (derived, not tuned): one element of rho or of G is a sum of at most dim products conj(bra_I) ket_J with
I -> J injective, so |got - exact| <= gamma_(dim+2) |bra|_2 |ket|_2, times 2 sqrt 2 for complex products
(``_det_ci_density_ref.pair_bound``; ``_det_ci_ref.density_bound`` is its bra = ket case), with dim the length of the
list.  The exact value comes from the oracle in ``numpy.longdouble``.  Relations between two computed tensors
(Hermiticity) get twice the bound.  Entries that no determinant of the list connects are sums of nothing and must be
exactly zero; the anti-symmetry of G is exact because its four copies are written from one sum.
bra != ket are random, not normalised and not orthogonal: a swapped bra and ket, a missing conj or a wrong sign on an
intermediate mask changes elements by far more than the bound.  Every output buffer is filled with NaN before the call.
Every comparison prints its worst ratio to the bound before it asserts."""

import functools
from math import comb

import numpy as np
import pytest
import torch

import _det_ci_density_ref as dref
import _det_ci_ref as ref
from test_gpu_det_ci import FORMS, H, dev
from test_gpu_det_ci_scale import WHERE

pytestmark = pytest.mark.gpu
SHAPES = [(4, 2), (6, 3), (7, 3), (8, 4), (7, 1), (7, 6), (5, 5)]                 # dims 6, 20, 35, 70, 7, 7, 1
M, N, DIM = 11, 5, 462


def pair(dim, cplx, seed):
    """bra != ket, norms 1.3 and 0.8, overlap far from zero."""
    rng = np.random.default_rng(seed)

    def draw():
        v = rng.standard_normal(dim)
        return v + 1j * rng.standard_normal(dim) if cplx else v

    bra = draw()
    ket = draw() + 0.5 * bra
    return 1.3 * bra / np.linalg.norm(bra), 0.8 * ket / np.linalg.norm(ket)


def nan_out(shape, cplx):
    dt = torch.complex128 if cplx else torch.float64
    return torch.full(shape, complex(np.nan, np.nan) if cplx else np.nan, dtype=dt, device="cuda")


def run(dets, bra, ket, m, n):
    """(rho, G) on the device into NaN-filled buffers; ``ket is bra`` is passed on as the same tensor."""
    from quantum_systems_amd import kernels

    cplx = np.iscomplexobj(bra) or np.iscomplexobj(ket)
    d_dets, d_bra = dev(dets), dev(bra)
    d_ket = d_bra if ket is bra else dev(ket)
    rho, G = nan_out((m, m), cplx), nan_out((m,) * 4, cplx)
    assert kernels.det_ci_transition_density1(d_dets, d_bra, d_ket, m, n, out=rho) is rho
    assert kernels.det_ci_density2(d_dets, d_bra, d_ket, m, n, out=G) is G
    return rho, G


def check(got, exact, bound, what):
    assert got.shape == exact.shape and not np.isnan(got).any(), f"{what}: NaN survived"
    err = float(np.abs(got - exact).max())
    print(f"{what}: worst |got - exact| / bound = {err / bound:.3f}")
    assert err <= bound, what


def check_structure(G, what):
    """Exact anti-symmetry in (p, q) and in (r, s) and exact zeros on p = q and r = s, on the device tensor."""
    assert bool((G.permute(1, 0, 2, 3) == -G).all()) and bool((G.permute(0, 1, 3, 2) == -G).all()), what
    m = G.shape[0]
    i = torch.arange(m, device=G.device)
    assert int(torch.count_nonzero(G[i, i])) == 0 and int(torch.count_nonzero(G[:, :, i, i])) == 0, what


def cases():
    out = [(f"m{m}_N{n}", m, n, None) for m, n in SHAPES]
    out.append(("m7_N3_half", 7, 3, np.sort(np.random.default_rng(73).permutation(35)[:17])))
    return out + [("m8_N3_cisd", 8, 3, "cisd")]


@pytest.mark.parametrize("case", cases(), ids=lambda c: c[0])
@pytest.mark.parametrize("form", list(FORMS))
def test_every_element_against_the_jordan_wigner_oracle(form, case):
    from quantum_systems_amd import truncated_space

    cplx = FORMS[form]
    name, m, n, keep = case
    full = ref.sector(m, n)
    if isinstance(keep, str):
        cisd = truncated_space(m, 0b00000111, 2)
        keep = np.searchsorted(full, cisd)
        assert (full[keep] == cisd).all() and 1 < len(cisd) < len(full)
    dets = full if keep is None else full[keep]
    assert keep is not None or len(dets) == comb(m, n)
    bra, ket = pair(len(dets), cplx, 1000 * m + n)
    for what, b, k in ((f"{form} {name} transition", bra, ket), (f"{form} {name} state", ket, ket)):
        rho, G = run(dets, b, k, m, n)
        assert rho.dtype == G.dtype == (torch.complex128 if cplx else torch.float64)
        rho_x, G_x = dref.jw_densities(b, k, m, n, keep)
        bound = dref.pair_bound(b, k)
        check(H(rho), rho_x, bound, what + " rho")
        check(H(G), G_x, bound, what + " G")
        check_structure(G, what)
        if n == 1:
            assert H(G).tobytes() == bytes(G.numel() * G.element_size()), f"{what}: one particle has no pair density"
        else:
            assert float(np.abs(G_x).max()) > 1e-3                                      # the comparison is not of zeros


@pytest.mark.parametrize("form", list(FORMS))
def test_swapping_bra_and_ket_conjugates(form):
    """G^{kl}[r,s,p,q] = conj(G^{lk}[p,q,r,s]) and rho^{kl}[q,p] = conj(rho^{lk}[p,q]): two computed tensors, twice the
    bound."""
    cplx = FORMS[form]
    for m, n in ((8, 4), (7, 3), (6, 3)):
        dets = ref.sector(m, n)
        bra, ket = pair(len(dets), cplx, 50 * m + n)
        rho_kl, G_kl = (H(x) for x in run(dets, bra, ket, m, n))
        rho_lk, G_lk = (H(x) for x in run(dets, ket, bra, m, n))
        bound = 2 * dref.pair_bound(bra, ket)
        e1 = float(np.abs(rho_kl - rho_lk.conj().T).max())
        e2 = float(np.abs(G_kl - G_lk.conj().transpose(2, 3, 0, 1)).max())
        print(f"{form} m={m} N={n}: Hermiticity of rho {e1 / bound:.3f}, of G {e2 / bound:.3f} of twice the bound")
        assert e1 <= bound and e2 <= bound
        if cplx:
            assert np.abs(G_kl - G_lk.transpose(2, 3, 0, 1)).max() > 1e3 * bound     # the conjugate is not optional


# ---- longer lists: several trips of the 256-thread loop, a partial last trip, missing targets ---------------------------
LISTS = {f"first{n}": np.arange(n) for n in (255, 256, 257)}
LISTS["holes300"] = np.sort(np.random.default_rng(300).permutation(DIM)[:300])
LISTS["full462"] = np.arange(DIM)


@pytest.mark.parametrize("name", list(LISTS))
@pytest.mark.parametrize("form", list(FORMS))
def test_several_trips_and_subsets_against_the_string_oracle(form, name):
    cplx = FORMS[form]
    full = ref.sector(M, N)
    keep = LISTS[name]
    bra, ket = pair(len(keep), cplx, 11)
    rho, G = run(full[keep], bra, ket, M, N)
    rho_x, G_x = dref.string_densities(bra, ket, full[keep], M)
    bound = dref.pair_bound(bra, ket)
    check(H(rho), rho_x, bound, f"{form} {name} rho")
    check(H(G), G_x, bound, f"{form} {name} G")
    check_structure(G, f"{form} {name}")


@pytest.mark.parametrize("form", list(FORMS))
def test_a_ket_held_by_the_upper_waves(form):
    """The ket is non-zero only on determinants 128 ... 255: threads of waves 2 and 3 alone read a non-zero ``ket[J]``, so
    G is right only if the closing sum takes all four waves."""
    cplx = FORMS[form]
    full = ref.sector(M, N)
    bra, ket = pair(DIM, cplx, 12)
    ket = ket.copy()
    ket[:128] = 0
    ket[256:] = 0
    rho, G = run(full, bra, ket, M, N)
    rho_x, G_x = dref.string_densities(bra, ket, full, M)
    bound = dref.pair_bound(bra, ket)
    assert float(np.abs(G_x).max()) > 1e-3
    check(H(rho), rho_x, bound, f"{form} upper waves rho")
    check(H(G), G_x, bound, f"{form} upper waves G")


# ---- high orbital indices ------------------------------------------------------------------------------------------------
# The 70 determinants of (8, 4) placed on eight scattered orbitals of a larger m.  The placement keeps the order of the
# orbitals, hence every sign: the compact oracle's densities ARE the answer on the placed block, and no determinant of
# the list holds any other orbital, so every other entry is a sum of nothing.  The output stays on the device (252 MB,
# complex128 at m = 63): the block is gathered there and the rest is counted.


@pytest.mark.parametrize("m", [33, 63])
@pytest.mark.parametrize("form", list(FORMS))
def test_scattered_orbitals_up_to_the_last_bit(form, m):
    cplx = FORMS[form]
    where = np.array(WHERE[m])
    assert m != 63 or WHERE[63] == [0, 15, 31, 32, 33, 47, 61, 62]
    dets8 = ref.sector(8, 4)
    dets = np.array([sum(1 << int(where[i]) for i in range(8) if x >> i & 1) for x in dets8.tolist()], dtype=np.int64)
    assert (np.diff(dets) > 0).all() and int(dets.max()) >> (m - 1) == 1
    bra, ket = pair(70, cplx, 6300 + m)
    rho, G = run(dets, bra, ket, m, 4)
    rho_x, G_x = dref.jw_densities(bra, ket, 8, 4)
    bound = dref.pair_bound(bra, ket)
    w = torch.from_numpy(where).cuda()
    rho_in = rho[w[:, None], w[None, :]]
    G_in = G[w[:, None, None, None], w[None, :, None, None], w[None, None, :, None], w[None, None, None, :]]
    check(H(rho_in), rho_x, bound, f"{form} m={m} rho on the placed orbitals")
    check(H(G_in), G_x, bound, f"{form} m={m} G on the placed orbitals")
    # x != 0 holds for NaN too: equal counts mean that nothing but the block is non-zero and no NaN survived anywhere
    assert int(torch.count_nonzero(rho)) == int(torch.count_nonzero(rho_in)), f"{form} m={m}: rho off the placed orbitals"
    assert int(torch.count_nonzero(G)) == int(torch.count_nonzero(G_in)), f"{form} m={m}: G off the placed orbitals"
    assert int(torch.count_nonzero(G_in)) > 8 ** 4 // 4
    check_structure(G, f"{form} m={m}")


# ---- bits ------------------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("form", list(FORMS))
def test_one_vector_gives_the_bits_of_density1_and_calls_repeat(form):
    from quantum_systems_amd import kernels

    cplx = FORMS[form]
    for m, n in ((8, 4), (M, N)):
        dets = ref.sector(m, n)
        c, other = pair(len(dets), cplx, 77 + m)
        d_dets, d_c, d_o = dev(dets), dev(c), dev(other)
        base = kernels.det_ci_density1(d_dets, d_c, m, n)
        assert torch.equal(kernels.det_ci_transition_density1(d_dets, d_c, d_c, m, n), base)          # the same tensor
        assert torch.equal(kernels.det_ci_transition_density1(d_dets, d_c, d_c.clone(), m, n), base)  # equal values
        first = kernels.det_ci_density2(d_dets, d_c, d_o, m, n)
        again = kernels.det_ci_density2(d_dets, d_c, d_o, m, n, out=nan_out((m,) * 4, cplx))
        assert H(first).tobytes() == H(again).tobytes()
        rho = kernels.det_ci_transition_density1(d_dets, d_c, d_o, m, n)
        assert H(rho).tobytes() == H(kernels.det_ci_transition_density1(d_dets, d_c, d_o, m, n)).tobytes()


def test_a_real_and_a_complex_vector_promote_and_bad_operands_are_refused():
    from quantum_systems_amd import kernels

    m, n = 6, 3
    dets = ref.sector(m, n)
    bra, ket = pair(20, False, 1)[0], pair(20, True, 2)[1]
    d_dets = dev(dets)
    rho = kernels.det_ci_transition_density1(d_dets, dev(bra), dev(ket), m, n)
    G = kernels.det_ci_density2(d_dets, dev(bra), dev(ket), m, n)
    assert rho.dtype == G.dtype == torch.complex128
    rho_x, G_x = dref.jw_densities(bra, ket, m, n)
    bound = dref.pair_bound(bra, ket)
    check(H(rho), rho_x, bound, "real bra, complex ket: rho")
    check(H(G), G_x, bound, "real bra, complex ket: G")
    with pytest.raises(ValueError):
        kernels.det_ci_density2(d_dets, dev(bra)[:19], dev(ket), m, n)
    with pytest.raises(ValueError):
        kernels.det_ci_density2(d_dets, dev(bra), dev(bra), m, n, out=torch.empty(m, m, m, m + 1, dtype=torch.float64, device="cuda"))
    with pytest.raises(Exception):
        kernels.det_ci_density2(d_dets, dev(bra), dev(bra), 64, n)                  # m = 64 does not fit a mask
