"""``kernels.string_ci_one_body`` on the GPU.

The exact value is the host sum of tests/_string_ci_response_ref.py in ``numpy.longdouble`` on the ladder oracle's ``E`` of
each list (which shares nothing with the tables), and for a spin-free operator on a dense sector also
``sum_pq A[p,q] E_pq`` with the dense Jordan-Wigner ``E``.  The bound is derived, not tuned:

    |got - exact| <= gamma_(2 m^2 + 2) one_body(|A_up|, |A_down|, |E_a|, |E_b|, |c|)

-- one element is a sum of at most 2 m^2 terms, every term one fma of a coefficient with an exactly signed copy of c --,
times 2 sqrt 2 where the product is complex (a complex A).  Every comparison prints its worst ratio to the bound before it
asserts."""

import functools

import numpy as np
import pytest
import torch

import _string_ci_ref as ref
import _string_ci_response_ref as rref

pytestmark = pytest.mark.gpu
FORMS = {"f64": (False, False), "real_a_complex_c": (False, True), "c128": (True, True)}      # (A complex, c complex)
S2 = 2.0 * np.sqrt(2.0)
# the launch geometries of tests/test_gpu_string_ci.py: 64, 128 and 256 threads, nb = 1, na = 1, and (11, 4, 4) with 330 x 330
# strings, two tiles along Ib, the second one with 74 live lanes of 256
GEOMETRY = [(7, 3, 3), (8, 4, 3), (9, 4, 4), (9, 5, 0), (9, 0, 5), (6, 6, 3), (11, 4, 4)]


def H(x):
    return torch.as_tensor(x).cpu().numpy()


def dev(x):
    return torch.from_numpy(np.array(x)).cuda()


def draw(shape, cplx, seed):
    rng = np.random.default_rng(seed)
    x = rng.standard_normal(shape)
    return x + 1j * rng.standard_normal(shape) if cplx else x


def ratio_of(err, bound, what):
    r = float((np.asarray(err, dtype=np.float64) / np.where(bound > 0, bound, 1.0)).max())
    print(f"{what}: worst error / bound = {r:.3f}")
    return r


@functools.lru_cache(maxsize=None)
def lists(m, Na, Nb):
    """(sa, sb, Ea, Eb) of the full lists; computed once, never modified."""
    sa, sb = ref.strings(m, Na), ref.strings(m, Nb)
    out = sa, sb, ref.list_E(sa, m), ref.list_E(sb, m)
    for a in out:
        a.setflags(write=False)
    return out


def tables(sa, sb, m, Na, Nb):
    from quantum_systems_amd import kernels

    return kernels.string_ci_table(dev(sa), m, Na), kernels.string_ci_table(dev(sb), m, Nb)


@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("m,Na,Nb", ref.SHAPES)
def test_against_the_dense_oracle(m, Na, Nb, form):
    """Every way to shape the call: A (m, m) and (d, m, m), c (na, nb) and (K, na, nb), spin-free and with another A_down.
    m = 3 is one partial table chunk (9 of 16 columns), m = 4 exactly one, Nb = 0 a beta list of one string."""
    from quantum_systems_amd import kernels

    ac, cc = FORMS[form]
    sa, sb, Ea, Eb = lists(m, Na, Nb)
    na, nb = len(sa), len(sb)
    ta, tb = tables(sa, sb, m, Na, Nb)
    Ed = ref.dense_E(m, Na, Nb).reshape(m * m, na * nb, na * nb)
    worst = 0.0
    for d in (None, 1, 3):
        for K in (None, 1, 3):
            Au, Ad = draw((d or 1, m, m), ac, 31 * m + (d or 0)), draw((d or 1, m, m), ac, 57 * m + (d or 0))
            c = draw((K or 1, na, nb), cc, 7 * (K or 0) + m)
            shape = (() if d is None else (d,)) + (() if K is None else (K,)) + (na, nb)
            give = lambda x, lead: dev(x if lead is not None else x[0])       # noqa: E731
            for down in (None, Ad):
                got = H(kernels.string_ci_one_body(give(Au, d), ta, tb, m, give(c, K), A_down=None if down is None else give(down, d)))
                assert got.shape == shape and got.dtype == (np.complex128 if cc else np.float64)
                lo = Au if down is None else down
                exact, bound = rref.one_body(Au, lo, Ea, Eb, c), rref.one_body_bound(Au, lo, Ea, Eb, c)
                err = np.abs(got.reshape(exact.shape) - exact)
                r = float((err / np.where(bound > 0, bound, 1.0)).max())
                assert r <= 1.0, f"({m},{Na},{Nb}) {form} d={d} K={K} A_down={'A_up' if down is None else 'other'}: ratio {r:.3f}"
                worst = max(worst, r)
                if down is None:
                    # the dense sector's own E: sum_pq A[p,q] E_pq on the flat vectors
                    wide = np.clongdouble if (ac or cc) else np.longdouble
                    dense = np.einsum("xa,aij,kj->xki", Au.reshape(-1, m * m).astype(wide), Ed.astype(wide), c.reshape(len(c), -1).astype(wide))
                    assert (np.abs(got.reshape(dense.shape) - dense) <= bound.reshape(dense.shape)).all()
                else:
                    assert np.abs(exact - rref.one_body(Au, Au, Ea, Eb, c)).max() > 1e-3 or Nb == 0     # A_down is seen
    print(f"one-body ({m},{Na},{Nb}) {form}: worst error / bound = {worst:.3f}")


@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("m,Na,Nb", GEOMETRY)
def test_launch_geometries_with_two_operator_groups(m, Na, Nb, form):
    """d = 5 is two operator groups, the second one of a single operator; K = 2.  For the spin-free operator the result is
    also the project's own ``string_ci_sigma(A_x, 0 W)``, whose path bound with W = 0 is gamma_(3 m^2 + 4) on the same sum of
    moduli."""
    from quantum_systems_amd import kernels

    ac, cc = FORMS[form]
    d, K = 5, 2
    sa, sb, Ea, Eb = lists(m, Na, Nb)
    na, nb = len(sa), len(sb)
    ta, tb = tables(sa, sb, m, Na, Nb)
    Au, Ad = draw((d, m, m), ac, 900 + m), draw((d, m, m), ac, 901 + m)
    c = draw((K, na, nb), cc, m + Na)
    dA, dD, dc = dev(Au), dev(Ad), dev(c)
    tag = f"({m},{Na},{Nb}) {form} {na} x {nb}"
    got = kernels.string_ci_one_body(dA, ta, tb, m, dc, A_down=dD)
    assert tuple(got.shape) == (d, K, na, nb)
    bound = rref.one_body_bound(Au, Ad, Ea, Eb, c)
    assert ratio_of(np.abs(H(got) - rref.one_body(Au, Ad, Ea, Eb, c)), bound, f"{tag} A_up, A_down") <= 1.0
    assert float(got.abs().max()) > 1e3 * float(bound.max())                      # the comparison sees the result
    assert torch.equal(got, kernels.string_ci_one_body(dA, ta, tb, m, dc, A_down=dD))     # a repeated call: identical bits

    free = kernels.string_ci_one_body(dA, ta, tb, m, dc)
    bound = rref.one_body_bound(Au, Au, Ea, Eb, c)
    assert ratio_of(np.abs(H(free) - rref.one_body(Au, Au, Ea, Eb, c)), bound, f"{tag} spin-free") <= 1.0
    assert float(free.abs().max()) > 1e3 * float(bound.max())
    assert torch.equal(free, kernels.string_ci_one_body(dA, ta, tb, m, dc))
    # sigma's bound on the same moduli: gamma_(3 m^2 + 4), 2 sqrt 2 for its complex products
    both = bound * (1.0 + ref.gamma(3 * m * m + 4) / ref.gamma(2 * m * m + 2) * (S2 if (cc and not ac) else 1.0))
    W0 = torch.zeros(m * m, m * m, dtype=dA.dtype, device="cuda")
    for x in range(d):
        sig = kernels.string_ci_sigma(dA[x].contiguous(), W0, ta, tb, dc)
        assert ratio_of(H((free[x] - sig).abs()), both[x], f"{tag} operator {x} against string_ci_sigma(A, 0)") <= 1.0


@pytest.mark.parametrize("form", ["f64", "c128"])
def test_a_truncated_alpha_list_drops_missing_targets(form):
    from quantum_systems_amd import kernels

    ac, cc = FORMS[form]
    m, Na, Nb = 8, 4, 3
    rng = np.random.default_rng(843)
    full = ref.strings(m, Na)
    sa, sb = np.sort(rng.choice(full, len(full) // 2, replace=False)), ref.strings(m, Nb)
    ta, tb = tables(sa, sb, m, Na, Nb)
    Ea, Eb = ref.list_E(sa, m), ref.list_E(sb, m)
    assert np.array_equal(H(ta), ref.table_from_E(Ea)) and np.array_equal(H(tb), ref.table_from_E(Eb))
    assert (H(ta) == 0).sum() > (ref.table_from_E(ref.list_E(full, m)) == 0).sum() // 2 + 1       # targets are missing
    Au, Ad, c = draw((2, m, m), ac, 1), draw((2, m, m), ac, 2), draw((3, len(sa), len(sb)), cc, 9)
    got = H(kernels.string_ci_one_body(dev(Au), ta, tb, m, dev(c), A_down=dev(Ad)))
    bound = rref.one_body_bound(Au, Ad, Ea, Eb, c)
    assert ratio_of(np.abs(got - rref.one_body(Au, Ad, Ea, Eb, c)), bound, f"half of the alpha list, {form}") <= 1.0


def test_orbitals_up_to_62_embedded_in_m_63():
    """(8, 4, 4) at spatial orbitals {0, 15, 31, 32, 33, 47, 61, 62} of m = 63, every other coefficient random and non-zero:
    the result is the plain (8, 4, 4) one (the replacements that exist meet the same coefficients in the same order); both
    bounds are added."""
    from quantum_systems_amd import kernels

    orb = np.array([0, 15, 31, 32, 33, 47, 61, 62])
    m, M = 8, 63
    small = ref.strings(m, 4)
    big = np.array([sum(1 << int(orb[p]) for p in range(m) if (int(x) >> p) & 1) for x in small], dtype=np.int64)
    assert (np.diff(big) > 0).all() and int(big.max()) >> 62 == 1
    A = draw((3, m, m), False, 63)
    gen = torch.Generator(device="cuda").manual_seed(63)
    Ab = torch.randn(3, M, M, generator=gen, device="cuda", dtype=torch.float64) + 2.0
    o = dev(orb)
    Ab[:, o[:, None], o[None, :]] = dev(A)
    ts = kernels.string_ci_table(dev(small), m, 4)
    tb = kernels.string_ci_table(dev(big), M, 4)
    c = draw((2, 70, 70), False, 64)
    plain = kernels.string_ci_one_body(dev(A), ts, ts, m, dev(c))
    got = kernels.string_ci_one_body(Ab, tb, tb, M, dev(c))
    E = ref.list_E(small, m)
    bound = rref.one_body_bound(A, A, E, E, c) * (1.0 + ref.gamma(2 * M * M + 2) / ref.gamma(2 * m * m + 2))
    assert ratio_of(H((got - plain).abs()), bound, "m = 63 embedding of (8,4,4)") <= 1.0
    assert ratio_of(np.abs(H(plain) - rref.one_body(A, A, E, E, c)), bound, "(8,4,4) itself") <= 1.0


@pytest.mark.parametrize("form", list(FORMS))
def test_adjoint(form):
    """<b| A c> = conj(<c| A^+ b>) at (11, 4, 4): each side is within sum_i |b_i| bound_i of its exact value (the dot products
    are taken in longdouble on the host)."""
    from quantum_systems_amd import kernels

    ac, cc = FORMS[form]
    m, Na, Nb = 11, 4, 4
    sa, sb, Ea, Eb = lists(m, Na, Nb)
    ta, tb = tables(sa, sb, m, Na, Nb)
    Au, Ad = draw((1, m, m), ac, 5), draw((1, m, m), ac, 6)
    b, c = draw((1, len(sa), len(sb)), cc, 7), draw((1, len(sa), len(sb)), cc, 8)
    dag = lambda x: np.ascontiguousarray(x.conj().transpose(0, 2, 1))             # noqa: E731
    wide = np.clongdouble if cc else np.longdouble
    Ac = H(kernels.string_ci_one_body(dev(Au), ta, tb, m, dev(c), A_down=dev(Ad))).astype(wide)
    Ab = H(kernels.string_ci_one_body(dev(dag(Au)), ta, tb, m, dev(b), A_down=dev(dag(Ad)))).astype(wide)
    left, right = np.vdot(b.astype(wide), Ac), np.conj(np.vdot(c.astype(wide), Ab))
    tol = float((np.abs(b) * rref.one_body_bound(Au, Ad, Ea, Eb, c)).sum() + (np.abs(c) * rref.one_body_bound(dag(Au), dag(Ad), Ea, Eb, b)).sum())
    print(f"adjoint {form}: |<b|A c> - conj(<c|A^+ b>)| / bound = {abs(left - right) / tol:.3f}, |<b|A c>| = {abs(left):.3e}")
    assert abs(left - right) <= tol and abs(left) > 1e3 * tol


@pytest.mark.parametrize("form", ["f64", "c128"])
def test_consistent_with_the_transition_density(form):
    """<b| A c> = sum_pq A[p,q] rho[q,p] with rho[q,p] = <b| E_pq |c> of ``string_ci_density1`` (bound of one element:
    gamma_(dim + 2) ||b|| ||c||, 2 sqrt 2 complex), at (9, 4, 4)."""
    from quantum_systems_amd import kernels

    ac, cc = FORMS[form]
    m, Na, Nb = 9, 4, 4
    sa, sb, Ea, Eb = lists(m, Na, Nb)
    ta, tb = tables(sa, sb, m, Na, Nb)
    A = draw((1, m, m), ac, 11)
    b, c = draw((1, len(sa), len(sb)), cc, 12), draw((1, len(sa), len(sb)), cc, 13)
    b, c = b / np.linalg.norm(b), c / np.linalg.norm(c)
    wide = np.clongdouble if cc else np.longdouble
    Ac = H(kernels.string_ci_one_body(dev(A[0]), ta, tb, m, dev(c[0]))).astype(wide)
    rho = H(kernels.string_ci_density1(ta, tb, m, dev(b[0]), dev(c[0]))).astype(wide)
    left, right = np.vdot(b[0].astype(wide), Ac), (A[0].astype(wide) * rho.T).sum()
    tol = float((np.abs(b) * rref.one_body_bound(A, A, Ea, Eb, c)).sum())
    tol += float(np.abs(A).sum()) * ref.gamma(len(sa) * len(sb) + 2) * (S2 if cc else 1.0)
    print(f"density {form}: |<b|A c> - sum A rho| / bound = {abs(left - right) / tol:.3f}, |<b|A c>| = {abs(left):.3e}")
    assert abs(left - right) <= tol and abs(left) > 1e2 * tol


def test_out_and_promotion():
    from quantum_systems_amd import kernels

    m, Na, Nb = 4, 2, 1
    sa, sb, Ea, Eb = lists(m, Na, Nb)
    na, nb = len(sa), len(sb)
    ta, tb = tables(sa, sb, m, Na, Nb)
    A, c = dev(draw((2, m, m), False, 1)), dev(draw((3, na, nb), False, 2))
    want = kernels.string_ci_one_body(A, ta, tb, m, c)
    out = torch.full((2, 3, na, nb), float("nan"), dtype=torch.float64, device="cuda")
    back = kernels.string_ci_one_body(A, ta, tb, m, c, out=out)
    assert back is out and torch.equal(out, want)
    one = torch.empty(na, nb, dtype=torch.float64, device="cuda")
    assert kernels.string_ci_one_body(A[1], ta, tb, m, c[2], out=one) is one and torch.equal(one, want[1, 2])
    for bad in (torch.empty(3, 2, na, nb, dtype=torch.float64, device="cuda"), torch.empty(2, 3, na, nb, dtype=torch.complex128, device="cuda"),
                torch.empty(2, 3, na, nb + 1, dtype=torch.float64, device="cuda")[..., :nb], torch.empty(2, 3, na, nb, dtype=torch.float64)):
        with pytest.raises(ValueError):
            kernels.string_ci_one_body(A, ta, tb, m, c, out=bad)
    with pytest.raises(ValueError):
        kernels.string_ci_one_body(A, ta, tb, m, c, out=c)                        # the wrong shape, and an alias
    with pytest.raises(ValueError, match="alias"):
        kernels.string_ci_one_body(A[0], ta, tb, m, c[0], out=c[0])
    with pytest.raises(ValueError):
        kernels.string_ci_one_body(A[:, :3], ta, tb, m, c)
    with pytest.raises(ValueError):
        kernels.string_ci_one_body(A, ta, tb, m, c, A_down=A[0])
    with pytest.raises(ValueError):
        kernels.string_ci_one_body(A, ta, tb, m, c[:, :-1])
    # a real c under a complex A is converted once: the complex form on c + 0 i
    Ac = dev(draw((2, m, m), True, 3))
    got = kernels.string_ci_one_body(Ac, ta, tb, m, c)
    assert got.dtype == torch.complex128 and torch.equal(got, kernels.string_ci_one_body(Ac, ta, tb, m, c.to(torch.complex128)))
    # a real A_down beside a complex A_up is promoted with it
    mixed = kernels.string_ci_one_body(Ac, ta, tb, m, c, A_down=A)
    assert torch.equal(mixed, kernels.string_ci_one_body(Ac, ta, tb, m, c, A_down=A.to(torch.complex128)))
