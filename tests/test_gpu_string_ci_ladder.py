"""``kernels.string_ci_ladder_table`` and ``kernels.string_ci_ladder`` on the GPU.

The table is compared bit for bit with the one of tests/_string_ci_ladder_ref.py, which comes from the textbook ``a_p`` on
lists of masks and shares nothing with the kernels.  The exact value of the operator is that helper's sum in
``numpy.longdouble``, and the bound is derived, not tuned:

    |got - exact| <= gamma_(m + 2) apply(|phi|, |L|, |c|)

-- one element is a sum of at most m terms, every term one fma of a coefficient with an exactly signed copy of c --, times
2 sqrt 2 where the product is complex (a complex phi).  Two operators in a row: the bound of the second on the computed
result of the first, plus the first one's bound carried through the moduli of the second.  Every comparison prints its worst
ratio to the bound before it asserts.

A case is ``(m, Na, Nb, spin, step)``: the ladder of ``spin`` (0 alpha, 1 beta) out of the (Na, Nb) sector, ``step`` = -1
annihilates and +1 creates.  Only sectors that exist are listed."""

import functools

import numpy as np
import pytest
import torch

import _string_ci_ladder_ref as lref
import _string_ci_ref as ref
import _string_ci_response_ref as rref
import _string_ci_spin_density_ref as spref

pytestmark = pytest.mark.gpu
FORMS = {"f64": (False, False), "real_phi_complex_c": (False, True), "c128": (True, True)}      # (phi complex, c complex)
S2 = 2.0 * np.sqrt(2.0)
SMALL = [(3, 1, 1), (4, 2, 2), (4, 3, 1), (4, 1, 0), (4, 4, 2)]


def exists(m, Na, Nb, spin, step):
    return 0 <= (Na + step if spin == 0 else Nb + step) <= m


def every_ladder(shapes):
    return [(m, Na, Nb, spin, step) for m, Na, Nb in shapes for spin in (0, 1) for step in (-1, 1) if exists(m, Na, Nb, spin, step)]


SMALL_CASES = every_ladder(SMALL)
assert (4, 1, 0, 1, 1) in SMALL_CASES and (4, 4, 2, 0, -1) in SMALL_CASES and (4, 1, 0, 1, -1) not in SMALL_CASES
# The launch geometries of tests/test_gpu_string_ci_one_body.py as far as their sectors exist: 64, 128 and 256 threads, a beta
# list of one string, an alpha list of one string whose target has six, and (11, 4, 4): for the beta ladder nb_t = 165 is one
# tile of 256 with 165 live lanes and nb_t = 462 two tiles, the second one with 206 live lanes; for the alpha ladder nb_t = 330
# is two tiles, the second one with 74 live lanes.
GEOMETRY_CASES = ([(7, 3, 3, 0, -1), (7, 3, 3, 1, -1)] + every_ladder([(8, 4, 3), (9, 4, 4)])
                  + [(9, 5, 0, 1, 1), (9, 5, 0, 0, -1), (9, 0, 5, 0, 1), (9, 0, 5, 1, -1), (6, 6, 3, 0, -1), (11, 4, 4, 1, -1), (11, 4, 4, 1, 1), (11, 4, 4, 0, -1)])


def H(x):
    return torch.as_tensor(x).cpu().numpy()


def dev(x):
    return torch.from_numpy(np.array(x)).cuda()


def draw(shape, cplx, seed):
    rng = np.random.default_rng(seed)
    x = rng.standard_normal(shape)
    return x + 1j * rng.standard_normal(shape) if cplx else x


def ratio_of(err, bound, what):
    bound = np.asarray(bound, dtype=np.float64)
    r = float((np.asarray(err, dtype=np.float64) / np.where(bound > 0, bound, 1.0)).max())
    print(f"{what}: worst error / bound = {r:.3f}")
    return r


@functools.lru_cache(maxsize=None)
def strings(m, N):
    s = ref.strings(m, N)
    s.setflags(write=False)
    return s


@functools.lru_cache(maxsize=None)
def one_spin_map(m, N_t, N_s):
    """The helper's map (m, n_t, n_s) between the full lists of N_t and of N_s particles; computed once, never modified."""
    M = lref.ladder(strings(m, N_t), strings(m, N_s), m)
    M.setflags(write=False)
    return M


@functools.lru_cache(maxsize=None)
def device_table(m, N_t, N_s):
    from quantum_systems_amd import kernels

    return kernels.string_ci_ladder_table(dev(strings(m, N_t)), dev(strings(m, N_s)), m)


class Ladder:
    """One case: the map, the device table, the extents of source and target, and the call."""

    def __init__(self, m, Na, Nb, spin, step):
        self.m, self.spin, self.n_alpha = m, spin, Na
        self.source = (Na, Nb)
        self.target = (Na + step, Nb) if spin == 0 else (Na, Nb + step)
        N_s, N_t = self.source[spin], self.target[spin]
        self.M, self.table = one_spin_map(m, N_t, N_s), device_table(m, N_t, N_s)
        self.shape_s = (len(strings(m, Na)), len(strings(m, Nb)))
        self.shape_t = (len(strings(m, self.target[0])), len(strings(m, self.target[1])))

    def __call__(self, phi, c, **kw):
        from quantum_systems_amd import kernels

        return kernels.string_ci_ladder(phi, self.table, self.spin, self.n_alpha, c, **kw)

    def exact(self, phi, c):
        return lref.apply(phi, self.spin, self.n_alpha, self.M, c)

    def bound(self, phi, c):
        return lref.bound(phi, self.spin, self.M, c)

    def moduli(self, phi, x):
        return lref.moduli(phi, self.spin, self.M, x)


# ---- the table ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("m,Na,Nb,spin,step", every_ladder(SMALL + [(11, 4, 4)]))
def test_table_is_the_helpers(m, Na, Nb, spin, step):
    N_s = (Na, Nb)[spin]
    got = H(device_table(m, N_s + step, N_s))
    want = lref.table(one_spin_map(m, N_s + step, N_s))
    assert got.dtype == np.int32 and got.shape == want.shape == (len(strings(m, N_s + step)), m)
    assert np.array_equal(got, want)
    # annihilation hits only p outside J, creation only p inside J, and every such p where the lists are full
    inside = ((strings(m, N_s + step)[:, None] >> np.arange(m)[None, :]) & 1).astype(bool)
    assert np.array_equal(got != 0, inside if step > 0 else ~inside)


@pytest.mark.parametrize("step", [-1, 1])
def test_table_of_half_a_source_list_has_zeros_for_the_missing(step):
    from quantum_systems_amd import kernels

    m, N = 8, 4
    full = ref.strings(m, N)
    source = np.sort(np.random.default_rng(84).choice(full, len(full) // 2, replace=False))
    target = ref.strings(m, N + step)
    got = H(kernels.string_ci_ladder_table(dev(target), dev(source), m))
    assert np.array_equal(got, lref.table(lref.ladder(target, source, m)))
    whole = H(device_table(m, N + step, N))
    assert 0 < (got != 0).sum() < (whole != 0).sum() and ((got != 0) <= (whole != 0)).all()
    # and half a target list: its rows are those of the whole table
    rows = np.sort(np.random.default_rng(85).choice(len(target), len(target) // 2, replace=False))
    part = H(kernels.string_ci_ladder_table(dev(target[rows]), dev(full), m))
    assert np.array_equal(part, whole[rows])


def test_table_with_orbitals_up_to_62():
    """(8, 4) and its neighbours at spatial orbitals {0, 15, 31, 32, 33, 47, 61, 62} of m = 63: the columns of those orbitals
    are the plain (8, .) table, every other column is 0."""
    from quantum_systems_amd import kernels

    orb = np.array([0, 15, 31, 32, 33, 47, 61, 62])
    m, M = 8, 63

    def embed(small):
        return np.array([sum(1 << int(orb[p]) for p in range(m) if (int(x) >> p) & 1) for x in small], dtype=np.int64)

    for N_t in (3, 5):
        source, target = embed(ref.strings(m, 4)), embed(ref.strings(m, N_t))
        assert (np.diff(source) > 0).all() and (np.diff(target) > 0).all() and int(source.max()) >> 62 == 1
        got = H(kernels.string_ci_ladder_table(dev(target), dev(source), M))
        assert got.shape == (len(target), M)
        assert np.array_equal(got, lref.table(lref.ladder(target, source, M)))
        assert np.array_equal(got[:, orb], H(device_table(m, N_t, 4))) and (np.delete(got, orb, axis=1) == 0).all()


# ---- the kernel against the helper -------------------------------------------------------------------------------------------

@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("m,Na,Nb,spin,step", SMALL_CASES)
def test_against_the_helper(m, Na, Nb, spin, step, form):
    """Every way to shape the call: phi (m,) and (d, m), c (na, nb) and (K, na, nb).  m = 3 and m = 4 are one partial chunk of
    table columns; (4, 1, 0) and (4, 4, 2) have lists of one string."""
    pc, cc = FORMS[form]
    L = Ladder(m, Na, Nb, spin, step)
    worst = 0.0
    for d in (None, 1, 3):
        for K in (None, 1, 3):
            phi, c = draw((d or 1, m), pc, 31 * m + (d or 0)), draw((K or 1,) + L.shape_s, cc, 7 * (K or 0) + m + Na)
            got = H(L(dev(phi if d else phi[0]), dev(c if K else c[0])))
            assert got.shape == (() if d is None else (d,)) + (() if K is None else (K,)) + L.shape_t
            assert got.dtype == (np.complex128 if cc else np.float64)
            exact, bound = L.exact(phi, c), L.bound(phi, c)
            r = float((np.abs(got.reshape(exact.shape) - exact) / np.where(bound > 0, bound, 1.0)).max())
            assert r <= 1.0, f"({m},{Na},{Nb}) spin {spin} step {step:+d} {form} d={d} K={K}: ratio {r:.3f}"
            assert float(np.abs(got).max()) > 1e3 * float(bound.max())                # the comparison sees the result
            worst = max(worst, r)
    print(f"ladder ({m},{Na},{Nb}) spin {spin} step {step:+d} {form}: worst error / bound = {worst:.3f}")


@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("m,Na,Nb,spin,step", GEOMETRY_CASES)
def test_launch_geometries_with_two_operator_groups(m, Na, Nb, spin, step, form):
    """d = 5 is two operator groups, the second one of a single operator; K = 2.  A repeated call gives the same bits, and
    so does a vector alone and in the batch."""
    pc, cc = FORMS[form]
    d, K = 5, 2
    L = Ladder(m, Na, Nb, spin, step)
    phi, c = draw((d, m), pc, 900 + m), draw((K,) + L.shape_s, cc, m + Na + spin)
    dphi, dc = dev(phi), dev(c)
    tag = f"({m},{Na},{Nb}) spin {spin} step {step:+d} {form} {L.shape_s} -> {L.shape_t}"
    got = L(dphi, dc)
    assert tuple(got.shape) == (d, K) + L.shape_t
    bound = L.bound(phi, c)
    assert ratio_of(np.abs(H(got) - L.exact(phi, c)), bound, tag) <= 1.0
    assert float(got.abs().max()) > 1e3 * float(bound.max())
    assert torch.equal(got, L(dphi, dc))
    for k in range(K):
        assert torch.equal(got[:, k], L(dphi, dc[k].contiguous()))
    assert torch.equal(got[4], L(dphi[4].contiguous(), dc))                           # the operator of the short group, alone


@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("spin,step", [(0, -1), (1, -1), (0, 1), (1, 1)])
def test_unit_vectors_in_three_groups_are_the_single_calls(spin, step, form):
    """phi = 1 (d = m = 9: three groups, in each of which most p have no coefficient at all) against the m calls with one
    unit vector: the skip of a whole group's zeros changes no bit."""
    pc, cc = FORMS[form]
    m = 9
    L = Ladder(m, 4, 4, spin, step)
    c = draw((2,) + L.shape_s, cc, 17 + spin)
    eye = np.eye(m) + (0j if pc else 0.0)
    dc = dev(c)
    got = L(dev(eye), dc)
    assert tuple(got.shape) == (m, 2) + L.shape_t
    for p in range(m):
        assert torch.equal(got[p], L(dev(eye[p]), dc)), p
    exact = L.exact(eye, c)
    # one term per element: the result is a signed copy
    assert np.array_equal(H(got), exact.astype(H(got).dtype)) and float(got.abs().max()) > 0


# ---- algebra through the kernel at (9, 4, 4) -----------------------------------------------------------------------------------

def two_steps(first, u, second, v, c):
    """``second(v) first(u) c`` on the device, downloaded, and its bound: that of ``second`` on the computed intermediate
    plus that of ``first`` carried through the moduli of ``second``."""
    mid = first(dev(u), dev(c))
    out = H(second(dev(v), mid))
    return out, second.bound(v[None], H(mid)[None])[0, 0] + second.moduli(v[None], first.bound(u[None], c[None])[0])[0, 0]


def pairs(m, pc, seed):
    """(u, v, exact): a random pair, the same unit vector twice, two different unit vectors; ``exact`` where the products
    u_p v_q are exact (a_p and a_q themselves)."""
    e = np.eye(m) + (0j if pc else 0.0)
    return [(draw((m,), pc, seed), draw((m,), pc, seed + 1), False), (e[2], e[2], True), (e[2], e[5], True)]


@pytest.mark.parametrize("form", list(FORMS))
def test_the_two_spins_anticommute(form):
    """a_alpha(u) a_beta(v) c = -a_beta(v) a_alpha(u) c through the two different intermediate sectors (9, 4, 3) and (9, 3, 4):
    what pins the (-1)^n_alpha of a beta ladder."""
    pc, cc = FORMS[form]
    m = 9
    beta_first, then_alpha = Ladder(m, 4, 4, 1, -1), Ladder(m, 4, 3, 0, -1)
    alpha_first, then_beta = Ladder(m, 4, 4, 0, -1), Ladder(m, 3, 4, 1, -1)
    c = draw(beta_first.shape_s, cc, 21)
    for u, v, _ in pairs(m, pc, 40):
        ab, b1 = two_steps(beta_first, v, then_alpha, u, c)
        ba, b2 = two_steps(alpha_first, u, then_beta, v, c)
        assert ab.shape == ba.shape == then_alpha.shape_t
        assert ratio_of(np.abs(ab + ba), b1 + b2, f"(9,4,4) {form}: a_alpha a_beta + a_beta a_alpha") <= 1.0
        assert float(np.abs(ab).max()) > 1e3 * float((b1 + b2).max())


@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("spin", [0, 1])
def test_anticommutator_and_number_operator_of_one_spin(spin, form):
    """a(u) a+(v) c + a+(v) a(u) c = (sum_p u_p v_p) c, and a+(u) (a(v) c) is ``string_ci_one_body`` with A = u v^T on that spin
    and 0 on the other, within the bound of the two ladder steps plus that of the one-body kernel."""
    from quantum_systems_amd import kernels

    pc, cc = FORMS[form]
    m, Na, Nb = 9, 4, 4
    down, up = Ladder(m, Na, Nb, spin, -1), Ladder(m, Na, Nb, spin, +1)
    back_up, back_down = Ladder(m, *down.target, spin, +1), Ladder(m, *up.target, spin, -1)
    c = draw(down.shape_s, cc, 23 + spin)
    sa, sb = strings(m, Na), strings(m, Nb)
    Ea, Eb = ref.list_E(sa, m), ref.list_E(sb, m)
    ta = kernels.string_ci_table(dev(sa), m, Na)
    for u, v, exact in pairs(m, pc, 50 + spin):
        first, b1 = two_steps(up, v, back_down, u, c)                                 # a(u) a+(v) c
        second, b2 = two_steps(down, u, back_up, v, c)                                # a+(v) a(u) c
        want = np.sum(u * v) * c
        tol = b1 + b2 + (m + 2) * ref.EPS * np.abs(want) * (S2 if pc else 1.0)        # and the host's own product
        assert ratio_of(np.abs(first + second - want), tol, f"(9,4,4) spin {spin} {form}: anticommutator") <= 1.0
        assert float(np.abs(first).max()) > 1e3 * float(tol.max())
        # the number-conserving product against the one-body kernel
        A = np.multiply.outer(v, u)[None]                                             # a+(v) a(u) = sum v_p u_q E_pq
        Aa, Ab = (A, 0 * A) if spin == 0 else (0 * A, A)
        one = H(kernels.string_ci_one_body(dev(Aa), ta, ta, m, dev(c), A_down=dev(Ab)))[0]
        # both bounds.  For e_p e_q^T the matrix A is exact; for the random pair every entry of A is one rounded product, a
        # relative error of eps (2 sqrt 2 eps for a complex product) that the operator carries on the moduli
        ob = rref.one_body_bound(Aa, Ab, Ea, Eb, c[None])[0, 0]
        rounded = 0.0 if exact else ref.EPS * ob / ref.gamma(2 * m * m + 2)          # ob = gamma (S2 if complex) sum of moduli
        tol = b2 + ob + rounded
        assert ratio_of(np.abs(second - one), tol, f"(9,4,4) spin {spin} {form}: a+ a against string_ci_one_body") <= 1.0


@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("spin", [0, 1])
def test_adjoint(spin, form):
    """<b| a(u) c> = conj(<c| a+(conj u) b>) with b in the smaller sector; the dot products are taken in longdouble on the host,
    each side within sum_i |x_i| bound_i of its exact value."""
    pc, cc = FORMS[form]
    m = 9
    down = Ladder(m, 4, 4, spin, -1)
    up = Ladder(m, *down.target, spin, +1)
    u = draw((1, m), pc, 61 + spin)
    c, b = draw((1,) + down.shape_s, cc, 62), draw((1,) + down.shape_t, cc, 63)
    wide = np.clongdouble if cc else np.longdouble
    ac = H(down(dev(u), dev(c))).astype(wide)
    ab = H(up(dev(u.conj()), dev(b))).astype(wide)
    left, right = np.vdot(b.astype(wide), ac), np.conj(np.vdot(c.astype(wide), ab))
    tol = float((np.abs(b) * down.bound(u, c)[0]).sum() + (np.abs(c) * up.bound(u.conj(), b)[0]).sum())
    print(f"adjoint spin {spin} {form}: |<b|a c> - conj(<c|a+ b>)| / bound = {abs(left - right) / tol:.3f}, |<b|a c>| = {abs(left):.3e}")
    assert abs(left - right) <= tol and abs(left) > 1e3 * tol


@pytest.mark.parametrize("form", ["f64", "c128"])
def test_overlaps_of_the_hole_states_are_the_spin_density(form):
    """<a_p c| a_q c> = rho_s[q, p] of ``string_ci_density2_spin`` at (9, 4, 4), the m hole states from one call with phi = 1.
    Tolerance: the ladder's bound through the host's dot product (its own rounding is in longdouble) plus the density's
    bound of tests/test_gpu_string_ci_spin_density.py."""
    from quantum_systems_amd import kernels

    pc, cc = FORMS[form]
    m, Na, Nb = 9, 4, 4
    s = strings(m, 4)
    E = ref.list_E(s, m)
    c = draw((len(s), len(s)), cc, 71)
    c = c / np.linalg.norm(c)
    t = kernels.string_ci_table(dev(s), m, 4)
    out = kernels.string_ci_density2_spin(t, t, m, dev(c), dev(c))
    T = kernels.string_ci_density2_spin_plan(m, len(s), len(s), torch.complex128 if cc else torch.float64)[2]
    _, rB = spref.spin_gamma_bound(E, E, c, c, T)
    eye = np.eye(m) + (0j if pc else 0.0)
    wide = np.clongdouble if cc else np.longdouble
    for spin in (0, 1):
        L = Ladder(m, Na, Nb, spin, -1)
        X = H(L(dev(eye), dev(c)))                                                    # (m, na_t, nb_t)
        Xb = L.bound(eye, c[None])[:, 0]
        flat, fb = X.reshape(m, -1).astype(wide), Xb.reshape(m, -1)
        gram = flat.conj() @ flat.T                                                   # gram[p, q] = <a_p c| a_q c>
        tol = np.abs(flat).astype(np.float64) @ fb.T + fb @ np.abs(flat).astype(np.float64).T + fb @ fb.T + rB[spin].T
        rho = H(out[3 + spin])
        assert ratio_of(np.abs(gram - rho.T), tol, f"(9,4,4) spin {spin} {form}: hole overlaps against rho") <= 1.0
        assert abs(np.trace(gram).real - 4.0) < 1e-12 and float(np.abs(gram).max()) > 1e3 * float(tol.max())


# ---- out= and the promotions ---------------------------------------------------------------------------------------------------

def test_out_and_promotion():
    from quantum_systems_amd import kernels

    m = 4
    L = Ladder(m, 2, 1, 0, -1)
    (na, nb), (nt, _) = L.shape_s, L.shape_t
    phi, c = dev(draw((2, m), False, 1)), dev(draw((3, na, nb), False, 2))
    want = L(phi, c)
    out = torch.full((2, 3, nt, nb), float("nan"), dtype=torch.float64, device="cuda")
    assert L(phi, c, out=out) is out and torch.equal(out, want)
    one = torch.empty(nt, nb, dtype=torch.float64, device="cuda")
    assert L(phi[1], c[2], out=one) is one and torch.equal(one, want[1, 2])
    for bad in (torch.empty(3, 2, nt, nb, dtype=torch.float64, device="cuda"), torch.empty(2, 3, nt, nb, dtype=torch.complex128, device="cuda"),
                torch.empty(2, 3, nt, nb + 1, dtype=torch.float64, device="cuda")[..., :nb], torch.empty(2, 3, nt, nb, dtype=torch.float64),
                torch.empty(2, 3, na, nb, dtype=torch.float64, device="cuda")):
        with pytest.raises(ValueError):
            L(phi, c, out=bad)
    flat = torch.zeros(max(na, nt) * nb, dtype=torch.float64, device="cuda")
    with pytest.raises(ValueError, match="alias"):
        L(phi[0], flat[:na * nb].view(na, nb), out=flat[:nt * nb].view(nt, nb))
    with pytest.raises(ValueError):
        L(phi[:, :3], c)
    with pytest.raises(ValueError):
        kernels.string_ci_ladder(phi, L.table, 2, 2, c)
    with pytest.raises(ValueError):
        kernels.string_ci_ladder(phi, L.table.to(torch.int64), 0, 2, c)
    # the table too
    tab = torch.full((nt, m), -7, dtype=torch.int32, device="cuda")
    assert kernels.string_ci_ladder_table(dev(strings(m, 1)), dev(strings(m, 2)), m, out=tab) is tab and torch.equal(tab, L.table)
    with pytest.raises(ValueError):
        kernels.string_ci_ladder_table(dev(strings(m, 1)), dev(strings(m, 2)), m, out=tab[:, :3])
    # a real c under a complex phi is converted once: the complex form on c + 0 i
    pz = dev(draw((2, m), True, 3))
    got = L(pz, c)
    assert got.dtype == torch.complex128 and torch.equal(got, L(pz, c.to(torch.complex128)))
    # a real phi with a complex c stays real: the result is the real kernel on the two parts
    cz = dev(draw((3, na, nb), True, 4))
    mixed = L(phi, cz)
    assert mixed.dtype == torch.complex128
    assert torch.equal(mixed.real, L(phi, cz.real.contiguous())) and torch.equal(mixed.imag, L(phi, cz.imag.contiguous()))
