"""``kernels.string_ci_density2_spin`` and ``StringCI``'s spin-resolved observables on it, on the GPU.

Tolerances (derived, not tuned; tests/_string_ci_spin_density_ref.py states them):
  * Gamma^st, elementwise: gamma_(dim+T+3) ( sum_K |E^s_rp bra| |E^t_qs ket| + delta_st delta_qr sum_K |bra| |E^s_ps ket| ),
    2 sqrt 2 for complex128 -- the dot-product bound, valid for any order of accumulation, with T the partial sums of the
    schedule (``qs_string_ci_density2_spin_plan``); rho^s by its own row, gamma_(dim+T+3) sum_K |bra| |E^s_pq ket|;
  * a sum of n elements (the spin sum, a trace, a partial trace, a symmetry that compares two): the sum of their bounds;
  * against ``string_ci_density2`` / ``string_ci_density1``: plus those kernels' own bounds (tests/_string_ci_density_ref.py,
    gamma_(dim+2) for unit vectors in ``string_ci_density1``);
  * against the project's ``det_ci_density2`` on ``determinant_order``: plus that test's own gamma_(dim+2) |bra| |ket|
    (``pair_bound``) for the one element of it that a spin block holds.
Every comparison prints its worst ratio to the bound before it asserts."""

import functools

import numpy as np
import pytest
import torch

import _det_ci_density_ref as ddref
import _det_ci_ref as dref
import _string_ci_density_ref as sref
import _string_ci_ref as ref
import _string_ci_spin_density_ref as spref

pytestmark = pytest.mark.gpu
FORMS = {"f64": False, "c128": True}
S2 = spref.S2
SPIN_OF = {"aa": (0, 0), "ab": (0, 1), "bb": (1, 1)}


def H(x):
    return torch.as_tensor(x).cpu().numpy()


def dev(x):
    return torch.from_numpy(np.array(x)).cuda()


def unit_pair(na, nb, cplx, seed):
    rng = np.random.default_rng(seed)
    c = rng.standard_normal((2, na, nb))
    if cplx:
        c = c + 1j * rng.standard_normal((2, na, nb))
    return c[0] / np.linalg.norm(c[0]), c[1] / np.linalg.norm(c[1])


def tables(sa, sb, m, Na, Nb):
    from quantum_systems_amd import kernels

    ta = kernels.string_ci_table(dev(sa), m, Na)
    return ta, (ta if sa is sb else kernels.string_ci_table(dev(sb), m, Nb))


def ratio_of(err, bound, what):
    bound = np.asarray(bound, dtype=np.float64)
    r = float((np.asarray(err, dtype=np.float64) / np.where(bound > 0, bound, 1.0)).max())
    print(f"{what}: worst error / bound = {r:.3f}")
    return r


def plan(m, na, nb, cplx):
    """(rows, passes, T, kc, bytes) of the schedule ``string_ci_density2_spin`` runs under the calling thread's tuning."""
    from quantum_systems_amd import kernels

    return kernels.string_ci_density2_spin_plan(m, na, nb, torch.complex128 if cplx else torch.float64)


def spin_call(ta, tb, m, db, dk):
    """The call, downloaded: ({"aa", "ab", "bb"} -> Gamma^st, (rho^a, rho^b))."""
    from quantum_systems_amd import kernels

    out = kernels.string_ci_density2_spin(ta, tb, m, db, dk)
    assert len(out) == 5 and all(x.dtype == db.dtype for x in out)
    assert all(x.shape == (m, m, m, m) for x in out[:3]) and all(x.shape == (m, m) for x in out[3:])
    return dict(zip(spref.BLOCKS, (H(x) for x in out[:3]))), (H(out[3]), H(out[4]))


@functools.lru_cache(maxsize=None)
def one_spin(m, N):
    """(strings, E of the list) of one spin; computed once, never modified."""
    s = ref.strings(m, N)
    E = ref.list_E(s, m)
    for a in (s, E):
        a.setflags(write=False)
    return s, E


@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("m,Na,Nb", ref.SHAPES)
def test_blocks_against_the_host_oracle_and_the_spin_summed_kernels(m, Na, Nb, form):
    from quantum_systems_amd import kernels

    cc = FORMS[form]
    (sa, Ea), (sb, Eb) = one_spin(m, Na), one_spin(m, Nb)
    na, nb = len(sa), len(sb)
    count = {"a": Na, "b": Nb}
    ta, tb = tables(sa, sb, m, Na, Nb)
    T = plan(m, na, nb, cc)[2]
    Tsum = int(ref_plan_T(m, na, nb, cc))
    bra, ket = unit_pair(na, nb, cc, 7 + m)
    for b, k, what in ((bra, bra, "state"), (bra, ket, "pair")):
        tag = f"({m},{Na},{Nb}) {form} {what}"
        db = dev(b)
        dk = db if k is b else dev(k)
        G, rho = spin_call(ta, tb, m, db, dk)
        Gx, rhox = spref.spin_gamma(Ea, Eb, b, k)
        B, rB = spref.spin_gamma_bound(Ea, Eb, b, k, T)
        for st in spref.BLOCKS:
            assert ratio_of(np.abs(G[st] - Gx[st]), B[st], f"{tag} Gamma^{st}") <= 1.0
        for s, r, rx, rb in zip("ab", rho, rhox, rB):
            assert ratio_of(np.abs(r - rx), rb, f"{tag} rho^{s}") <= 1.0
        # the existing kernels: the spin sum against string_ci_density2, rho^a + rho^b against string_ci_density1
        Gs, _ = kernels.string_ci_density2(ta, tb, m, db, dk)
        sum_bound = spref.spin_sum(B) + sref.gamma_bound((Ea, Eb), b, k, Tsum)
        assert ratio_of(np.abs(spref.spin_sum(G) - H(Gs)), sum_bound, f"{tag} spin sum against string_ci_density2") <= 1.0
        rho1 = H(kernels.string_ci_density1(ta, tb, m, db, dk))
        one_bound = rB[0] + rB[1] + ref.gamma(na * nb + 2) * (S2 if cc else 1.0)
        assert ratio_of(np.abs(rho[0] + rho[1] - rho1), one_bound, f"{tag} rho^a + rho^b against string_ci_density1") <= 1.0
        # exchange symmetry of the equal-spin blocks (two elements each)
        for st in ("aa", "bb"):
            assert ratio_of(np.abs(G[st] + G[st].transpose(1, 0, 2, 3)), B[st] + B[st].transpose(1, 0, 2, 3),
                            f"{tag} Gamma^{st}[p,q] = -Gamma^{st}[q,p]") <= 1.0
            assert ratio_of(np.abs(G[st] + G[st].transpose(0, 1, 3, 2)), B[st] + B[st].transpose(0, 1, 3, 2),
                            f"{tag} Gamma^{st}[r,s] = -Gamma^{st}[s,r]") <= 1.0
        # both trace rules
        overlap = np.vdot(b, k)
        for st in spref.BLOCKS:
            s, t = st
            fac = count[t] - (1 if s == t else 0)
            r_s, rb_s = rho["ab".index(s)], rB["ab".index(s)]
            assert ratio_of(np.abs(np.einsum("pqrq->pr", G[st]) - fac * r_s.T), np.einsum("pqrq->pr", B[st]) + fac * rb_s.T,
                            f"{tag} partial trace of Gamma^{st}") <= 1.0
            assert ratio_of(abs(np.einsum("pqpq->", G[st]) - count[s] * fac * overlap),
                            np.float64(np.einsum("pqpq->", B[st]) + 4 * ref.EPS * count[s] * fac * abs(overlap)),
                            f"{tag} trace of Gamma^{st}") <= 1.0
        if k is b:
            for st in spref.BLOCKS:
                Bh = B[st] + B[st].transpose(2, 3, 0, 1)
                assert ratio_of(np.abs(G[st] - G[st].transpose(2, 3, 0, 1).conj()), Bh, f"{tag} Hermiticity of Gamma^{st}") <= 1.0
        if Na and Nb:
            assert float(np.abs(G["ab"]).max()) > 1e3 * float(B["ab"].max())       # the comparison sees the result


def ref_plan_T(m, na, nb, cplx):
    """T of the spin-summed ``qs_string_ci_density2`` under the calling thread's tuning (for its own bound)."""
    import ctypes

    from quantum_systems_amd import _lib, kernels

    out = (ctypes.c_int64 * 5)()
    assert _lib.load().qs_string_ci_density2_plan(1 if cplx else 0, m, na, nb, kernels.STRING_CI_BYTES, ctypes.cast(out, ctypes.c_void_p)) == 0
    return out[2]


def det_blocks(sa, sb, m, bra, ket):
    """The project's det_ci_density2 on the interleaved determinants: its three spin blocks, each ONE of its elements."""
    from quantum_systems_amd import kernels
    from quantum_systems_amd.string_ci import determinant_order

    masks, perm, phase = determinant_order(sa, sb)
    N = dref.popcount(int(masks[0]))
    ph, pm = dev(phase).to(bra.dtype), dev(perm)
    vb = (bra.reshape(-1) * ph)[pm].contiguous()
    vk = vb if ket is bra else (ket.reshape(-1) * ph)[pm].contiguous()
    G = kernels.det_ci_density2(dev(masks), vb, vk, 2 * m, N)
    return {st: H(G[a::2, b::2, a::2, b::2]) for st, (a, b) in SPIN_OF.items()}


# (11, 4, 4): 330 x 330, the 256-thread workgroup, two tiles along Ib, the second one with 74 live lanes of 256;
# m = 7, 9, 11: m^2 off the 16-column chunk and odd (the fp64 ket panel has a pad column per spin);
# (9, 5, 0) and (9, 0, 5): an empty spin on either side, the list [0] and a table of zeros
GEOMETRY = [(7, 3, 3), (9, 5, 0), (9, 0, 5), (6, 6, 3), (11, 4, 4)]


@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("m,Na,Nb", GEOMETRY)
def test_launch_and_alignment_geometries_against_det_ci_density2(m, Na, Nb, form):
    from quantum_systems_amd import kernels

    cc = FORMS[form]
    (sa, Ea), (sb, Eb) = one_spin(m, Na), one_spin(m, Nb)
    na, nb = len(sa), len(sb)
    ta, tb = tables(sa, sb, m, Na, Nb)
    T = plan(m, na, nb, cc)[2]
    bra, ket = unit_pair(na, nb, cc, m + Na)
    db, dk = dev(bra), dev(ket)
    out = kernels.string_ci_density2_spin(ta, tb, m, db, dk)
    want = det_blocks(sa, sb, m, db, dk)
    B, _ = spref.spin_gamma_bound(Ea, Eb, bra, ket, T)
    pair = ddref.pair_bound(bra.reshape(-1), ket.reshape(-1))
    tag = f"({m},{Na},{Nb}) {form} {na} x {nb}, T = {T}"
    for st, G in zip(spref.BLOCKS, out[:3]):
        assert ratio_of(np.abs(H(G) - want[st]), B[st] + pair, f"{tag} Gamma^{st}") <= 1.0
        s, t = st
        empty = (Na if s == "a" else Nb) == 0 or (Na if t == "a" else Nb) == 0 or (s == t and (Na if s == "a" else Nb) < 2)
        if empty:
            assert not G.any()                                                    # an empty spin: exact zeros
        else:
            assert float(G.abs().max()) > 1e3 * float((B[st] + pair).max())       # the comparison sees the result
    again = kernels.string_ci_density2_spin(ta, tb, m, db, dk)
    assert all(torch.equal(x, y) for x, y in zip(out, again))                     # a repeated call: identical bits


@pytest.mark.parametrize("form", list(FORMS))
def test_passes_under_three_byte_budgets(form):
    """(9, 4, 4), 126 x 126: one pass, several equal passes, and a ragged last pass whose slices end in zeros."""
    from quantum_systems_amd import kernels

    cc = FORMS[form]
    m, Na, Nb = 9, 4, 4
    sa, Ea = one_spin(m, Na)
    na = nb = len(sa)
    count = {"a": Na, "b": Nb}
    ta, tb = tables(sa, sa, m, Na, Nb)
    es = 16 if cc else 8
    h = m * m if cc else m * m + (m * m & 1)
    budgets = {}
    for r in range(na, 0, -1):
        budget = (2 * m * m + 1 + 2 * h) * (r * nb + 64) * es
        with kernels.tuning(string_ci_bytes=budget):
            rows, passes, T, kc, _ = plan(m, na, nb, cc)
        if passes == 1:
            kind = "one"
        elif na % rows == 0:
            kind = "equal" if passes >= 3 else None
        else:
            kind = "ragged"                                                      # the last pass ends inside the slices
            assert (na - (passes - 1) * rows) * nb < T * kc
        if kind:
            budgets.setdefault(kind, (budget, rows, passes, T, kc))
    assert set(budgets) >= {"one", "equal", "ragged"}, budgets
    bra, ket = unit_pair(na, nb, cc, 94)
    db, dk = dev(bra), dev(ket)
    Tmax = max(b[3] for b in budgets.values())
    B, rB = spref.spin_gamma_bound(Ea, Ea, bra, ket, Tmax)
    got = {}
    for kind, (budget, rows, passes, T, kc) in budgets.items():
        kernels.dispatch_log = log = []
        try:
            with kernels.tuning(string_ci_bytes=budget):
                assert plan(m, na, nb, cc)[:4] == (rows, passes, T, kc)
                G, rho = spin_call(ta, tb, m, db, dk)
        finally:
            kernels.dispatch_log = None
        print(f"{form} {kind}: {passes} passes of {rows} rows, T = {T}, kc = {kc}, last pass {(na - (passes - 1) * rows) * nb} of {T * kc}")
        assert len(log) == 1 and "string_ci" in log[0], log                       # one entry names the whole call
        w = 2 if cc else 1
        for name in (f"string_ci_expand_panel_kernel<{w}, false, 2>", f"string_ci_expand_panel_kernel<{w}, true, 2>", "gemm",
                     f"string_ci_gamma_close_kernel<{w}>"):
            assert name in log[0], (name, log[0])
        assert "det_ci" not in log[0] and "string_ci_expand_kernel" not in log[0]
        got[kind] = G
        # oracle-free, per block: sum_q Gamma^st[p,q,r,q] = (N_t - delta_st) rho^s[r,p]
        for st in spref.BLOCKS:
            s, t = st
            fac = count[t] - (1 if s == t else 0)
            r_s, rb_s = rho["ab".index(s)], rB["ab".index(s)]
            err = np.abs(np.einsum("pqrq->pr", G[st]) - fac * r_s.T)
            assert ratio_of(err, np.einsum("pqrq->pr", B[st]) + fac * rb_s.T, f"{form} {kind}: partial trace of Gamma^{st}") <= 1.0
    for kind in ("equal", "ragged"):
        for st in spref.BLOCKS:
            assert ratio_of(np.abs(got[kind][st] - got["one"][st]), 2 * B[st], f"{form} {kind} against one pass, Gamma^{st}") <= 1.0
    for st in spref.BLOCKS:
        assert float(np.abs(got["one"][st]).max()) > 1e3 * float(B[st].max())


@pytest.mark.parametrize("form", list(FORMS))
def test_the_close_past_its_grid_cap_on_one_particle_per_spin(form):
    """m = 49, one particle per spin, the 49 strings ``1 << i`` on either side: 3 m^4 = 17 294 403 elements of the three Gamma
    against the close's cap of 65 536 workgroups of 256 threads = 16 777 216, so its grid-stride loop takes a second trip (the
    last 517 187 elements of Gamma^bb, and the rho^b they write).  One pass of 2401 determinants.  The outputs are handed in
    full of NaN: an element the close does not write fails.

    String i is orbital i and every sign is +, so (E^a_pq c)[Ia, Ib] = delta(Ia, p) c[q, Ib] and (E^b_pq c)[Ia, Ib] =
    delta(Ib, p) c[Ia, q], and the densities have closed forms (host: longdouble):
      * Gamma^ab[p,q,r,s] = conj(bra[p,q]) ket[r,s]: ONE non-zero term in the dot product over the determinants, every other
        term and every partial sum an exact zero.  fp64: one rounding, that of the product.  complex128: the two products and
        one addition of a real or imaginary part are at most two roundings, sqrt 2 gamma_2 for the modulus.  The bound is
        gamma_2 |bra[p,q]| |ket[r,s]|, times the suite's 2 sqrt 2 for complex128.
      * rho^a[q,p] = sum_b conj(bra[p,b]) ket[q,b], rho^b[q,p] = sum_a conj(bra[a,p]) ket[a,q]: nb (na) non-zero terms, spread
        over at most T partial sums that are then added: at most nb + T - 1 additions and one product rounding each,
        gamma_(nb+T+1) sum |bra| |ket| for any order (the exact zeros among the terms add nothing).
      * Gamma^aa[p,q,r,s] = delta_qr (X - <E^a_ps>) with X = <E^a_ps> = sum_b conj(bra[p,b]) ket[s,b] in exact arithmetic:
        zero, and on the device the difference of two such sums, each within gamma_(nb+T+1) sum_b |bra[p,b]| |ket[s,b]| of
        the same number (the final subtraction rounds a difference that small by less than the slack between gamma_(nb+T)
        and gamma_(nb+T+1)): twice that.  For q != r every term is an exact zero: exact zeros.  Gamma^bb likewise over a."""
    from quantum_systems_amd import kernels

    cc = FORMS[form]
    m = 49
    cap = 65536 * 256
    assert 2 * m ** 4 < cap < 3 * m ** 4                                          # the second trip exists, in Gamma^bb
    s = np.array([1 << i for i in range(m)], dtype=np.int64)
    ta = kernels.string_ci_table(dev(s), m, 1)
    assert np.array_equal(H(ta).reshape(m, m, m), np.eye(m, dtype=np.int32)[:, :, None] * (np.arange(m, dtype=np.int32) + 1))
    rows, passes, T, kc, _ = plan(m, m, m, cc)
    assert passes == 1 and rows == m
    bra, ket = unit_pair(m, m, cc, 49)
    dt = torch.complex128 if cc else torch.float64
    out = tuple(torch.full(shape, float("nan"), dtype=dt, device="cuda") for shape in ((m,) * 4,) * 3 + ((m, m),) * 2)
    got = kernels.string_ci_density2_spin(ta, ta, m, dev(bra), dev(ket), out=out)
    assert all(g is o for g, o in zip(got, out))
    G = dict(zip(spref.BLOCKS, (H(x) for x in out[:3])))
    rho = (H(out[3]), H(out[4]))
    # every element is compared below; those of the loop's second trip lie past cap - 2 m^4 in Gamma^bb
    assert all(x.size == m ** 4 and np.isfinite(x.reshape(-1)[cap // 3:]).all() for x in G.values())
    cx = S2 if cc else 1.0
    bw, kw, ab, ak = ref._wide(bra), ref._wide(ket), np.abs(bra), np.abs(ket)
    tag = f"m = 49 {form}, T = {T}"
    want = np.multiply.outer(bw.conj(), kw)
    bound = ref.gamma(2) * cx * np.multiply.outer(ab, ak)
    assert ratio_of(np.abs(G["ab"] - want), bound, f"{tag} Gamma^ab") <= 1.0
    assert float(np.abs(G["ab"]).max()) > 1e3 * float(bound.max())                # the comparison sees the result
    del want, bound
    # e[p, q] = <bra| E^s_pq |ket> and sum |bra| |E^s_pq ket|, alpha over b and beta over a
    e = {"a": bw.conj() @ kw.T, "b": bw.conj().T @ kw}
    eb = {"a": ab @ ak.T, "b": ab.T @ ak}
    scale = ref.gamma(m + T + 1) * cx
    for spin, r in zip("ab", rho):
        assert ratio_of(np.abs(r - e[spin].T), scale * eb[spin].T, f"{tag} rho^{spin}") <= 1.0
        assert float(np.abs(r).max()) > 1e3 * float(scale * eb[spin].max())
        g = G[spin + spin].transpose(1, 2, 0, 3)                                  # [q, r, p, s]
        assert not g[~np.eye(m, dtype=bool)].any()                                # q != r: exact zeros
        diag = g[np.arange(m), np.arange(m)]                                      # [q, p, s], X - <E^s_ps>
        assert ratio_of(np.abs(diag), np.broadcast_to(2 * scale * eb[spin], diag.shape), f"{tag} Gamma^{spin}{spin}") <= 1.0


@pytest.mark.parametrize("form", list(FORMS))
def test_a_truncated_alpha_list_against_the_cut_intermediate(form):
    """A random half of the alpha list of (7, 3, 3): E^t_qs ket is cut to the lists before E^s_pr acts."""
    cc = FORMS[form]
    m, Na, Nb = 7, 3, 3
    rng = np.random.default_rng(733)
    full = ref.strings(m, Na)
    sa, sb = np.sort(rng.choice(full, len(full) // 2, replace=False)), ref.strings(m, Nb)
    na, nb = len(sa), len(sb)
    ta, tb = tables(sa, sb, m, Na, Nb)
    Ea, Eb = ref.list_E(sa, m), ref.list_E(sb, m)
    assert np.array_equal(H(ta), ref.table_from_E(Ea)) and (H(ta) == 0).sum() > (ref.table_from_E(ref.list_E(full, m)) == 0).sum() // 2 + 1
    T = plan(m, na, nb, cc)[2]
    bra, ket = unit_pair(na, nb, cc, 8)
    for b, k, what in ((bra, bra, "state"), (bra, ket, "pair")):
        db = dev(b)
        G, rho = spin_call(ta, tb, m, db, db if k is b else dev(k))
        Gx, rhox = spref.spin_gamma(Ea, Eb, b, k)
        B, rB = spref.spin_gamma_bound(Ea, Eb, b, k, T)
        for st in spref.BLOCKS:
            assert ratio_of(np.abs(G[st] - Gx[st]), B[st], f"half of the alpha list, {form} {what}: Gamma^{st}") <= 1.0
            assert float(np.abs(G[st]).max()) > 1e3 * float(B[st].max())
        for s, r, rx, rb in zip("ab", rho, rhox, rB):
            assert ratio_of(np.abs(r - rx), rb, f"half of the alpha list, {form} {what}: rho^{s}") <= 1.0


@pytest.mark.parametrize("form", list(FORMS))
def test_spin_squared_read_off_the_opposite_spin_block(form):
    """(7, 3, 3), a state: S_z (S_z + 1) + N_b - sum_pq Gamma^ab[q,p,p,q] against <c| S^2 c> of ``string_ci_spin_squared``,
    the dot product in longdouble on the host; the bound is the m^2 elements of Gamma^ab plus that kernel's own
    elementwise bound weighted by |c|."""
    from quantum_systems_amd import kernels

    cc = FORMS[form]
    m, Na, Nb = 7, 3, 3
    (sa, Ea), (sb, Eb) = one_spin(m, Na), one_spin(m, Nb)
    na, nb = len(sa), len(sb)
    ta, tb = tables(sa, sb, m, Na, Nb)
    T = plan(m, na, nb, cc)[2]
    c, _ = unit_pair(na, nb, cc, 73)
    dc = dev(c)
    G, _ = spin_call(ta, tb, m, dc, dc)
    got = spref.spin_squared(G, Na, Nb)
    Sc = H(kernels.string_ci_spin_squared(ta, tb, m, Na, Nb, dc))
    want = np.sum(ref._wide(c).conj() * ref._wide(Sc))
    B, _ = spref.spin_gamma_bound(Ea, Eb, c, c, T)
    bound = float(np.einsum("qppq->", B["ab"]) + np.sum(np.abs(c) * sref.spin_bound(Ea, Eb, Na, Nb, c[None])[0]))
    bound += ref.gamma(m * m + 2) * (abs(sref.spin_s0(Na, Nb)) + float(np.einsum("qppq->", np.abs(G["ab"]))))     # the host's own sum
    assert ratio_of(abs(got - want), np.float64(bound), f"(7,3,3) {form}: <S^2> off Gamma^ab against <c|S^2 c>") <= 1.0
    assert abs(want) > 1e3 * bound


# ---- solver level ------------------------------------------------------------------------------------------------------


def random_spatial_system(l, n, seed, cplx):
    """The system of test_gpu_string_ci.py's solver test: a seeded RandomBasisSet made physical, 2 n electrons."""
    import quantum_systems_amd as qsa

    np.random.seed(seed)
    bs = qsa.RandomBasisSet(l, 2)
    part = (lambda x: x) if cplx else (lambda x: np.ascontiguousarray(x.real))
    bs.h = part(bs.h)
    s = part(bs.s)
    bs.s = np.eye(l) + 0.1 * (s - np.diag(np.diag(s)))
    u = 0.3 * part(bs.u)
    u = u + u.conj().transpose(2, 3, 0, 1)
    bs.u = u + u.transpose(1, 0, 3, 2)
    system = qsa.SpatialOrbitalSystem(2 * n, bs)
    host = (np.array(bs.h), np.array(bs.s), np.array(bs.u), float(bs.nuclear_repulsion_energy))
    system.change_module(qsa.hip)
    return system, host


def state_bounds(ci, E1, r):
    """The oracle bounds of solved state ``r`` of ``ci`` with the one-spin operators ``E1 = (Ea, Eb)``."""
    c = H(ci.c)[r]
    T = plan(ci.m, ci.na, ci.nb, np.iscomplexobj(c))[2]
    return c, spref.spin_gamma_bound(E1[0], E1[1], c, c, T)


@pytest.mark.parametrize("form", list(FORMS))
def test_polarised_states_of_a_solver(form):
    """m = 6, three up and one down: spin density, <S^2>, the energy and the natural spin orbitals from the spin blocks."""
    from quantum_systems_amd import StringCI, hip

    cplx = FORMS[form]
    l, Na, Nb = 6, 3, 1
    system, (h, s, u, e_nuc) = random_spatial_system(l, 2, 6031, cplx)
    X = dref.loewdin(s)
    ci = StringCI(system, hip.asarray(X), n_up=Na, n_down=Nb)
    for method in (ci.one_body_density_spin, ci.spin_density, ci.two_body_density_spin, ci.spin_squared_from_densities,
                   ci.natural_spin_orbitals):
        with pytest.raises(RuntimeError, match="solve"):
            method(0)
    with pytest.raises(RuntimeError, match="solve"):
        ci.pair_density_matrix(np.ones(l), 0)
    E, _ = ci.solve(3, tol=1e-9)
    assert ci.converged
    E, m = H(E), ci.m
    E1 = (one_spin(m, Na)[1], one_spin(m, Nb)[1])
    ht = X.conj().T @ h @ X
    ut = np.einsum("pa,qb,pqrs,rc,sd->abcd", X.conj(), X.conj(), u, X, X, optimize=True)
    for r in range(3):
        c, (B, rB) = state_bounds(ci, E1, r)
        tag = f"{form} root {r}"
        rho_a, rho_b = (H(x) for x in ci.one_body_density_spin(r))
        sd = H(ci.spin_density(r))
        assert np.array_equal(sd, rho_a - rho_b)
        # trace of the spin density: N_a - N_b = 2 times <c|c>, the norm of a solved state being 1 to a few ulp
        norm = float(np.vdot(c, c).real)
        trace_bound = float(np.trace(rB[0]) + np.trace(rB[1])) + ref.gamma(2 * m) * (Na + Nb)      # and the host's own sum
        assert ratio_of(abs(np.trace(sd) - (Na - Nb) * norm), np.float64(trace_bound), f"{tag}: trace of the spin density") <= 1.0
        assert abs(np.trace(sd)) > 1e3 * trace_bound
        # <S^2> off Gamma^ab against <c|S^2 c>: m^2 elements of Gamma^ab, the elementwise bound of S^2 c weighted by |c|, and
        # the device's dot product over dim terms
        s2d, s2 = ci.spin_squared_from_densities(r), ci.spin_squared(r)
        Sc = H(ci.apply_spin_squared(ci._c[r]))
        bound = float(np.einsum("qppq->", B["ab"]) + np.sum(np.abs(c) * sref.spin_bound(E1[0], E1[1], Na, Nb, c[None])[0]))
        bound += ref.gamma(ci.dim + m * m + 2) * (float(np.sum(np.abs(c) * np.abs(Sc))) + abs(s2d) + 2 * abs(sref.spin_s0(Na, Nb))) * (S2 if cplx else 1.0)
        print(f"{tag}: <S^2> = {s2:.12f}, from Gamma^ab {s2d:.12f}")
        assert isinstance(s2d, float) and ratio_of(abs(s2d - s2), np.float64(bound), f"{tag}: spin_squared_from_densities against spin_squared") <= 1.0
        assert s2 > 1e3 * bound                                                    # S >= 1 here: <S^2> >= 2
        # the energy from the spin blocks: the Davidson tolerance 1e-9 is the source of 1e-8 (second order in the residual
        # with a margin for near-degenerate roots), as for energy_from_densities
        Gaa, Gab, Gbb = (H(x) for x in ci.two_body_density_spin(r))
        e = np.sum(ref._wide(ht) * (rho_a + rho_b).T) + np.longdouble(0.5) * np.sum(ref._wide(ut) * (Gaa + Gbb + 2 * Gab))
        assert abs(float(e.real) + e_nuc - E[r]) <= 1e-8 * max(1.0, abs(E[r]))
        # natural spin orbitals: an eigenvalue moves by at most the 2-norm of the error of rho^s, below the sum of its element
        # bounds; eigh itself is backward stable, p(m) eps |rho^s|_2 with p(m) = m^2 and |rho^s|_2 <= 1
        na_, Ca, nb_, Cb = (H(x) for x in ci.natural_spin_orbitals(r))
        for n_s, C_s, N_s, rb in ((na_, Ca, Na, rB[0]), (nb_, Cb, Nb, rB[1])):
            slack = float(rb.sum()) + m * m * ref.EPS
            assert n_s.shape == (m,) and C_s.shape == (l, m) and np.all(np.diff(n_s) <= 0)
            assert n_s.min() >= -slack and n_s.max() <= 1.0 + slack
            assert abs(n_s.sum() - N_s * norm) <= m * slack
    with pytest.raises(ValueError, match="spins"):
        ci.pair_density_matrix(np.ones(m), 0, spins="up")
    with pytest.raises(ValueError, match="phi0"):
        ci.pair_density_matrix(np.ones(m + 1), 0)


@pytest.mark.parametrize("parity", [1, -1])
def test_states_of_definite_spin_parity_have_no_spin_density(parity):
    from quantum_systems_amd import StringCI, hip

    l, n = 6, 2
    system, (h, s, u, e_nuc) = random_spatial_system(l, n, 6022, False)
    ci = StringCI(system, hip.asarray(dref.loewdin(s)), spin_parity=parity)
    ci.solve(2, tol=1e-9)
    assert ci.converged
    Ea = one_spin(ci.m, n)[1]
    for r in range(2):
        c, (B, rB) = state_bounds(ci, (Ea, Ea), r)
        assert np.array_equal(c, parity * c.T)
        sd = H(ci.spin_density(r))
        rho_a, _ = ci.one_body_density_spin(r)
        assert ratio_of(np.abs(sd), rB[0] + rB[1], f"parity {parity:+d} root {r}: rho^a - rho^b") <= 1.0
        assert float(np.abs(H(rho_a)).max()) > 1e3 * float((rB[0] + rB[1]).max())


@pytest.mark.parametrize("form", list(FORMS))
def test_pair_density_matrix(form):
    """Against an einsum of the downloaded blocks -- m^2 products of three factors per element, gamma_(m^2+2) times the
    sum of their moduli, 2 sqrt 2 per complex product (two of them) -- and the sum rule over the unit vectors,
    sum_q M(e_q) = (N_t - delta_st) rho^s, within the sum of the elements' bounds."""
    from quantum_systems_amd import StringCI, hip

    cplx = FORMS[form]
    l, Na, Nb = 6, 3, 1
    system, (h, s, u, e_nuc) = random_spatial_system(l, 2, 6031, cplx)
    ci = StringCI(system, hip.asarray(dref.loewdin(s)), n_up=Na, n_down=Nb)
    ci.solve(1, tol=1e-9)
    m = ci.m
    E1 = (one_spin(m, Na)[1], one_spin(m, Nb)[1])
    c, (B, rB) = state_bounds(ci, E1, 0)
    Gaa, Gab, Gbb = (H(x) for x in ci.two_body_density_spin(0))
    rho = dict(zip("ab", (H(x) for x in ci.one_body_density_spin(0))))
    blocks = {"aa": Gaa, "ab": Gab, "ba": Gab.transpose(1, 0, 3, 2), "bb": Gbb}
    blocks["sum"] = Gaa + Gbb + Gab + blocks["ba"]
    bounds = {"aa": B["aa"], "ab": B["ab"], "ba": B["ab"].transpose(1, 0, 3, 2), "bb": B["bb"]}
    rng = np.random.default_rng(66)
    phi = rng.standard_normal(m) + (1j * rng.standard_normal(m) if cplx else 0.0)
    cx = S2 * S2 if cplx else 1.0
    for spins, G in blocks.items():
        M = H(ci.pair_density_matrix(phi, 0, spins=spins))
        want = np.einsum("pqrs,q,s->rp", ref._wide(G), ref._wide(phi).conj(), ref._wide(phi))
        Gabs = sum(np.abs(blocks[st]) for st in ("aa", "ab", "ba", "bb")) if spins == "sum" else np.abs(G)
        moduli = np.einsum("pqrs,q,s->rp", Gabs, np.abs(phi), np.abs(phi))
        # "sum" adds four blocks on the device before the contraction: three more roundings of each element
        eb = ref.gamma(m * m + 2 + (3 if spins == "sum" else 0)) * moduli * cx
        assert M.shape == (m, m) and ratio_of(np.abs(M - want), eb, f"{form} pair_density_matrix {spins} against einsum") <= 1.0
        if spins == "bb" and Nb < 2:
            assert not M.any()                                                    # no pair of down particles: exact zeros
        else:
            assert float(np.abs(M).max()) > 1e3 * float(eb.max())                 # the comparison sees the result
    count = {"a": Na, "b": Nb}
    eye = np.eye(m)
    for spins in ("aa", "ab", "ba", "bb"):
        s_, t_ = spins
        fac = count[t_] - (1 if s_ == t_ else 0)
        total = sum(H(ci.pair_density_matrix(eye[q], 0, spins=spins)) for q in range(m))
        # M(e_q)[r,p] = Gamma^st[p,q,r,q] exactly (one non-zero product); the host sum of m of them
        bound = np.einsum("pqrq->rp", bounds[spins]) + fac * rB["ab".index(s_)] + ref.gamma(m) * np.einsum("pqrq->rp", np.abs(blocks[spins]))
        assert ratio_of(np.abs(total - fac * rho[s_]), bound, f"{form} sum over unit vectors, {spins}") <= 1.0
