"""The host reference of the ladder kernel and of the removal / addition spectra (tests/_string_ci_ladder_ref.py) against
dense Jordan-Wigner algebra, and ``response.lanczos`` / ``response.SpectralFunction`` on host tensors against the dense spectra
of the neighbouring sectors.  No GPU.

The list helper ``ladder`` / ``apply`` is pinned against ``dense_ladder`` for every orbital, both spins and both directions, by
the anticommutators (``{a_p alpha, a_q beta} = 0`` is what fixes the ``(-1)^n_alpha`` of a beta ladder) and by
``a+_p a_q = E_pq`` of the one-body reference.  Spectra: the three cases of ``_string_ci_response_ref``; errors are relative to
``sum_j w_j |p_j|^q`` (moments) and to the sums of moduli of ``_string_ci_ladder_ref.response`` / ``green``; the tolerance
1e-12 is that of the one-body host test."""

import numpy as np
import pytest

import _string_ci_ladder_ref as lref
import _string_ci_ref as ref
import _string_ci_response_ref as rref

TOL = 1e-12
SHAPES = [(3, 1, 1), (4, 2, 2), (4, 2, 1), (4, 3, 1)]


def draw(shape, cplx, seed):
    rng = np.random.default_rng(seed)
    x = rng.standard_normal(shape)
    return x + 1j * rng.standard_normal(shape) if cplx else x


def sector(m, Na, Nb, spin, step):
    """(Na, Nb) after ``step`` particles of ``spin``, or None where it does not exist."""
    Nat, Nbt = (Na + step, Nb) if spin == 0 else (Na, Nb + step)
    return (Nat, Nbt) if 0 <= Nat <= m and 0 <= Nbt <= m else None


def maps(m, Na, Nb, spin, step):
    """``(M, (Nat, Nbt))`` of the ladder of ``spin`` out of the (Na, Nb) sector."""
    Nat, Nbt = sector(m, Na, Nb, spin, step)
    M = lref.ladder(ref.strings(m, Nat if spin == 0 else Nbt), ref.strings(m, Na if spin == 0 else Nb), m)
    return M, (Nat, Nbt)


def unit(m, p):
    e = np.zeros((1, m))
    e[0, p] = 1.0
    return e


@pytest.mark.parametrize("cplx", [False, True])
@pytest.mark.parametrize("m,Na,Nb", SHAPES)
def test_list_helper_is_the_dense_ladder(m, Na, Nb, cplx):
    na, nb = len(ref.strings(m, Na)), len(ref.strings(m, Nb))
    c = draw((2, na, nb), cplx, 10 * m + Na)
    seen = 0
    for spin in (0, 1):
        for step in (-1, 1):
            if sector(m, Na, Nb, spin, step) is None:
                continue
            M, (Nat, Nbt) = maps(m, Na, Nb, spin, step)
            T = lref.table(M)
            assert T.shape == (M.shape[1], m) and (np.abs(T) <= M.shape[2]).all()
            for p in range(m):
                dense = lref.dense_ladder(m, Na, Nb, p, spin) if step < 0 else lref.dense_ladder(m, Nat, Nbt, p, spin).T
                got = lref.apply(unit(m, p), spin, Na, M, c)
                assert got.shape[:2] == (1, 2) and got.shape[2] * got.shape[3] == dense.shape[0]
                want = c.reshape(2, -1) @ dense.T
                assert np.abs(got[0].reshape(2, -1) - want).max() == 0.0, (spin, step, p)
                seen += int(np.abs(want).max() > 0)
                b = lref.bound(unit(m, p), spin, M, c)
                assert b.shape == got.shape and (b >= 0).all() and b.max() < 1e-13
    assert seen >= 2 * m


@pytest.mark.parametrize("cplx", [False, True])
@pytest.mark.parametrize("m,Na,Nb", SHAPES)
def test_anticommutators_through_the_helper(m, Na, Nb, cplx):
    """``{a_p s, a+_q s'} = delta_pq delta_ss'`` and ``{a_p alpha, a_q beta} = 0`` on random vectors: signs only, so the sums
    are exact up to the rounding of one addition."""
    na, nb = len(ref.strings(m, Na)), len(ref.strings(m, Nb))
    c = draw((1, na, nb), cplx, 3 * m + Nb)

    def hop(vec, N, spin, step, p):
        """``(a_p or a+_p of spin) vec`` on the (N[0], N[1]) sector -> (new vector, new sector)."""
        M, Nt = maps(m, N[0], N[1], spin, step)
        return lref.apply(unit(m, p), spin, N[0], M, vec)[0], Nt

    N = (Na, Nb)
    tol = 4 * ref.EPS * np.abs(c).max()
    for s in (0, 1):                                                      # every sector one step away exists at SHAPES
        for t in (0, 1):
            for p in range(m):
                for q in range(m):
                    raised, Nu = hop(c, N, t, +1, q)
                    first, back = hop(raised, Nu, s, -1, p)               # a_p,s a+_q,t c
                    lowered, Nd = hop(c, N, s, -1, p)
                    second, again = hop(lowered, Nd, t, +1, q)            # a+_q,t a_p,s c
                    assert back == again and first.shape == second.shape
                    if s == t:
                        assert back == N and np.abs(first + second - (c if p == q else 0.0 * c)).max() <= tol, (s, p, q)
                    else:
                        assert np.abs(first + second).max() == 0.0, (s, t, p, q)
    # the two spins: through (Na - 1, Nb) and through (Na, Nb - 1) to (Na - 1, Nb - 1)
    seen = 0.0
    for p in range(m):
        for q in range(m):
            first, N1 = hop(c, N, 1, -1, q)
            ab, Nab = hop(first, N1, 0, -1, p)                            # a_p,alpha a_q,beta c
            first, N2 = hop(c, N, 0, -1, p)
            ba, Nba = hop(first, N2, 1, -1, q)                            # a_q,beta a_p,alpha c
            assert Nab == Nba == (Na - 1, Nb - 1) and np.abs(ab + ba).max() == 0.0, (p, q)
            seen = max(seen, float(np.abs(ab).max()))
    assert seen > 0.0


@pytest.mark.parametrize("cplx", [False, True])
@pytest.mark.parametrize("m,Na,Nb", SHAPES)
def test_creation_after_annihilation_is_the_one_body_operator(m, Na, Nb, cplx):
    """``a+_p (a_q c)`` through the N - 1 sector is ``one_body`` with ``A = e_p e_q^T`` on that spin and 0 on the other."""
    sa, sb = ref.strings(m, Na), ref.strings(m, Nb)
    Ea, Eb = ref.list_E(sa, m), ref.list_E(sb, m)
    c = draw((2, len(sa), len(sb)), cplx, 7 * m + Na + Nb)
    for spin in (0, 1):
        down, Nt = maps(m, Na, Nb, spin, -1)
        up, back = maps(m, Nt[0], Nt[1], spin, +1)
        assert back == (Na, Nb)
        for p in range(m):
            for q in range(m):
                A = np.zeros((1, m, m))
                A[0, p, q] = 1.0
                want = rref.one_body(A if spin == 0 else 0 * A, A if spin == 1 else 0 * A, Ea, Eb, c)
                got = lref.apply(unit(m, p), spin, Nt[0], up, lref.apply(unit(m, q), spin, Na, down, c)[0])
                assert np.abs(got - want).max() == 0.0, (spin, p, q)


@pytest.fixture(scope="module")
def response():
    import __graft_entry__ as entry

    entry.build()
    from quantum_systems_amd import response

    return response


def spectra(response, H_other, phi, E0, steps):
    import torch

    Ht = torch.from_numpy(np.array(H_other))
    start = torch.from_numpy(np.array(phi).astype(H_other.dtype if np.iscomplexobj(H_other) else phi.dtype))
    out = []
    for n, reorth in steps:
        alpha, beta, norm2 = response.lanczos(lambda V: V @ Ht.transpose(0, 1).to(V.dtype), start, n, reorthogonalize=reorth)
        assert abs(norm2 - np.vdot(phi, phi).real) <= 1e-14 * norm2
        out.append((n, response.SpectralFunction(alpha, beta, norm2, E0)))
    return out


@pytest.mark.parametrize("m,Na,Nb,cplx", rref.CASES)
def test_the_driver_on_host_tensors_gives_the_dense_removal_and_addition_spectra(response, m, Na, Nb, cplx):
    """``phi = a(v) c0`` and ``a+(v) c0`` from the list helper, ``response.lanczos`` on the dense ``H`` of the neighbouring
    sector as host tensors: moments up to 2 n - 1, the response on the kept frequencies (taken on the moduli of the poles:
    ``response`` is singular at ``+-p_j``), and the retarded G at eta = 0.05 against the dense double sum."""
    ht, ut, H, _, _, c0, _, _ = rref.case(m, Na, Nb, cplx)
    E0 = float(np.vdot(c0, H @ c0).real)
    na, nb = len(ref.strings(m, Na)), len(ref.strings(m, Nb))
    v = draw((m,), cplx, 77)
    for spin in (0, 1):
        final = {}
        for step, dense in ((-1, lref.dense_removal_spectrum), (+1, lref.dense_addition_spectrum)):
            om, w = dense(ht, ut, Na, Nb, v, spin, c0)
            M, (Nat, Nbt) = maps(m, Na, Nb, spin, step)
            phi = lref.apply(v[None], spin, Na, M, c0.reshape(1, na, nb))[0, 0].reshape(-1)
            phi = phi.astype(np.complex128 if np.iscomplexobj(phi) else np.float64)
            assert abs(w.sum() - np.vdot(phi, phi).real) <= 1e-13 * w.sum()
            Hn = ref.dense_hamiltonian(ht, ut, Nat, Nbt)
            dim = Hn.shape[0]
            runs = spectra(response, Hn, phi, E0, [(min(6, dim), False), (min(12, dim), False), (dim, True)])
            for n, S in runs:
                err = rref.worst_moment_error(om, w, S.poles, S.weights, range(2 * len(S.alpha)))
                print(f"({m},{Na},{Nb}) complex={cplx} spin={spin} step={step:+d} n={n}: worst moment error {err:.2e}")
                assert err <= TOL
            S = runs[-1][1]
            freq = rref.kept_frequencies(np.abs(om))
            want, scale = lref.response(om, w, freq)
            rerr = float((np.abs(S.response(freq) - want) / scale).max())
            print(f"({m},{Na},{Nb}) complex={cplx} spin={spin} step={step:+d}: response error {rerr:.2e} on {len(freq)} frequencies")
            assert len(freq) >= 10 and rerr <= TOL
            final[step] = ((om, w), (S.poles, S.weights))
        omega = np.linspace(min(final[1][0][0].min(), -final[-1][0][0].max()) - 1.0, max(final[1][0][0].max(), -final[-1][0][0].min()) + 1.0, 41)
        want, scale = lref.green(final[1][0], final[-1][0], omega, 0.05)
        got, _ = lref.green(final[1][1], final[-1][1], omega, 0.05)
        gerr = float((np.abs(got - want) / scale).max())
        print(f"({m},{Na},{Nb}) complex={cplx} spin={spin}: retarded G error {gerr:.2e}")
        assert gerr <= TOL and np.abs(want.imag).max() > 0 and (want.imag <= 0).all()
