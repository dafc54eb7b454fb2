"""Removal and addition spectra and the one-particle Green's function on the GPU: ``response.lanczos`` on
``kernels.string_ci_sigma`` of the neighbouring sector from ``kernels.string_ci_ladder``, and ``StringCI.neighbour`` /
``annihilate`` / ``create`` / ``removal_spectrum`` / ``addition_spectrum`` / ``green_function`` / ``dyson_orbitals`` on them.

The kernel-level runs go against the dense spectra of tests/_string_ci_ladder_ref.py on the three cases of
tests/_string_ci_response_ref.py, with the sums and scales of tests/test_string_ci_ladder_ref_host.py: moments relative to
``sum_j w_j |p_j|^q``, the response relative to ``sum_j w_j (1 / |p_j - omega| + 1 / |p_j + omega|)``.  The tolerance 1e-10 is
that of tests/test_gpu_string_ci_response.py: the host recurrence alone stays below 1e-13 on these inputs, and a wrong sign or
a wrong sector shows at 1e-2 or worse.  The tolerances of the ``StringCI`` level are those of the issue; where a solved state
enters, ``solve`` runs to a residual of 1e-12."""

import numpy as np
import pytest
import torch

import _det_ci_ref as dref
import _string_ci_ladder_ref as lref
import _string_ci_ref as ref
import _string_ci_response_ref as rref

pytestmark = pytest.mark.gpu
TOL = 1e-10


def H(x):
    return torch.as_tensor(x).cpu().numpy()


def dev(x):
    return torch.from_numpy(np.array(x)).cuda()


def draw(shape, cplx, seed):
    rng = np.random.default_rng(seed)
    x = rng.standard_normal(shape)
    return x + 1j * rng.standard_normal(shape) if cplx else x


@pytest.mark.parametrize("spin,step", [(0, -1), (0, 1), (1, -1), (1, 1)])
@pytest.mark.parametrize("m,Na,Nb,cplx", rref.CASES)
def test_kernel_level_driver_against_the_dense_spectra(m, Na, Nb, cplx, spin, step):
    from quantum_systems_amd import kernels, response

    ht, ut, Hd, _, _, c0, _, _ = rref.case(m, Na, Nb, cplx)
    E0 = float(np.vdot(c0, Hd @ c0).real)
    v = draw((m,), cplx, 77)
    om, w = (lref.dense_removal_spectrum if step < 0 else lref.dense_addition_spectrum)(ht, ut, Na, Nb, v, spin, c0)
    Nat, Nbt = (Na + step, Nb) if spin == 0 else (Na, Nb + step)
    sa, sb, sat, sbt = (dev(ref.strings(m, N)) for N in (Na, Nb, Nat, Nbt))
    na, nb, nat, nbt = len(sa), len(sb), len(sat), len(sbt)
    table = kernels.string_ci_ladder_table(sat if spin == 0 else sbt, sa if spin == 0 else sb, m)
    phi = kernels.string_ci_ladder(dev(v), table, spin, Na, dev(c0).reshape(na, nb))
    assert tuple(phi.shape) == (nat, nbt)
    if cplx:
        phi = phi.to(torch.complex128)
    k, W = ref.kh_operands(ht, ut)
    dk, dW = dev(k), dev(W)
    ta, tb = kernels.string_ci_table(sat, m, Nat), kernels.string_ci_table(sbt, m, Nbt)
    dim = nat * nbt

    def sigma(V):
        return kernels.string_ci_sigma(dk, dW, ta, tb, V.reshape(V.shape[0], nat, nbt)).reshape(V.shape[0], dim)

    tag = f"({m},{Na},{Nb}) complex={cplx} spin {spin} step {step:+d}"
    worst = 0.0
    for n, reorth in ((min(6, dim), False), (min(12, dim), False), (dim, True)):
        alpha, beta, norm2 = response.lanczos(sigma, phi, n, reorthogonalize=reorth)
        S = response.SpectralFunction(alpha, beta, norm2, E0)
        err = rref.worst_moment_error(om, w, S.poles, S.weights, range(2 * len(alpha)))
        print(f"{tag} n={n}: worst moment error / {TOL:.0e} = {err / TOL:.2e}")
        worst = max(worst, err)
    freq = rref.kept_frequencies(np.abs(om))
    want, scale = lref.response(om, w, freq)
    rerr = float((np.abs(S.response(freq) - want) / scale).max())
    print(f"{tag} n=dim={dim} reorthogonalised: response error / {TOL:.0e} = {rerr / TOL:.2e} on {len(freq)} frequencies")
    assert len(freq) >= 10 and abs(norm2 - w.sum()) <= 1e-12 * w.sum()
    assert worst <= TOL and rerr <= TOL


def random_spatial_system(l, n, seed, cplx, on_device=True):
    """A seeded RandomBasisSet made physical (s positive definite near 1, u with the symmetries of <pq|rs>) with 2 n
    electrons, as in tests/test_gpu_string_ci_response.py."""
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
    assert system.n == n
    overlap = np.array(bs.s)
    if on_device:
        system.change_module(qsa.hip)
    return system, overlap


SOLVE = dict(tol=1e-12, max_iter=300)


@pytest.mark.parametrize("module", ["hip", "numpy"])
@pytest.mark.parametrize("cplx", [False, True])
def test_string_ci_level(cplx, module):
    """Everything twice: on a system in the device module, whose results come back as device arrays, and on one in numpy,
    whose results come back as numpy arrays.  The vectors of ``annihilate`` / ``create`` are device tensors in both."""
    import gc

    import quantum_systems_amd as qsa
    from quantum_systems_amd import StringCI, hip, kernels, response

    l, n = 6, 2
    system, s = random_spatial_system(l, n, 7117, cplx, on_device=module == "hip")
    X = hip.asarray(dref.loewdin(s)) if module == "hip" else dref.loewdin(s)
    kind = qsa.DeviceArray if module == "hip" else np.ndarray
    ci = StringCI(system, X)
    v = draw((l,), cplx, 11)
    v = v / np.linalg.norm(v)

    # the neighbours: shared integrals, the unchanged spin's list and table carried over, built once
    ion, anion = ci.neighbour(d_up=-1), ci.neighbour(d_up=+1)
    assert ion._ut is ci._ut and ion._C is ci._C and ion._ht is ci._ht and ion._k is ci._k and ion._W is ci._W
    assert ion._tb is ci._tb and ion._sb is ci._sb and ion._ta is not ci._ta and ion.spin_parity is None
    assert (ion.n_up, ion.n_down, ion.na, ion.nb) == (1, 2, 6, 15) and (anion.n_up, anion.n_down, anion.na, anion.nb) == (3, 2, 20, 15)
    assert ci.neighbour(d_up=-1) is ion and ci.neighbour(-1, 0) is ion and ci.neighbour(d_up=-1, strings=ion.strings_up) is not ion
    down = ci.neighbour(d_down=-1)
    assert down._ta is ci._ta and (down.n_up, down.n_down, down.na, down.nb) == (2, 1, 15, 6)
    E_ion, _ = ion.solve(n_roots=3, **SOLVE)
    fresh = StringCI(system, X, n_up=1, n_down=2)
    E_fresh, _ = fresh.solve(n_roots=3, **SOLVE)
    assert ion.converged and fresh.converged and isinstance(E_ion, kind)
    assert np.abs(H(E_ion) - H(E_fresh)).max() <= 1e-10

    # annihilate and create are the kernel-level calls on the tables between the lists
    c = dev(draw((2, ci.na, ci.nb), cplx, 12))
    for spin, s_, step, other, src in (("up", 0, -1, ion, ci._sa), ("up", 0, +1, anion, ci._sa), ("down", 1, -1, down, ci._sb)):
        table = kernels.string_ci_ladder_table(other._sa if s_ == 0 else other._sb, src, l)
        op = ci.annihilate if step < 0 else ci.create
        for v_, c_ in ((v, c), (v, c[0]), (np.stack([v, 2 * v, v.conj()]), c)):
            got = op(v_, c_, spin=spin)
            want = kernels.string_ci_ladder(dev(v_), table, s_, ci.n_up, c_)
            assert isinstance(got, torch.Tensor) and got.is_cuda and torch.equal(got, want)
            assert tuple(got.shape[-2:]) == (other.na, other.nb)
        assert torch.equal(op(hip.asarray(v), c, spin=spin, other=other), op(v, c, spin=spin))
    assert len(ci._ladders) == 3                                                    # one table per (other, spin, direction)
    # the cache holds weak references: a sector built for one call is not kept alive by it
    passing = ci.neighbour(d_up=-1, strings=ion.strings_up)
    assert torch.equal(ci.annihilate(v, c, other=passing), ci.annihilate(v, c)) and len(ci._ladders) == 4
    del passing
    gc.collect()
    assert sum(kept() is not None for kept, _ in ci._ladders.values()) == 3

    # the lowest removal pole is the first ionisation energy of the two solves
    E, _ = ci.solve(n_roots=1, **SOLVE)
    assert ci.converged
    S = ci.removal_spectrum(v, n_steps=ion.dim, reorthogonalize=True)
    assert isinstance(S, response.SpectralFunction)
    first = float(H(E_ion)[0]) - float(H(E)[0])
    heavy = S.poles[S.weights > 1e-12 * S.weights.sum()]
    print(f"complex={cplx}: lowest removal pole {heavy[0]:.12f}, E0(N-1) - E0(N) = {first:.12f}")
    assert abs(heavy[0] - first) <= 1e-8

    # sum rules: moment(0) of the removal spectrum is v^+ rho v, of the addition spectrum v^+ (1 - rho) v
    nst = 16
    rho_a, rho_b = (H(x) for x in ci.one_body_density_spin(0))                      # rho[q, p] = <a+_p a_q>
    for spin, rho in (("up", rho_a), ("down", rho_b)):
        Sm, Sp = ci.removal_spectrum(v, spin=spin, n_steps=nst), ci.addition_spectrum(v, spin=spin, n_steps=nst)
        hole = float(np.einsum("p,q,qp->", v.conj(), v, rho).real)                  # |a(v) c|^2 = sum conj(v_p) v_q <a+_p a_q>
        part = float(np.einsum("p,q,pq->", v.conj(), v, np.eye(l) - rho).real)      # |a+(v) c|^2 = sum conj(v_p) v_q <a_p a+_q>
        print(f"complex={cplx} {spin}: moment(0) removal {Sm.moment(0):.15f} against {hole:.15f}, addition {Sp.moment(0):.15f} against {part:.15f}")
        assert abs(Sm.moment(0) - hole) <= 1e-12 and abs(Sp.moment(0) - part) <= 1e-12

    # the Green's function is the double sum over the two spectra
    Sm, Sp = ci.removal_spectrum(v, n_steps=nst), ci.addition_spectrum(v, n_steps=nst)
    omega = np.linspace(-3.0, 3.0, 25)
    G = ci.green_function(omega, v, eta=0.05, n_steps=nst)
    want, scale = lref.green((Sp.poles, Sp.weights), (Sm.poles, Sm.weights), omega, 0.05)
    assert isinstance(G, kind) and tuple(G.shape) == (25,) and H(G).dtype == np.complex128
    assert (np.abs(H(G) - want) / scale).max() <= 1e-12 and (H(G).imag < 0).all()
    one = ci.green_function(0.3, v, eta=0.05, n_steps=nst)
    assert tuple(one.shape) == () and abs(complex(H(one)) - lref.green((Sp.poles, Sp.weights), (Sm.poles, Sm.weights), [0.3], 0.05)[0][0]) <= 1e-12

    # state= : the same run from a given vector, normalised inside, its energy from one sigma
    St = ci.removal_spectrum(v, n_steps=nst, state=3.0 * ci._c[0])
    assert abs(St.E_state - Sm.E_state) <= 1e-10 and abs(St.norm2 - Sm.norm2) <= 1e-12
    assert rref.worst_moment_error(Sm.poles, Sm.weights, St.poles, St.weights, range(2 * nst)) <= TOL
    unsolved = StringCI(system, X)
    Su = unsolved.addition_spectrum(v, n_steps=nst, state=ci._c[0])
    assert unsolved._c is None and rref.worst_moment_error(Sp.poles, Sp.weights, Su.poles, Su.weights, range(2 * nst)) <= TOL
    # a vector that the operator annihilates: the empty spectrum
    lone = StringCI(system, X, n_up=1, n_down=n)
    only = torch.zeros(lone.na, lone.nb, dtype=torch.float64, device="cuda")
    only[0] = 1.0                                                                   # the up particle in orbital 0: a_1 gives 0
    Se = lone.removal_spectrum(np.eye(l)[1], n_steps=4, state=only)
    assert Se.poles.shape == (0,) and Se.moment(0) == 0.0

    # Dyson orbitals against ALL states of the smaller sector: the strengths add up to the occupations
    every = ci.neighbour(d_up=-1, strings=ion.strings_up)
    every.solve(n_roots=every.dim, **SOLVE)
    g, orbitals = ci.dyson_orbitals(every)
    assert isinstance(g, kind) and isinstance(orbitals, kind) and tuple(g.shape) == (every.dim, l) and tuple(orbitals.shape) == (l, every.dim)
    g = H(g)
    strength = (np.abs(g) ** 2).sum(axis=0)
    print(f"complex={cplx}: sum_j |g[j,p]|^2 - rho[p,p]: {np.abs(strength - np.diag(rho_a).real).max():.2e}; first pole strength {np.sum(np.abs(g[0]) ** 2):.6f}")
    assert np.abs(strength - np.diag(rho_a).real).max() <= 1e-10
    assert np.abs(H(orbitals) - H(X) @ g.T).max() <= 1e-13 and 0.0 < np.sum(np.abs(g[0]) ** 2) <= 1.0 + 1e-12
    # the amplitudes are the weights of the spectrum: |sum_p v_p g[0, p]|^2 is the weight of the lowest pole
    assert abs(abs(np.sum(v * g[0])) ** 2 - S.weights[S.weights > 1e-12 * S.weights.sum()][0]) <= 1e-8
    # the other direction: from the ion, the neutral state is reached by a+_p
    every.solve(n_roots=1, **SOLVE)
    back, _ = every.dyson_orbitals(ci)
    assert tuple(back.shape) == (1, l)
    assert np.abs(np.abs(H(back)[0]) - np.abs(g[0])).max() <= 1e-8                  # <N|a+_p|N-1> = conj(<N-1|a_p|N>), up to the phases

    # refusals
    for bad in (dict(), dict(d_up=1, d_down=1), dict(d_up=2), dict(d_up=-1, d_down=1), dict(d_down=-2)):
        with pytest.raises(ValueError):
            ci.neighbour(**bad)
    full, none = StringCI(system, X, n_up=l, n_down=n), lone.neighbour(d_up=-1)
    assert (full.n_up, full.na) == (l, 1) and (none.n_up, none.na) == (0, 1)
    with pytest.raises(ValueError):
        full.neighbour(d_up=+1)                                                     # n_up = m + 1
    with pytest.raises(ValueError):
        none.neighbour(d_up=-1)                                                     # n_up = -1
    with pytest.raises(ValueError):
        ci.annihilate(v, c, other=anion)                                            # the wrong sector
    with pytest.raises(ValueError):
        ci.create(v, c, spin="down", other=anion)
    with pytest.raises(ValueError):
        ci.removal_spectrum(v, other=down)
    with pytest.raises(ValueError):
        ci.annihilate(v, c, spin="sideways")
    with pytest.raises(ValueError):
        ci.annihilate(v[:-1], c)
    with pytest.raises(ValueError):
        ci.removal_spectrum(np.stack([v, v]))                                       # one combination at a time
    with pytest.raises(ValueError):
        ci.dyson_orbitals(anion)                                                    # not solved
    with pytest.raises(ValueError):
        ci.dyson_orbitals(ion, spin="down")


@pytest.mark.parametrize("cplx", [False, True])
def test_on_numpy_arrays_the_results_come_back_as_numpy(cplx):
    from quantum_systems_amd import StringCI

    l, n, nst = 6, 2, 12
    system, s = random_spatial_system(l, n, 7117, cplx, on_device=False)
    X = dref.loewdin(s)
    ci = StringCI(system, X)
    E, _ = ci.solve(n_roots=1, **SOLVE)
    ion = ci.neighbour(d_down=-1)
    E_ion, _ = ion.solve(n_roots=2, **SOLVE)
    assert isinstance(E_ion, np.ndarray) and ion._ut is ci._ut
    v = np.eye(l)[0]
    G = ci.green_function(np.linspace(-1.0, 1.0, 5), v, spin="down", eta=0.1, n_steps=nst)
    assert isinstance(G, np.ndarray) and G.dtype == np.complex128 and G.shape == (5,)
    g, orbitals = ci.dyson_orbitals(ion, spin="down")
    assert isinstance(g, np.ndarray) and isinstance(orbitals, np.ndarray) and g.shape == (2, l) and orbitals.shape == (l, 2)
    S = ci.removal_spectrum(v, spin="down", n_steps=ion.dim, reorthogonalize=True)
    assert abs(S.poles[S.weights > 1e-12 * S.weights.sum()][0] - (E_ion[0] - E[0])) <= 1e-8
    assert isinstance(ci.annihilate(v, ci._c[0], spin="down"), torch.Tensor)


@pytest.mark.parametrize("module", ["hip", "numpy"])
def test_spin_parity_keeps_the_spectra_of_the_singlet_ground_state(module):
    from quantum_systems_amd import StringCI, hip

    l, n, nst = 6, 2, 10
    system, s = random_spatial_system(l, n, 7117, False, on_device=module == "hip")
    X = hip.asarray(dref.loewdin(s)) if module == "hip" else dref.loewdin(s)
    v = draw((l,), False, 13)
    plain, even = StringCI(system, X), StringCI(system, X, spin_parity=+1)
    Ep, _ = plain.solve(n_roots=1, **SOLVE)
    Ee, _ = even.solve(n_roots=1, **SOLVE)
    assert plain.converged and even.converged and abs(plain.spin_squared(0)) <= 1e-8 and abs(float(H(Ep)[0]) - float(H(Ee)[0])) <= 1e-10
    assert even.neighbour(d_up=-1).spin_parity is None
    for spectrum in ("removal_spectrum", "addition_spectrum"):
        Sp, Se = getattr(plain, spectrum)(v, n_steps=nst), getattr(even, spectrum)(v, n_steps=nst)
        dp = np.abs(Sp.poles - Se.poles).max() / np.abs(Sp.poles).max()
        dw = np.abs(Sp.weights - Se.weights).max() / Sp.weights.sum()
        print(f"{spectrum}, spin_parity=+1 against none: poles differ by {dp:.2e}, weights by {dw:.2e} (tolerance 1e-10)")
        assert dp <= 1e-10 and dw <= 1e-10
    # a singlet: the up and the down spectra agree
    up, dn = even.removal_spectrum(v, spin="up", n_steps=nst), even.removal_spectrum(v, spin="down", n_steps=nst)
    assert np.abs(up.poles - dn.poles).max() <= 1e-10 * np.abs(up.poles).max() and np.abs(up.weights - dn.weights).max() <= 1e-10 * up.weights.sum()
