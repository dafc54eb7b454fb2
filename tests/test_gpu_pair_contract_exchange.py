"""``kernels.pair_contract_exchange`` (``qs_pair_contract_exchange``) on the GPU: parity on every element against the
long-double packed-triangle sum of tests/_rccd_ref.py under its any-order bound, the promises of include/qs_amd.h bit for
bit (only the half r <= s of U is read; a result knows neither its batch nor the group size; a symmetric T gives a
symmetric S and an anti-symmetric T an anti-symmetric one; a NaN stays in its row pair / its amplitude), the
cross-check against ``kernels.pair_contract``, the dispatch and the Python layer.

Shapes.  A workgroup takes 8 row pairs {(p,q), (q,p)}, p <= q, a wave 2 of them; a wave walks the n = l (l + 1) / 2
packed positions of a row in steps of 64, the T values are staged in chunks of 3 steps (192 positions; fp64 and mixed) or
2 steps (128 positions; complex128) in two buffers.  So:
  l = 1    one pair, one term                      l = 2    n = 3: two waves, the second with one pair
  l = 3    n = 6: three waves                      l = 4    n = 10 > 8: a second workgroup
  l = 5, 7   n = 15, 28: odd l, runs at odd 8-byte alignment
  l = 10 | 11   n = 55 | 66: one | two steps       l = 15 | 16   n = 120 | 136: two | three steps (complex: one | two chunks)
  l = 19 | 20   n = 190 | 210: one | two chunks (fp64)      l = 22   n = 253, odd (complex: two chunks, the second three positions short)
  l = 27 | 28   n = 378 | 406: two | three chunks (fp64), three | four (complex): the first buffer is reused
  l = 32   n = 528: nine steps, 66 workgroups
K in {1, G, G + 1, 2 G + 3}: a lone amplitude, a full group, a group and a partial one on the smallest instantiation,
two groups and a partial one."""

import re

import numpy as np
import pytest
import torch

import _rccd_ref as rc
import _two_particle_ref as tp

pytestmark = pytest.mark.gpu

FORMS = {"fp64": (False, False), "complex128": (True, True), "mixed": (False, True)}
SIZES = [1, 2, 3, 4, 5, 7, 10, 11, 15, 16, 19, 20, 22, 27, 28, 32]
G = 8                                       # the shipped group size of both kernel forms
WORST = {}


def rand(rng, shape, cplx):
    x = rng.standard_normal(shape)
    return x + 1j * rng.standard_normal(shape) if cplx else x


def dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def exchange_u(rng, l, cplx):
    """Random with U[p,q,r,s] = U[q,p,s,r] bit for bit and no other symmetry (not Hermitian, not r <-> s)."""
    w = rand(rng, (l,) * 4, cplx)
    return w + w.transpose(1, 0, 3, 2)


def padded(ud, ldu, fill=float("nan")):
    """The same tensor with its (p, q) rows ``ldu`` elements apart inside a buffer filled with ``fill``."""
    l = ud.shape[0]
    buf = torch.full((l * l * ldu,), fill, dtype=ud.dtype, device="cuda")
    rows = buf.view(l, l, ldu)
    rows[:, :, :l * l] = ud.reshape(l, l, l * l)
    return rows[:, :, :l * l].unflatten(2, (l, l))


def bits(x):
    return (torch.view_as_real(x) if x.is_complex() else x).contiguous().view(torch.int64)


def launches(entry):
    mine, other = [], []
    for part in filter(None, (p.strip() for p in entry.split(";"))):
        m = re.match(r"qs::pair_contract_exchange_kernel<(\d+), (\d+)>(?: x(\d+))?$", part)
        if m:
            mine.append((int(m.group(1)), int(m.group(2)), int(m.group(3) or 1)))
        else:
            other.append(part)
    return mine, other


@pytest.fixture(scope="module", autouse=True)
def parity_report():
    yield
    for form, (ratio, where) in WORST.items():
        print(f"pair_contract_exchange parity {form}: largest error / bound = {ratio:.3f} at l = {where}")


@pytest.mark.parametrize("l", SIZES)
@pytest.mark.parametrize("form", list(FORMS))
def test_parity_half_read_and_batches(form, l):
    from quantum_systems_amd import kernels

    cu, ct = FORMS[form]
    rng = np.random.default_rng(100 * l + len(form))
    K = 2 * G + 3
    u, T = exchange_u(rng, l, cu), rand(rng, (K, l, l), ct)
    assert np.array_equal(u, u.transpose(1, 0, 3, 2))
    ud, Td = dev(u), dev(T)
    S = kernels.pair_contract_exchange(ud, Td)
    assert S.shape == (K, l, l) and S.dtype == (torch.complex128 if ct else torch.float64)
    mine, other = launches(kernels.last_dispatch())
    cols = 2 * K if form == "mixed" else K
    assert not other and sum(c for _, _, c in mine) == -(-cols // G) and all(f == int(cu) for f, _, _ in mine)

    # parity on every element, the any-order bound
    err = np.abs(S.cpu().numpy() - rc.pair_contract_exchange(u, T, extended=True)).astype(np.float64)
    bound = rc.pair_bound(u, T)
    ratio = float((err[bound > 0] / bound[bound > 0]).max())
    print(f"{form} l={l}: largest error / bound = {ratio:.3f}")
    if ratio > WORST.get(form, (0.0, None))[0]:
        WORST[form] = (ratio, l)
    assert (err <= bound).all()

    # every K of the list against its place in the large batch, a 2-D T, and out=
    b = bits(S)
    for k in (1, G, G + 1):
        assert torch.equal(bits(kernels.pair_contract_exchange(ud, Td[:k])), b[:k]), k
    assert torch.equal(bits(kernels.pair_contract_exchange(ud, Td[K - 1])), b[K - 1])
    out = torch.empty_like(S)
    assert kernels.pair_contract_exchange(ud, Td, out=out) is out and torch.equal(bits(out), b)

    # only the half is read: NaN in every U[., ., r > s] and in the padding between the rows
    lower = np.tril(np.ones((l, l), dtype=bool), -1)
    up = np.where(lower[None, None], float("nan"), u)
    for ldu in (l * l, l * l + 3):
        got = kernels.pair_contract_exchange(padded(dev(up), ldu), Td)
        assert torch.equal(bits(got), b), ldu
        assert torch.equal(bits(kernels.pair_contract_exchange(padded(ud, ldu), Td[:G + 1])), b[:G + 1]), ldu


@pytest.mark.parametrize("l", [66, 130])
def test_parity_where_a_step_stays_inside_its_run(l):
    """Up to l = 64 every step of 64 positions leaves its run, so the lane cursor always wraps.  l = 66: the first run is
    66 long, its lanes 0 and 1 step without a wrap; l = 130: runs past 128, two such steps in a row.  fp64, K = 3, a
    contiguous u (152 MB | 2.3 GB, drawn on the device).  The parity assertion of ``test_parity_half_read_and_batches``
    on (p, q) and (q, p) of EVERY row pair p <= q, which is every element (the long-double sums of all 8515 row pairs
    at l = 130 take a few seconds)."""
    from quantum_systems_amd import kernels

    K, n = 3, l * (l + 1) // 2
    gen = torch.Generator(device="cuda").manual_seed(l)
    w = torch.randn((l,) * 4, dtype=torch.float64, device="cuda", generator=gen)
    ud = w + w.permute(1, 0, 3, 2)
    del w
    assert torch.equal(ud, ud.permute(1, 0, 3, 2))
    T = rand(np.random.default_rng(l), (K, l, l), False)
    S = kernels.pair_contract_exchange(ud, dev(T))
    mine, other = launches(kernels.last_dispatch())
    assert not other and mine == [(0, 4, 1)]

    p, q = (torch.from_numpy(x).cuda() for x in rc.triangle(l))
    arows, brows = ud[p, q].cpu().numpy(), ud[q, p].cpu().numpy()
    upper, lower = rc.packed_rows(arows, brows, T, extended=True)
    bound = rc.rows_bound(arows, brows, T)
    worst = 0.0
    for got, want in ((S[:, p, q], upper), (S[:, q, p], lower)):
        err = np.abs(got.cpu().numpy() - want).astype(np.float64)
        worst = max(worst, float((err[bound > 0] / bound[bound > 0]).max()))
        assert (err <= bound).all()
    print(f"fp64 l={l}: largest error / bound = {worst:.3f} on {n} row pairs")


@pytest.mark.parametrize("form", list(FORMS))
def test_a_result_knows_neither_its_batch_nor_the_group_size(form):
    from quantum_systems_amd import kernels

    cu, ct = FORMS[form]
    rng = np.random.default_rng(11)
    l, K = 11, 2 * G + 3
    ud, Td = dev(exchange_u(rng, l, cu)), dev(rand(rng, (K, l, l), ct))
    alone = [bits(kernels.pair_contract_exchange(ud, Td[k:k + 1])[0]) for k in range(K)]
    for order in (list(range(K))[::-1], rng.permutation(K).tolist(), [3, 0, 3], rng.permutation(K).tolist()[:G + 1]):
        S = bits(kernels.pair_contract_exchange(ud, Td[order].contiguous()))
        for pos, k in enumerate(order):
            assert torch.equal(S[pos], alone[k]), (order, pos)
    S = bits(kernels.pair_contract_exchange(ud, Td))
    for g in (1, 2, 4, 8):
        with kernels.tuning(pair_contract_g=g):
            assert torch.equal(bits(kernels.pair_contract_exchange(ud, Td)), S), g
            mine, _ = launches(kernels.last_dispatch())
            assert mine[0][1] == g
    assert torch.equal(bits(kernels.pair_contract_exchange(ud, Td)), S)              # repeatable


@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("l", [5, 16])
def test_symmetric_and_antisymmetric_amplitudes(form, l):
    """Promise 3: T[k] = T[k]^T bit for bit gives S[k,q,p] and S[k,p,q] the same bits, T[k] = -T[k]^T the same but for
    the sign bit."""
    from quantum_systems_amd import kernels

    cu, ct = FORMS[form]
    rng = np.random.default_rng(l)
    ud = dev(exchange_u(rng, l, cu))
    x = rand(rng, (G + 1, l, l), ct)
    r, s = torch.triu_indices(l, l, offset=1, device="cuda")
    b = bits(kernels.pair_contract_exchange(ud, dev(x + x.transpose(0, 2, 1))))
    assert torch.equal(b[:, s, r], b[:, r, s])
    b = bits(kernels.pair_contract_exchange(ud, dev(x - x.transpose(0, 2, 1))))
    sign = torch.tensor(-2 ** 63, dtype=torch.int64, device="cuda")
    assert torch.equal(b[:, s, r], b[:, r, s] ^ sign)


@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("l", [5, 11])
def test_a_nan_stays_where_it_is(form, l):
    from quantum_systems_amd import kernels

    cu, ct = FORMS[form]
    rng = np.random.default_rng(5)
    K = 3
    ud, Td = dev(exchange_u(rng, l, cu)), dev(rand(rng, (K, l, l), ct))
    want = kernels.pair_contract_exchange(ud, Td)
    nan = float("nan")
    # a read element of U: row (p, q) at its last packed position (l - 1, l - 1), then the mirror row (q, p) at (0, 1)
    p, q = 1, l - 2
    hit = torch.zeros(l, l, dtype=torch.bool, device="cuda")
    hit[p, q] = hit[q, p] = True
    for where in ((p, q, l - 1, l - 1), (q, p, 0, 1)):
        bad = ud.clone()
        bad[where] = nan
        got = kernels.pair_contract_exchange(bad, Td)
        assert torch.isnan(got[:, hit].real).all()
        assert torch.equal(bits(got[:, ~hit]), bits(want[:, ~hit]))
    # a diagonal row reaches its own element only
    bad = ud.clone()
    bad[2, 2, 1, 3] = nan
    got = kernels.pair_contract_exchange(bad, Td)
    hit = torch.zeros(l, l, dtype=torch.bool, device="cuda")
    hit[2, 2] = True
    assert torch.isnan(got[:, hit].real).all() and torch.equal(bits(got[:, ~hit]), bits(want[:, ~hit]))
    # an element the kernel does not read changes nothing
    bad = ud.clone()
    bad[q, p, 1, 0] = nan
    bad[p, q, l - 1, 0] = nan
    bad[2, 2, 3, 1] = nan
    assert torch.equal(bits(kernels.pair_contract_exchange(bad, Td)), bits(want))
    # T[k] reaches S[k] only, wherever it sits (all of T is read)
    for where in ((1, 0, 1), (1, l - 1, 0), (1, 2, 2)):
        Tb = Td.clone()
        Tb[where] = nan
        got = kernels.pair_contract_exchange(ud, Tb)
        assert torch.isnan(got[1].real).all()
        assert torch.equal(bits(got[0]), bits(want[0])) and torch.equal(bits(got[2]), bits(want[2]))


@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("l", [9, 16])
def test_against_the_full_pair_contraction(form, l):
    """On a u with the symmetry the full contraction is the same sum: the two agree within the sum of their two
    any-order bounds."""
    from quantum_systems_amd import kernels

    cu, ct = FORMS[form]
    rng = np.random.default_rng(l)
    u, T = exchange_u(rng, l, cu), rand(rng, (G + 1, l, l), ct)
    ud, Td = dev(u), dev(T)
    a = kernels.pair_contract_exchange(ud, Td).cpu().numpy()
    b = kernels.pair_contract(ud, Td).cpu().numpy()
    assert (np.abs(a - b) <= rc.pair_bound(u, T) + tp.error_bound(u, T)).all()


def test_python_layer_and_the_system_method():
    import quantum_systems_amd as qsa
    from quantum_systems_amd import hip, kernels
    from quantum_systems_amd.sharded_module import ShardedTensor4

    z = torch.zeros(4, 4, 4, 4, dtype=torch.float64, device="cuda")
    for bad in (torch.zeros(2, 5, 5, device="cuda", dtype=torch.float64), torch.zeros(0, 4, 4, device="cuda", dtype=torch.float64),
                torch.zeros(16, device="cuda", dtype=torch.float64)):
        with pytest.raises(ValueError):
            kernels.pair_contract_exchange(z, bad)
    with pytest.raises(ValueError):
        kernels.pair_contract_exchange(z[:2], torch.zeros(4, 4, device="cuda", dtype=torch.float64))
    with pytest.raises(ValueError):
        kernels.pair_contract_exchange(z, torch.zeros(2, 4, 4, device="cuda", dtype=torch.float64),
                                       out=torch.zeros(2, 4, 3, device="cuda", dtype=torch.float64))
    # a permuted u is made contiguous, not misread
    rng = np.random.default_rng(8)
    w, T = exchange_u(rng, 4, False), rand(rng, (2, 4, 4), True)
    got = kernels.pair_contract_exchange(dev(w.transpose(2, 3, 0, 1)).permute(2, 3, 0, 1), dev(T))
    np.testing.assert_allclose(got.cpu().numpy(), np.einsum("pqrs,krs->kpq", w, T), rtol=1e-12, atol=1e-12)

    np.random.seed(77)
    spatial = qsa.SpatialOrbitalSystem(2, qsa.RandomBasisSet(5, 2))
    spatial.change_module(hip)
    u = torch.as_tensor(spatial.u).cpu().numpy()
    T = rand(rng, (3, 5, 5), True)
    want = np.einsum("pqrs,krs->kpq", u, T)
    got = spatial.contract_two_body_pairs(hip.asarray(T), exchange=True)
    assert isinstance(got, qsa.DeviceArray)
    assert "pair_contract_exchange_kernel" in kernels.last_dispatch()
    np.testing.assert_allclose(torch.as_tensor(got).cpu().numpy(), want, rtol=1e-12, atol=1e-12)
    got = spatial.contract_two_body_pairs(hip.asarray(T), u=spatial.u, exchange=True)      # a u of the caller's
    np.testing.assert_allclose(torch.as_tensor(got).cpu().numpy(), want, rtol=1e-12, atol=1e-12)
    np.testing.assert_allclose(torch.as_tensor(spatial.contract_two_body_pairs(hip.asarray(T))).cpu().numpy(), want,
                               rtol=1e-12, atol=1e-12)
    assert "pair_contract_exchange_kernel" not in kernels.last_dispatch()
    with pytest.raises(ValueError, match="one of them"):
        spatial.contract_two_body_pairs(hip.asarray(T), antisymmetric=True, exchange=True)
    spatial._basis_set.u = ShardedTensor4(torch.as_tensor(spatial.u).as_subclass(torch.Tensor).contiguous(), 5, 0, 0, 1)
    with pytest.raises(NotImplementedError, match="sharded"):
        spatial.contract_two_body_pairs(hip.asarray(T), exchange=True)
