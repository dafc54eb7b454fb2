"""``kernels.pair_contract_antisym`` (``qs_pair_contract_antisym``) on the GPU: parity on every element against the
long-double packed-triangle sum of tests/_ccd_ref.py under its any-order bound, the promises of include/qs_amd.h bit for
bit (only the quarter p < q, r < s is read; the mirror is the negation of the same value; a result knows neither its
batch nor the group size; a NaN stays in its row / its amplitude), the cross-check against ``kernels.pair_contract``,
the dispatch and the Python layer.

Shapes.  A workgroup takes 16 pair rows (p < q), a wave 4 of them; a wave walks the n = l (l - 1) / 2 packed positions
of a row in steps of 64, the T values are staged in chunks of 3 steps (192 positions) in two buffers.  So:
  l = 2    one pair row, one term                  l = 3    n = 3: one wave, not all of its 4 rows
  l = 4    n = 6: a second wave                    l = 5    n = 10: odd l, runs at odd 8-byte alignment
  l = 7    n = 21 > 16: a second workgroup         l = 9    n = 36: the cross-check's small size
  l = 11 | 12   n = 55 | 66: one | two steps       l = 16 | 17   n = 120 | 136: two | three steps
  l = 20 | 21   n = 190 | 210: one | two chunks    l = 23   n = 253, odd
  l = 28 | 29   n = 378 | 406: two | three chunks (the first buffer is reused)
  l = 33   n = 528: nine steps, 33 workgroups
K in {1, G, G + 1, 2 G + 3}: a lone amplitude, a full group, a group and a partial one on the smallest instantiation,
two groups and a partial one."""

import re

import numpy as np
import pytest
import torch

import _ccd_ref as cc
import _two_particle_ref as tp

pytestmark = pytest.mark.gpu

FORMS = {"fp64": (False, False), "complex128": (True, True), "mixed": (False, True)}
SIZES = [2, 3, 4, 5, 7, 9, 11, 12, 16, 17, 20, 21, 23, 28, 29, 33]
G = 8                                       # the shipped group size of both kernel forms
WORST = {}


def rand(rng, shape, cplx):
    x = rng.standard_normal(shape)
    return x + 1j * rng.standard_normal(shape) if cplx else x


def dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def antisym_u(rng, l, cplx):
    w = rand(rng, (l,) * 4, cplx)
    w = w - w.transpose(1, 0, 2, 3)
    return w - w.transpose(0, 1, 3, 2)


def antisym_T(rng, K, l, cplx):
    x = rand(rng, (K, l, l), cplx)
    return x - x.transpose(0, 2, 1)


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
        m = re.match(r"qs::pair_contract_antisym_kernel<(\d+), (\d+)>(?: x(\d+))?$", part)
        if m:
            mine.append((int(m.group(1)), int(m.group(2)), int(m.group(3) or 1)))
        else:
            other.append(part)
    return mine, other


@pytest.fixture(scope="module", autouse=True)
def parity_report():
    yield
    for form, (ratio, where) in WORST.items():
        print(f"pair_contract_antisym parity {form}: largest error / bound = {ratio:.3f} at l = {where}")


@pytest.mark.parametrize("l", SIZES)
@pytest.mark.parametrize("form", list(FORMS))
def test_parity_quarter_read_mirror_and_batches(form, l):
    from quantum_systems_amd import kernels

    cu, ct = FORMS[form]
    rng = np.random.default_rng(100 * l + len(form))
    K = 2 * G + 3
    u, T = antisym_u(rng, l, cu), antisym_T(rng, K, l, ct)
    ud, Td = dev(u), dev(T)
    S = kernels.pair_contract_antisym(ud, Td)
    assert S.shape == (K, l, l) and S.dtype == (torch.complex128 if ct else torch.float64)
    mine, other = launches(kernels.last_dispatch())
    cols = 2 * K if form == "mixed" else K
    assert not other and sum(c for _, _, c in mine) == -(-cols // G) and all(f == int(cu) for f, _, _ in mine)

    # parity on every element, the any-order bound
    err = np.abs(S.cpu().numpy() - cc.pair_contract_antisym(u, T, extended=True)).astype(np.float64)
    bound = cc.pair_bound(u, T)
    ratio = float((err[bound > 0] / bound[bound > 0]).max())
    print(f"{form} l={l}: largest error / bound = {ratio:.3f}")
    if ratio > WORST.get(form, (0.0, None))[0]:
        WORST[form] = (ratio, l)
    assert (err <= bound).all()

    # the mirror is the negation of the same value, the diagonal +0
    b = bits(S)
    sign = torch.tensor(-2 ** 63, dtype=torch.int64, device="cuda")
    r, s = torch.triu_indices(l, l, offset=1, device="cuda")
    assert torch.equal(b[:, s, r], b[:, r, s] ^ sign)
    d = torch.arange(l, device="cuda")
    assert (b[:, d, d] == 0).all()

    # every K of the list against its place in the large batch, a 2-D T, and out=
    for k in (1, G, G + 1):
        assert torch.equal(bits(kernels.pair_contract_antisym(ud, Td[:k])), b[:k]), k
    assert torch.equal(bits(kernels.pair_contract_antisym(ud, Td[K - 1])), b[K - 1])
    out = torch.empty_like(S)
    assert kernels.pair_contract_antisym(ud, Td, out=out) is out and torch.equal(bits(out), b)

    # only the quarter is read: NaN everywhere else in U and T and in the padding between the rows
    nan = float("nan")
    rr, ss = np.triu_indices(l, 1)
    keep_u = np.zeros((l, l), dtype=bool)
    keep_u[rr, ss] = True
    quarter = keep_u[:, :, None, None] & keep_u[None, None, :, :]
    up = np.where(quarter, u, nan)
    Tp = np.where(keep_u[None], T, nan)
    for ldu in (l * l, l * l + 3):
        got = kernels.pair_contract_antisym(padded(dev(up), ldu), dev(Tp))
        assert torch.equal(bits(got), b), ldu
        assert torch.equal(bits(kernels.pair_contract_antisym(padded(ud, ldu), Td[:G + 1])), b[:G + 1]), ldu


@pytest.mark.parametrize("l", [66, 130])
def test_parity_where_a_step_stays_inside_its_run(l):
    """Up to l = 65 every step of 64 positions leaves its run, so the lane cursor always wraps.  l = 66: the first run is
    65 long, its lane 0 steps from (0, 1) to (0, 65) without a wrap; l = 130: runs past 128, two such steps in a row.
    fp64, K = 3, a contiguous u (152 MB | 2.3 GB, drawn on the device).  The parity assertion of
    ``test_parity_quarter_read_mirror_and_batches`` on EVERY pair row p < q (only those rows come back to the host: the
    long-double sums of all 8385 rows at l = 130 take a few seconds); the mirror and the diagonal are checked bit for bit
    on every element."""
    from quantum_systems_amd import kernels

    K, n = 3, l * (l - 1) // 2
    gen = torch.Generator(device="cuda").manual_seed(l)
    w = torch.randn((l,) * 4, dtype=torch.float64, device="cuda", generator=gen)
    w = w - w.transpose(0, 1)
    ud = w - w.transpose(2, 3)
    del w
    T = antisym_T(np.random.default_rng(l), K, l, False)
    S = kernels.pair_contract_antisym(ud, dev(T))
    mine, other = launches(kernels.last_dispatch())
    assert not other and mine == [(0, 4, 1)]

    p, q = (torch.from_numpy(x).cuda() for x in cc.triangle(l))
    urows = ud[p, q].cpu().numpy()
    err = np.abs(S[:, p, q].cpu().numpy() - cc.packed_rows(urows, T, extended=True)).astype(np.float64)
    bound = cc.rows_bound(urows, T)
    print(f"fp64 l={l}: largest error / bound = {float((err[bound > 0] / bound[bound > 0]).max()):.3f} on {n} rows")
    assert (err <= bound).all()

    b = bits(S)
    sign = torch.tensor(-2 ** 63, dtype=torch.int64, device="cuda")
    r, s = torch.triu_indices(l, l, offset=1, device="cuda")
    assert torch.equal(b[:, s, r], b[:, r, s] ^ sign)
    d = torch.arange(l, device="cuda")
    assert (b[:, d, d] == 0).all()


@pytest.mark.parametrize("form", list(FORMS))
def test_a_result_knows_neither_its_batch_nor_the_group_size(form):
    from quantum_systems_amd import kernels

    cu, ct = FORMS[form]
    rng = np.random.default_rng(11)
    l, K = 12, 2 * G + 3
    ud, Td = dev(antisym_u(rng, l, cu)), dev(antisym_T(rng, K, l, ct))
    alone = [bits(kernels.pair_contract_antisym(ud, Td[k:k + 1])[0]) for k in range(K)]
    for order in (list(range(K))[::-1], rng.permutation(K).tolist(), [3, 0, 3], rng.permutation(K).tolist()[:G + 1]):
        S = bits(kernels.pair_contract_antisym(ud, Td[order].contiguous()))
        for pos, k in enumerate(order):
            assert torch.equal(S[pos], alone[k]), (order, pos)
    S = bits(kernels.pair_contract_antisym(ud, Td))
    for g in (1, 2, 4, 8):
        with kernels.tuning(pair_contract_g=g):
            assert torch.equal(bits(kernels.pair_contract_antisym(ud, Td)), S), g
            mine, _ = launches(kernels.last_dispatch())
            assert mine[0][1] == g
    assert torch.equal(bits(kernels.pair_contract_antisym(ud, Td)), S)              # repeatable


@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("l", [5, 12])
def test_a_nan_stays_where_it_is(form, l):
    from quantum_systems_amd import kernels

    cu, ct = FORMS[form]
    rng = np.random.default_rng(5)
    K = 3
    ud, Td = dev(antisym_u(rng, l, cu)), dev(antisym_T(rng, K, l, ct))
    want = kernels.pair_contract_antisym(ud, Td)
    nan = float("nan")
    # a read element of U: row (p, q), p < q, at its last packed position (l - 2, l - 1)
    p, q = 1, l - 2
    bad = ud.clone()
    bad[p, q, l - 2, l - 1] = nan
    got = kernels.pair_contract_antisym(bad, Td)
    hit = torch.zeros(l, l, dtype=torch.bool, device="cuda")
    hit[p, q] = hit[q, p] = True
    assert torch.isnan(got[:, hit].real).all()
    assert torch.equal(bits(got[:, ~hit]), bits(want[:, ~hit]))
    # an element the kernel does not read changes nothing
    bad = ud.clone()
    bad[q, p, 0, 1] = nan
    bad[p, q, 1, 0] = nan
    bad[p, q, 2, 2] = nan
    assert torch.equal(bits(kernels.pair_contract_antisym(bad, Td)), bits(want))
    # T[k] reaches S[k] only
    Tb = Td.clone()
    Tb[1, 0, 1] = nan
    got = kernels.pair_contract_antisym(ud, Tb)
    off = ~torch.eye(l, dtype=torch.bool, device="cuda")
    assert torch.isnan(got[1][off].real).all()
    assert torch.equal(bits(got[0]), bits(want[0])) and torch.equal(bits(got[2]), bits(want[2]))


@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("l", [9, 17])
def test_against_the_full_pair_contraction(form, l):
    """On a truly anti-symmetrised u and anti-symmetric amplitudes the full contraction is the same sum: the two
    agree within the sum of their two any-order bounds."""
    from quantum_systems_amd import kernels

    cu, ct = FORMS[form]
    rng = np.random.default_rng(l)
    u, T = antisym_u(rng, l, cu), antisym_T(rng, G + 1, l, ct)
    ud, Td = dev(u), dev(T)
    a = kernels.pair_contract_antisym(ud, Td).cpu().numpy()
    b = kernels.pair_contract(ud, Td).cpu().numpy()
    assert (np.abs(a - b) <= cc.pair_bound(u, T) + tp.error_bound(u, T)).all()


def test_python_layer_and_the_system_method():
    import quantum_systems_amd as qsa
    from quantum_systems_amd import hip, kernels
    from quantum_systems_amd.sharded_module import ShardedTensor4

    z = torch.zeros(4, 4, 4, 4, dtype=torch.float64, device="cuda")
    for bad in (torch.zeros(2, 5, 5, device="cuda", dtype=torch.float64), torch.zeros(0, 4, 4, device="cuda", dtype=torch.float64),
                torch.zeros(16, device="cuda", dtype=torch.float64)):
        with pytest.raises(ValueError):
            kernels.pair_contract_antisym(z, bad)
    with pytest.raises(ValueError):
        kernels.pair_contract_antisym(z[:2], torch.zeros(4, 4, device="cuda", dtype=torch.float64))
    with pytest.raises(ValueError):
        kernels.pair_contract_antisym(z, torch.zeros(2, 4, 4, device="cuda", dtype=torch.float64),
                                      out=torch.zeros(2, 4, 3, device="cuda", dtype=torch.float64))
    # a permuted u is made contiguous, not misread
    rng = np.random.default_rng(8)
    w, T = antisym_u(rng, 4, False), antisym_T(rng, 2, 4, True)
    got = kernels.pair_contract_antisym(dev(w.transpose(2, 3, 0, 1)).permute(2, 3, 0, 1), dev(T))
    np.testing.assert_allclose(got.cpu().numpy(), np.einsum("pqrs,krs->kpq", w, T), rtol=1e-12, atol=1e-12)

    np.random.seed(77)
    spatial = qsa.SpatialOrbitalSystem(2, qsa.RandomBasisSet(3, 2))
    spatial.change_module(hip)
    gos = spatial.construct_general_orbital_system(anti_symmetrize=True)
    u = torch.as_tensor(gos.u).cpu().numpy()
    T = antisym_T(rng, 3, 6, True)
    want = np.einsum("pqrs,krs->kpq", u, T)
    got = gos.contract_two_body_pairs(hip.asarray(T), antisymmetric=True)
    assert isinstance(got, qsa.DeviceArray)
    assert "pair_contract_antisym_kernel" in kernels.last_dispatch()
    np.testing.assert_allclose(torch.as_tensor(got).cpu().numpy(), want, rtol=1e-12, atol=1e-12)
    np.testing.assert_allclose(torch.as_tensor(gos.contract_two_body_pairs(hip.asarray(T))).cpu().numpy(), want,
                               rtol=1e-12, atol=1e-12)
    plain = spatial.construct_general_orbital_system(anti_symmetrize=False)
    with pytest.raises(ValueError, match="anti-symmetrised"):
        plain.contract_two_body_pairs(hip.asarray(T), antisymmetric=True)
    with pytest.raises(ValueError, match="anti-symmetrised"):
        gos.contract_two_body_pairs(hip.asarray(T), u=gos.u, antisymmetric=True)
    gos._basis_set.u = ShardedTensor4(torch.as_tensor(gos.u).as_subclass(torch.Tensor).contiguous(), 6, 0, 0, 1)
    with pytest.raises(NotImplementedError, match="sharded"):
        gos.contract_two_body_pairs(hip.asarray(T), antisymmetric=True)
