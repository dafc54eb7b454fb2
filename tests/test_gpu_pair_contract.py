"""``kernels.pair_contract`` (``qs_pair_contract``) on the GPU: parity on every element against the long-double
restatement of tests/_two_particle_ref.py under its any-order bound, the four promises of include/qs_amd.h with
``torch.equal``, the launch counts, and the Python layer.

Shapes: the smallest at which each mechanism can break.  A wave walks a row in steps of 64 16-byte items (128 real or
64 complex elements) and the T values are staged in chunks of 3 steps with two buffers, so besides the issue's list
(one element, odd Y with alternating row alignment, Y below / at / over a wave's and a workgroup's width, several
chunks) the L on either side of every step- and chunk-count boundary up to the third chunk are included:
real u 11 | 12 (one | two steps), 19 | 20 (one | two chunks), 27 | 28 (two | three chunks: the first buffer is reused);
complex u 8 | 9, 13 | 14, 19 | 20."""

import os
import re

import numpy as np
import pytest
import torch

import _two_particle_ref as tp

pytestmark = pytest.mark.gpu

FORMS = {"fp64": (False, False), "complex128": (True, True), "mixed": (False, True)}
SQUARE = [1, 2, 3, 5, 8, 9, 11, 12, 13, 14, 16, 19, 20, 23, 27, 28, 32]
SHAPES = [(L, L, L, L) for L in SQUARE] + [(3, 5, 7, 9)]
WORST = {}


def rand(rng, shape, cplx):
    x = rng.standard_normal(shape)
    return x + 1j * rng.standard_normal(shape) if cplx else x


def dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def launches(entry):
    """[(form, G, count)] of the streaming launches in one ``qs_last_dispatch`` entry, and the other kernel names."""
    mine, other = [], []
    for part in filter(None, (p.strip() for p in entry.split(";"))):
        m = re.match(r"qs::pair_contract_kernel<(\d+), (\d+)>(?: x(\d+))?$", part)
        if m:
            mine.append((int(m.group(1)), int(m.group(2)), int(m.group(3) or 1)))
        else:
            other.append(part)
    return mine, other


def last_dispatch():
    from quantum_systems_amd import _lib

    return _lib.load().qs_last_dispatch().decode()


_G = {}


def group_size(form):
    """G of the form, read from the dispatch log of a call with more vectors than any group holds."""
    from quantum_systems_amd import kernels

    if form not in _G:
        cu, ct = FORMS[form]
        u = torch.zeros(1, 1, 2, 2, dtype=torch.complex128 if cu else torch.float64, device="cuda")
        T = torch.zeros(64, 2, 2, dtype=torch.complex128 if ct else torch.float64, device="cuda")
        kernels.pair_contract(u, T)
        mine, _ = launches(last_dispatch())
        _G[form] = mine[0][1]
    return _G[form]


@pytest.fixture(scope="module", autouse=True)
def parity_report():
    yield
    path = os.environ.get("QS_PAIR_PARITY_OUT")
    for form, (ratio, where) in WORST.items():
        line = f"pair_contract parity {form}: largest error / bound = {ratio:.3f} at {where}"
        print(line)
        if path:
            with open(path, "a") as fh:
                fh.write(line + "\n")


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("form", list(FORMS))
def test_parity_batches_and_row_slices(form, shape):
    from quantum_systems_amd import kernels

    cu, ct = FORMS[form]
    G = group_size(form)
    rng = np.random.default_rng(sum(shape) + 7 * len(form))
    K = 2 * G + 1
    u, T = rand(rng, shape, cu), rand(rng, (K,) + shape[2:], ct)
    ud, Td = dev(u), dev(T)
    S = kernels.pair_contract(ud, Td)
    assert S.shape == (K,) + shape[:2] and S.dtype == (torch.complex128 if ct else torch.float64)
    err = np.abs(S.cpu().numpy() - tp.pair_contract(u, T, extended=True)).astype(np.float64)
    bound = tp.error_bound(u, T)
    ratio = float((err / bound).max())
    print(f"{form} {shape}: largest error / bound = {ratio:.3f}")
    if ratio > WORST.get(form, (0.0, None))[0]:
        WORST[form] = (ratio, shape)
    assert (err <= bound).all()
    # promise 1: every K of the issue's list, each result against its place in the large batch
    for k in sorted({1, max(1, G - 1), G, G + 1}):
        assert torch.equal(kernels.pair_contract(ud, Td[:k]), S[:k]), k
    assert torch.equal(kernels.pair_contract(ud, Td[K - 1]), S[K - 1])          # 2-D T -> (P, Q)
    # promise 2: leading rows of u
    for P in sorted({1, min(3, shape[0]), shape[0]}):
        assert torch.equal(kernels.pair_contract(ud[:P], Td), S[:, :P]), P
    lo = shape[0] // 2
    assert torch.equal(kernels.pair_contract(ud[lo:lo + 3], Td[:2]), S[:2, lo:lo + 3])


@pytest.mark.parametrize("form", list(FORMS))
def test_a_result_does_not_know_its_batch(form):
    from quantum_systems_amd import kernels

    cu, ct = FORMS[form]
    G = group_size(form)
    rng = np.random.default_rng(11)
    L, K = 12, 2 * G + 3
    ud, Td = dev(rand(rng, (L,) * 4, cu)), dev(rand(rng, (K, L, L), ct))
    alone = [kernels.pair_contract(ud, Td[k:k + 1])[0] for k in range(K)]
    for order in (list(range(K)), list(range(K))[::-1], rng.permutation(K).tolist(), [3, 0, 3], rng.permutation(K).tolist()[:G + 1]):
        S = kernels.pair_contract(ud, Td[order].contiguous())
        for pos, k in enumerate(order):
            assert torch.equal(S[pos], alone[k]), (order, pos)
    # ... nor the group size it ran under
    S = kernels.pair_contract(ud, Td)
    for g in (1, 2, 4, 8):
        with kernels.tuning(pair_contract_g=g):
            assert torch.equal(kernels.pair_contract(ud, Td), S), g
            mine, _ = launches(last_dispatch())
            assert mine[0][1] == g
    # promise 3, and out= handed back as it is
    out = torch.empty_like(S)
    assert kernels.pair_contract(ud, Td, out=out) is out and torch.equal(out, S)
    assert torch.equal(kernels.pair_contract(ud, Td), S)


@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("shape", [(5, 5, 5, 5), (4, 3, 11, 13), (6, 6, 6, 6)], ids=str)
def test_slab_position_leading_dimension_and_containment(form, shape):
    """Rows at an odd element offset inside a larger buffer and at a leading dimension above Y (8- and 16-byte aligned
    row starts, odd and even Y), the buffer NaN everywhere else: the bytes of the straddling half-items and past the
    last row are NaN.  Then the NaN placements of promise 4."""
    from quantum_systems_amd import kernels

    cu, ct = FORMS[form]
    rng = np.random.default_rng(5)
    P, Q, R, S_ = shape
    X, Y, K = P * Q, R * S_, 3
    u, T = rand(rng, shape, cu), rand(rng, (K, R, S_), ct)
    ud, Td = dev(u), dev(T)
    want = kernels.pair_contract(ud, Td)
    nan = float("nan")
    for lead, ldu in [(1, Y), (3, Y), (1, Y + 1), (2, Y + 3), (5, Y + 4)]:
        buf = torch.full((lead + X * ldu + 7,), nan, dtype=ud.dtype, device="cuda")
        rows = buf[lead:lead + X * ldu].view(P, Q, ldu)
        rows[:, :, :Y] = ud.reshape(P, Q, Y)
        slab = rows[:, :, :Y].unflatten(2, (R, S_))
        assert slab.data_ptr() == buf.data_ptr() + lead * buf.element_size()
        got = kernels.pair_contract(slab, Td)
        assert torch.equal(got, want), (lead, ldu)
        assert torch.isnan(buf[:lead]).all() and torch.isnan(buf[lead + X * ldu:]).all()      # read in place, nothing written
    # a non-finite value in row x of U reaches S[:, x] only
    x = X // 2
    bad = ud.clone()
    bad.view(X, Y)[x, Y - 1] = nan
    got = kernels.pair_contract(bad, Td).view(K, X)
    keep = torch.arange(X, device="cuda") != x
    assert torch.isnan(got[:, x].real).all() and torch.equal(got[:, keep], want.view(K, X)[:, keep])
    bad.view(X, Y)[x, Y - 1] = float("inf")
    got = kernels.pair_contract(bad, Td).view(K, X)
    assert not torch.isfinite(got[:, x].real).any() and torch.equal(got[:, keep], want.view(K, X)[:, keep])
    # ... one in T[k] reaches S[k] only
    Tb = Td.clone()
    Tb[1, 0, 0] = nan
    got = kernels.pair_contract(ud, Tb)
    assert torch.isnan(got[1].real).all() and torch.equal(got[0], want[0]) and torch.equal(got[2], want[2])


@pytest.mark.parametrize("form", list(FORMS))
def test_launch_counts(form):
    from quantum_systems_amd import kernels

    cu, ct = FORMS[form]
    G = group_size(form)
    code = {"fp64": 0, "complex128": 1, "mixed": 2}[form]
    rng = np.random.default_rng(2)
    L = 9
    ud = dev(rand(rng, (L,) * 4, cu))
    for K in (1, G - 1, G, G + 1, 2 * G + 1, 5 * G):
        if K < 1:
            continue
        kernels.pair_contract(ud, dev(rand(rng, (K, L, L), ct)))
        mine, other = launches(last_dispatch())
        assert not other, other                                   # no gemm, no closing launch
        assert all(f == code for f, _, _ in mine)
        assert sum(c for _, _, c in mine) == -(-K // G), (K, mine)
        want = {G: K // G} if K >= G else {}
        if K % G:                                                 # the partial group: the smallest instantiation that holds it
            small = 1
            while small < K % G:
                small *= 2
            want[small] = want.get(small, 0) + 1
        got = {}
        for _, g, c in mine:
            got[g] = got.get(g, 0) + c
        assert got == want, (K, mine)


def test_python_layer_errors_and_the_system_method():
    import quantum_systems_amd as qsa
    from quantum_systems_amd import hip, kernels

    u = torch.zeros(3, 4, 5, 6, dtype=torch.float64, device="cuda")
    for bad in (torch.zeros(2, 5, 5, device="cuda", dtype=torch.float64), torch.zeros(6, 5, device="cuda", dtype=torch.float64),
                torch.zeros(0, 5, 6, device="cuda", dtype=torch.float64), torch.zeros(30, device="cuda", dtype=torch.float64),
                torch.zeros(1, 2, 5, 6, device="cuda", dtype=torch.float64)):
        with pytest.raises(ValueError):
            kernels.pair_contract(u, bad)
    with pytest.raises(ValueError):
        kernels.pair_contract(u[0], torch.zeros(5, 6, device="cuda", dtype=torch.float64))
    with pytest.raises(ValueError):
        kernels.pair_contract(u, torch.zeros(2, 5, 6, device="cuda", dtype=torch.float64),
                              out=torch.zeros(2, 4, 3, device="cuda", dtype=torch.float64))
    with pytest.raises(RuntimeError, match="GPU only"):
        kernels.pair_contract(u.cpu(), torch.zeros(5, 6, dtype=torch.float64))
    with pytest.raises(TypeError):
        kernels.pair_contract(np.zeros((3, 4, 5, 6)), torch.zeros(5, 6, device="cuda", dtype=torch.float64))
    # a permuted u is made contiguous, not misread
    rng = np.random.default_rng(8)
    w, T = rand(rng, (4, 4, 4, 4), False), rand(rng, (2, 4, 4), True)
    got = kernels.pair_contract(dev(w).permute(1, 0, 3, 2), dev(T))
    np.testing.assert_allclose(got.cpu().numpy(), tp.pair_contract(w.transpose(1, 0, 3, 2), T), rtol=1e-12, atol=1e-12)

    np.random.seed(77)
    host = qsa.SpatialOrbitalSystem(2, qsa.RandomBasisSet(6, 2))
    T = rand(rng, (3, 6, 6), True)
    want = tp.pair_contract(np.asarray(host.u), T)
    got_np = host.contract_two_body_pairs(T)
    assert isinstance(got_np, np.ndarray)
    np.testing.assert_allclose(got_np, want, rtol=1e-12, atol=1e-12)
    np.testing.assert_allclose(host.contract_two_body_pairs(T[0]), want[0], rtol=1e-12, atol=1e-12)
    host.change_module(hip)
    got_dev = host.contract_two_body_pairs(hip.asarray(T))
    assert isinstance(got_dev, qsa.DeviceArray)
    np.testing.assert_array_equal(torch.as_tensor(got_dev).cpu().numpy(), got_np)
    from quantum_systems_amd.sharded_module import ShardedTensor4

    sharded_u = ShardedTensor4(torch.as_tensor(host.u).as_subclass(torch.Tensor).contiguous(), 6, 0, 0, 1)
    with pytest.raises(NotImplementedError, match="sharded"):
        host.contract_two_body_pairs(hip.asarray(T), u=sharded_u)
