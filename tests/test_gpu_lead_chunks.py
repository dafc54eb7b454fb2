"""The chunk loop of ``lead_contract_kernel`` (qs_lead_contract.hip) and the panel loop of the block transform's
mixed-form product route.

The kernel stages the rows of A in LDS, [a][R] with R = 4 / 8 / 16 / 32 rows, and in chunks of kc values of a when
k R (8 or 16 bytes) exceeds 64 KB: kc = 2048 / 1024 / 512 / 256 for a real A and half of that for a complex one.  The
second trip of that loop -- its extra barrier, the ring of eight rows of B that is carried across the chunk boundary,
and a launch with exactly 65536 bytes of dynamic LDS -- needs k > kc; every other test of the kernel stops at k = 55.
Here k = kc - 1, kc, kc + 1, kc + 9 and 2 kc + 3 (one, one, two, two and three chunks) for every (form, R), at n = 515
(odd, three workgroups), each asserting

1. |T - exact| <= gamma_(k+2) |A| |B| (times 2 sqrt 2 with complex products) on every element, exact = numpy.longdouble;
2. row i of the m-row call has the bits of the 1-row call on that row (R = 4, which chunks a quarter ... an eighth as
   often): the identical chains the C ABI promises;
3. the same bits from a column slice of a wider NaN-filled buffer and from a base offset by one element.

``transform_two_body_blocks`` with M0 above ``lead_rows_max`` takes the tiled products; a real u with complex
coefficients cuts the second index into panels of M1, and L = 10, M1 = 3 (panels 3, 3, 3, 1) and L = 11, M1 = 4 (4, 4,
3) are the first cases here whose last panel is narrower -- against tests/_blocks_ref.py under its bound.

The worst error / bound per form is printed and, when QS_LEAD_CHUNKS_OUT names a file, appended there
(profiles/r15_fast_walk.txt holds the figures measured on the MI355X)."""

import os

import numpy as np
import pytest
import torch

import _blocks_ref as ref

pytestmark = pytest.mark.gpu
FORMS = ["fp64", "complex128", "mixed"]
N = 515
LDS_BYTES = 64 * 1024
DEPTH = 8
WORST = {}


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def host(t):
    return t.cpu().numpy()


def rand(rng, form, which, *shape):
    x = rng.standard_normal(shape)
    cplx = form == "complex128" or (form == "mixed" and which == "C")
    return x + 1j * rng.standard_normal(shape) if cplx else x


def rows_instantiation(m):
    return 4 if m <= 4 else 8 if m <= 8 else 16 if m <= 16 else 32


def chunk_rows(form, R):
    """kc of lc_launch: the values of a whose [a][R] rows of A fill 64 KB, a multiple of the pipeline depth."""
    aw = 1 if form == "fp64" else 2
    return LDS_BYTES // (R * aw * 8) // DEPTH * DEPTH


def test_chunk_sizes_are_the_documented_ones():
    assert [chunk_rows("fp64", R) for R in (4, 8, 16, 32)] == [2048, 1024, 512, 256]
    assert [chunk_rows("mixed", R) for R in (4, 8, 16, 32)] == [1024, 512, 256, 128]
    assert chunk_rows("complex128", 32) * 32 * 16 == LDS_BYTES


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    lines = [f"lead chunks {key}: largest error / bound = {r:.4f}" for key, r in sorted(WORST.items())]
    print("\n" + "\n".join(lines))
    if os.environ.get("QS_LEAD_CHUNKS_OUT"):
        with open(os.environ["QS_LEAD_CHUNKS_OUT"], "a") as f:
            f.write("\n".join(lines) + "\n")


@pytest.mark.parametrize("m", [3, 8, 16, 32])
@pytest.mark.parametrize("form", FORMS)
def test_chunked_rows_of_a(form, m):
    from quantum_systems_amd import kernels

    R = rows_instantiation(m)
    fit = chunk_rows(form, R)
    rng = np.random.default_rng(100 * FORMS.index(form) + m)
    ld = np.longdouble if form == "fp64" else np.clongdouble
    dt = torch.float64 if form != "complex128" else torch.complex128
    kmax = 2 * fit + 3
    Ah, Bh = rand(rng, form, "C", m, kmax), rand(rng, form, "u", kmax, N)
    for k in (fit - 1, fit, fit + 1, fit + 9, kmax):
        A, B = dev(Ah[:, :k]), dev(Bh[:k])
        T = kernels.lead_contract(A, B)
        ran = kernels.last_dispatch()
        assert ran.split(" x")[0] == f"qs::lead_contract_kernel<{FORMS.index(form)}, {R}>", ran
        exact = Ah[:, :k].astype(ld) @ Bh[:k].astype(ld)
        bound = ref.gamma(k + 2) * (np.abs(Ah[:, :k]) @ np.abs(Bh[:k])) * (1.0 if form == "fp64" else 2.0 * np.sqrt(2.0))
        ratio = float((np.abs(host(T) - exact) / bound).max())
        print(f"lead chunks {form} R={R} k={k} ({-(-k // fit)} chunks): max error / bound = {ratio:.4f}  [{ran}]")
        key = f"{form} <{FORMS.index(form)}, {R}>"
        WORST[key] = max(WORST.get(key, 0.0), ratio)
        assert ratio <= 1.0, (form, m, k, ratio)
        # rows: the 1-row call (R = 4) on every row
        for i in range(m):
            assert torch.equal(kernels.lead_contract(A[i:i + 1], B), T[i:i + 1]), (form, m, k, i)
        assert f"lead_contract_kernel<{FORMS.index(form)}, 4>" in kernels.last_dispatch()
        # a column slice of a wider buffer whose surplus is NaN (odd n: the last 16-byte item of a real row straddles into it)
        wide = torch.full((k, N + 7), float("nan"), dtype=dt, device="cuda")
        wide[:, :N] = B
        assert torch.equal(kernels.lead_contract(A, wide[:, :N]), T), (form, m, k, "slice")
        # a base offset by one element
        flat = torch.empty(k * N + 1, dtype=dt, device="cuda")
        flat[1:] = B.reshape(-1)
        assert torch.equal(kernels.lead_contract(A, flat[1:].view(k, N)), T), (form, m, k, "offset")
        del wide, flat


@pytest.mark.parametrize("L,M", [(10, (9, 3, 4, 4)), (11, (9, 4, 5, 3))])
@pytest.mark.parametrize("form", FORMS)
def test_block_transform_with_a_narrower_last_panel(form, L, M):
    from quantum_systems_amd import kernels

    # default lead_rows_max (8) < M0 = 9: the tiled products; mixed form: panels of M1 second indices, L % M1 != 0
    rng = np.random.default_rng(1000 + L)
    u = rand(rng, form, "u", L, L, L, L)
    ops = (u, rand(rng, form, "C", M[0], L), rand(rng, form, "C", M[1], L), rand(rng, form, "C", L, M[2]),
           rand(rng, form, "C", L, M[3]))
    got = host(kernels.transform_two_body_blocks(*map(dev, ops)))
    ran = kernels.last_dispatch()
    assert "lead_contract_kernel" not in ran and "gemm" in ran, ran
    if form == "mixed":
        assert ran.count("lc_split_kernel") == 1 and ran.count("lc_interleave_kernel") == -(-L // M[1]), ran     # one per panel
    assert got.shape == M and got.dtype == (np.float64 if form == "fp64" else np.complex128)
    ratio = float((np.abs(got - ref.blocks(*ops, extended=True)) / ref.error_bound(*ops)).max())
    print(f"blocks panels {form} L={L} M={M}: max error / bound = {ratio:.4f}  [{ran}]")
    key = f"blocks {form}"
    WORST[key] = max(WORST.get(key, 0.0), ratio)
    assert ratio <= 1.0, (form, L, M, ratio)
