"""The exact fp64 forms of the VALU-free product kernel (qs_gemm_fast.hip: <false, 4, 4, true, false> and
<false, 2, 4, true, false>) stage their operands HBM -> LDS directly (LDS-DMA, XOR-swizzled A rows).  The MFMA order
along k is the one of the general kernel, so every product and the whole transform must come out BIT-identical to
the general kernel (gemm_fast = 0), not merely close.  Shapes: every product of the l = 128 transform at full size,
and those of l = 256 with the same extents along n and k (the tile walk and K = 256) on fewer rows / batches."""

import pytest
import torch

pytestmark = pytest.mark.gpu

F44 = "qs::gemm_fast_kernel<false, 4, 4, true, false>"
F24 = "qs::gemm_fast_kernel<false, 2, 4, true, false>"


@pytest.fixture(scope="module")
def K():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    from quantum_systems_amd import kernels

    return kernels


def _rand(seed, *shape):
    g = torch.Generator(device="cuda:0").manual_seed(seed)
    return torch.rand(shape, dtype=torch.float64, device="cuda:0", generator=g) - 0.5


def _product(K, A, B, m, n, k, lda, ldb, ldc, batch, sa, sb, sc, out=None, accumulate=False):
    if out is None:
        out = torch.empty(batch * m * n if batch > 1 else m * ldc, dtype=torch.float64, device="cuda:0")
    K.gemm_raw(torch.float64, A, B, out, m, n, k, lda, ldb, ldc, batch, sa, sb, sc, accumulate)
    return out


def _both_routes(K, kernel, A, B, *shape, accumulate_into=None):
    """The product on the fast kernel (route asserted) and on the general one; the accumulate form too."""
    with K.tuning(gemm_fast=1):
        fast = _product(K, A, B, *shape)
        assert K.last_dispatch().split(" x")[0] == kernel, K.last_dispatch()
        fast_acc = None
        if accumulate_into is not None:
            fast_acc = _product(K, A, B, *shape, out=accumulate_into.clone(), accumulate=True)
            assert K.last_dispatch().split(" x")[0] == kernel, K.last_dispatch()
    with K.tuning(gemm_fast=0):
        general = _product(K, A, B, *shape)
        assert "qs::gemm_kernel<" in K.last_dispatch(), K.last_dispatch()
        general_acc = None
        if accumulate_into is not None:
            general_acc = _product(K, A, B, *shape, out=accumulate_into.clone(), accumulate=True)
    torch.cuda.synchronize()
    return fast, general, fast_acc, general_acc


def _shapes(l, rows3, batch_c, batch_b, n_a):
    """(name, m, n, k, lda, ldb, ldc, batch, sa, sb, sc) of the transform's products at basis size l (L = M = l)."""
    return [
        ("d", rows3, l, l, l, l, l, 1, 0, 0, 0),                                   # u[(abc), d] C[d, s]
        ("c", l, l, l, l, l, l, batch_c, 0, l * l, l * l),                         # CT . T1[ab], shared A
        ("b", l, l * l, l, l, l * l, l * l, batch_b, 0, l * l * l, l * l * l),     # Ct . T2[a], shared A
        ("a", l, n_a, l, l, n_a, n_a, 1, 0, 0, 0),                                 # Ct . T3
    ]


@pytest.mark.parametrize("l,rows3,batch_c,batch_b,n_a", [(128, 128**3, 128**2, 128, 128**3),
                                                          (256, 256 * 256 * 8, 512, 4, 256 * 256 * 4)])
def test_exact_form_products_bit_identical_to_general_kernel(K, l, rows3, batch_c, batch_b, n_a):
    for step, (name, m, n, k, lda, ldb, ldc, batch, sa, sb, sc) in enumerate(_shapes(l, rows3, batch_c, batch_b, n_a)):
        a_elems = m * lda if sa == 0 else batch * sa
        b_elems = k * ldb if batch == 1 else batch * sb
        A = _rand(10 * l + step, a_elems)
        B = _rand(10 * l + step + 5, b_elems)
        c_elems = batch * sc if batch > 1 else m * ldc
        acc0 = _rand(10 * l + step + 7, c_elems) if name in ("d", "c") else None
        fast, general, fast_acc, general_acc = _both_routes(K, F44, A, B, m, n, k, lda, ldb, ldc, batch, sa, sb, sc,
                                                            accumulate_into=acc0)
        assert torch.isfinite(fast).all()
        assert torch.equal(fast, general), (l, name)
        if acc0 is not None:
            assert torch.equal(fast_acc, general_acc), (l, name, "accumulate")
            assert not torch.equal(fast_acc, acc0)
        del A, B, fast, general, fast_acc, general_acc, acc0
        torch.cuda.empty_cache()


@pytest.mark.parametrize("m,n,k,batch", [(64, 128, 16, 1), (192, 256, 128, 3), (320, 1024, 256, 2), (64, 128 * 64, 64, 5)])
def test_64_row_form_bit_identical_to_general_kernel(K, m, n, k, batch):
    A = _rand(m + k, m * k)
    B = _rand(n + batch, batch * k * n)
    acc0 = _rand(7, batch * m * n)
    fast, general, fast_acc, general_acc = _both_routes(K, F24, A, B, m, n, k, k, n, n, batch, 0, k * n, m * n,
                                                        accumulate_into=acc0)
    assert torch.equal(fast, general)
    assert torch.equal(fast_acc, general_acc)


def test_whole_transform_l128_bit_identical_to_general_kernel_chain(K):
    # the transform (four launches of the DMA-staged kernel) against the same four contractions on the general kernel
    l = 128
    u = _rand(128, l, l, l, l)
    g = torch.Generator(device="cuda:0").manual_seed(3)
    C, _ = torch.linalg.qr(torch.randn(l, l, dtype=torch.float64, device="cuda:0", generator=g))
    C = C.contiguous()
    CT = C.t().contiguous()
    with K.tuning(gemm_fast=1):
        out = K.transform_two_body(u, C, CT)
        assert K.last_dispatch() == F44 + " x4", K.last_dispatch()
    with K.tuning(gemm_fast=0):
        t1 = _product(K, u, C, l**3, l, l, l, l, l, 1, 0, 0, 0)
        assert "qs::gemm_kernel<" in K.last_dispatch()
        t2 = _product(K, CT, t1, l, l, l, l, l, l, l * l, 0, l * l, l * l)
        del t1
        t3 = _product(K, CT, t2, l, l * l, l, l, l * l, l * l, l, 0, l**3, l**3)
        del t2
        ref = _product(K, CT, t3, l, l**3, l, l, l**3, l**3, 1, 0, 0, 0)
        del t3
    torch.cuda.synchronize()
    assert torch.isfinite(out).all()
    assert torch.equal(out.reshape(-1), ref), (out.reshape(-1) - ref).abs().max().item()
