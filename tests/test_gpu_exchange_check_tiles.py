"""The check kernel (``kernels.two_body_exchange_symmetric``) on a 3 x 3 grid of tiles with a ragged edge, l = 70.

A workgroup compares the four elements of a tile of u[a,b] that each thread holds in registers (rows ``ty + 8 j``)
against the tile of u[b,a] turned in LDS.  One flipped mantissa bit must be found wherever it sits: in every tile pair
(ti, tj) of the grid, in each of the four row slots j, on either side of the pair (a, b) and on the diagonal a == b,
where u[a,a] must be a symmetric matrix.  The tensor is restored after every flip, so the last verdict is "symmetric"."""

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
L = 70


@pytest.mark.parametrize("dtype", [torch.float64, torch.complex128], ids=["f64", "c128"])
def test_one_flipped_bit_is_found_in_every_tile_and_row_slot(dtype):
    from quantum_systems_amd import kernels as K

    g = torch.Generator(device=DEV).manual_seed(70)
    u = torch.randn((L, L, L, L), dtype=torch.float64, device=DEV, generator=g)
    if dtype.is_complex:
        u = torch.complex(u, torch.randn((L, L, L, L), dtype=torch.float64, device=DEV, generator=g))
    u = (u + u.permute(1, 0, 3, 2)).contiguous()           # x + y is commutative in IEEE arithmetic: exactly symmetric
    assert K.two_body_exchange_symmetric(u) is True
    parts = [torch.view_as_real(u)[..., k] for k in (0, 1)] if dtype.is_complex else [u]
    checked = 0
    for a, b in [(1, 4), (4, 1), (2, 2), (L - 1, L - 1), (0, L - 1)]:
        for ti in range(3):
            for tj in range(3):
                for slot in range(4):                      # rows ty + 8 * slot of the tile, ty = 3
                    c = ti * 32 + 3 + 8 * slot
                    if c >= L:
                        c = L - 1 - slot                   # the ragged last tile has six rows
                    d = min(tj * 32 + 17, L - 1)
                    assert (a, c) != (b, d)                # (an element that pairs with itself cannot break the symmetry)
                    bits = parts[(ti + tj + slot) % len(parts)].view(torch.int64)
                    bits[a, b, c, d] ^= 1
                    assert K.two_body_exchange_symmetric(u) is False, (a, b, c, d)
                    bits[a, b, c, d] ^= 1
                    checked += 1
    assert checked == 180
    assert K.two_body_exchange_symmetric(u) is True
