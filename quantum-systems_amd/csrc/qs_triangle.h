// The upper triangle of an n x n grid as one flat list: pair t is the t-th (i, j >= i) in row-major order.  ONE remap for
// host and device: the check kernel's pair decode (qs_permute.hip), the triangular batch of the products (qs_gemm.hip,
// qs_gemm_fast.hip), the packed walks of the two triangle pair contractions (pair_unpack of qs_pair_walk.h: the strict
// triangle r < s of l is this one of n = l - 1 with its second index shifted by one) and qs_triangle_pair (qs_api.hip)
// all go through triangle_row.
//
// Everything is 32-bit: a grid of at most kTriangleMax rows has fewer than 2^31 pairs, and every product below stays under
// 2^32.  Inside a product kernel the remap runs once per tile on a wave-uniform index, so it has to be light on
// registers: a single-precision first guess and unsigned scalar arithmetic (a double-precision square root and 64-bit
// products cost the tiled kernels ten vector registers and a second workgroup per CU in two shapes).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <cmath>

namespace qs {

constexpr int64_t kTriangleMax = 65535;      // n (n + 1) / 2 < 2^31 and n^2 < 2^32

// First linear index of row a <= n.
__host__ __device__ __forceinline__ uint32_t triangle_row_start(uint32_t a, uint32_t n) { return a * n - ((a * (a - 1u)) >> 1); }

// Row a of the upper triangle of an n x n grid (rows of n, n - 1, ... entries) that holds linear index idx < n (n + 1) / 2,
// 1 <= n <= kTriangleMax.  The square root is only a first guess (exact up to n = 2047, where its argument is an integer
// below 2^24; a few rows off beyond): the integer loops settle the row, so the result does not depend on how sqrt
// rounds, on the host or on the device.
__host__ __device__ __forceinline__ uint32_t triangle_row(uint32_t idx, uint32_t n) {
    const float w = 2.0f * (float)n + 1.0f;
    const float d = w * w - 8.0f * (float)idx;
    const float g = (w - sqrtf(d > 0.0f ? d : 0.0f)) * 0.5f;
    uint32_t a = g > 0.0f ? (uint32_t)g : 0u;
    if (a > n - 1u) a = n - 1u;
    while (a > 0u && triangle_row_start(a, n) > idx) --a;
    while (a + 1u < n && triangle_row_start(a + 1u, n) <= idx) ++a;
    return a;
}

// Pair t < n (n + 1) / 2 -> its flat index i n + j in the full grid (< 2^32).
__host__ __device__ __forceinline__ uint32_t triangle_flat(uint32_t t, uint32_t n) {
    const uint32_t i = triangle_row(t, n);
    return i * n + i + (t - triangle_row_start(i, n));
}

}  // namespace qs
