// Occupation strings as 64-bit masks (bit p = orbital p occupied) and the search of an ascending list of them: what the
// determinant kernels (qs_det_ci.hip) and the string tables (qs_string_ci.hip) share.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace qs {

__device__ __forceinline__ uint64_t dc_bit(int p) { return uint64_t(1) << p; }

// orbitals strictly between a and b
__device__ __forceinline__ uint64_t dc_between(int a, int b) {
    const int lo = a < b ? a : b, hi = a < b ? b : a;
    return (dc_bit(hi) - 1) & ~((dc_bit(lo) << 1) - 1);
}

__device__ __forceinline__ int dc_lowest(uint64_t x) { return __ffsll((unsigned long long)x) - 1; }

// position of mask J in dets, or -1
__device__ __forceinline__ int64_t dc_find(const int64_t* __restrict__ dets, int64_t dim, uint64_t J) {
    int64_t lo = 0, hi = dim;
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if ((uint64_t)dets[mid] < J) lo = mid + 1;
        else hi = mid;
    }
    return (lo < dim && (uint64_t)dets[lo] == J) ? lo : -1;
}

}  // namespace qs
