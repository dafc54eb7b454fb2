// Device toolkit of the fused small-basis kernels on v_mfma_f64_4x4x4_4b_f64 (Out_t = Lm . In_t . R: qs_sandwich4.hip,
// qs_sandwich4b.hip, qs_small4.hip, qs_quad4s.h, qs_pair4s.h): ONE copy of what every one of them needs.  Device code only
// (the trace read-out at the end, development builds, is the exception).
#pragma once

#include <type_traits>

#include "qs_common.h"
#include "qs_fast_items.h"      // f64x2, uniform64

namespace qs {

typedef unsigned u32x2 __attribute__((ext_vector_type(2)));
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));

// f(I), f(I + 1), ... f(N - 1) with compile-time arguments, in this order (halving: the 1152 groups of a 96-orbital quad would
// exceed the template recursion depth one at a time)
template <int I, int N, class F>
__device__ __forceinline__ void unroll(F&& f) {
    if constexpr (N - I == 1) {
        f(std::integral_constant<int, I>{});
    } else if constexpr (N - I > 1) {
        constexpr int MID = I + (N - I) / 2;
        unroll<I, MID>(f);
        unroll<MID, N>(f);
    }
}

// The instruction issues four independent 4 x 4 x 4 products ("blocks").  Lane layout (tools/probe_mfma4_layout.hip), lane =
// x + 4 y + 16 z:  A holds row x, block y, k z;  B holds k z, block y, column x;  D holds row z, block y, column x -- the
// accumulator layout is the B-operand layout, so Y = In . R goes from the accumulators straight into Lm . Y.
// e: this lane's element z * 4 + x of a 4 x 4 fragment in the R / Lm tables.  (qs_sandwich4.hip and qs_sandwich4b.hip spell
// the four out: through the struct the compiler schedules them differently, profiles/mfma4_toolkit_isa.txt.)
struct Lane4 {
    int x, y, z, e;
};
__device__ __forceinline__ Lane4 lane4(int lane) {
    const int x = lane & 3, y = (lane >> 2) & 3, z = lane >> 4;
    return {x, y, z, z * 4 + x};
}

__device__ __forceinline__ double mfma4(double a, double b, double c) {
    return __builtin_amdgcn_mfma_f64_4x4x4f64(a, b, c, 0, 0, 0);
}

// The parked-lane convention: a lane whose element does not exist gets this lane offset, past num_records of every
// descriptor below -- the hardware answers its load with 0.0 and drops its store, no branch, no VALU work.
constexpr unsigned kParked = 0x80000000u;

// Buffer descriptor in SGPRs for a wave-uniform address; `range` = num_records in bytes (0: every load answers 0.0 and every
// store is dropped -- the descriptor-range ablations of development builds).
__device__ __forceinline__ auto uniform_rsrc(uint64_t addr, int range = 0x7fffffff) {
    return __builtin_amdgcn_make_buffer_rsrc(reinterpret_cast<void*>(uniform64(addr)), (short)0, range, 0x00020000);
}
// ... for tuple `tuple` of a batch: `per_tuple` items of `item_stride` elements each
template <class T>
__device__ __forceinline__ auto tuple_rsrc(const T* base, unsigned tuple, int per_tuple, int64_t item_stride,
                                           int range = 0x7fffffff) {
    return uniform_rsrc(reinterpret_cast<uint64_t>(base + (int64_t)tuple * per_tuple * item_stride), range);
}

// workgroup barrier that waits for this wave's LDS traffic only (a __syncthreads would also drain the fetches in flight)
__device__ __forceinline__ void lds_barrier() {
    __builtin_amdgcn_s_waitcnt(0xC07F);        // lgkmcnt(0), vmcnt / expcnt untouched
    __builtin_amdgcn_s_barrier();
}

// SGPR fence: the compiler may not fold what it knows about v into later address arithmetic
__device__ __forceinline__ unsigned opaque(unsigned v) {
    asm volatile("" : "+s"(v));
    return v;
}

// Position of element (row, item, k) of a fragment in its 512-byte transit slot (slot parity par): 128-byte line
// k, 8-byte bank pair (row ^ 2 (k & 1)) + 4 (item ^ ((k >> 1) | 2 par)).  Any 16 adjacent lanes that go to LDS
// together -- (row, item) at fixed k when the MFMA lanes read, either of the two fetch layouts when the fetch
// lanes write their first or their second element -- hit 16 different bank pairs (searched over the XOR masks
// that are linear in (k, par)); the plain lane order would put four lanes of every write on each bank.
__device__ __forceinline__ constexpr unsigned slot_pos(int row, int item, int k, int par) {
    return (unsigned)(16 * k + ((row ^ ((k & 1) << 1)) + 4 * (item ^ ((k >> 1) | (par << 1)))));
}

// Work units [0, n) over the grid (a multiple of 8 workgroups): XCD x = workgroup % 8 takes the x-th contiguous range of
// `per` units and neighbouring workgroups of an XCD take neighbouring units (they share lines of the tensor in the XCD's
// L2).  A workgroup walks first, first + stride, ... below end; `split` adjacent workgroups of an XCD share a unit.
struct XcdRange {
    unsigned first, end, stride;
};
__device__ __forceinline__ XcdRange xcd_range_of(unsigned n, unsigned per, unsigned split = 1) {
    const unsigned n_xcd = 8, xcd = blockIdx.x % n_xcd, slot = (blockIdx.x / n_xcd) / split;
    const unsigned end = (xcd + 1) * per < n ? (xcd + 1) * per : n;
    return {xcd * per + slot, end, (gridDim.x / n_xcd) / split};
}
__device__ __forceinline__ XcdRange xcd_range(unsigned n, unsigned split = 1) {
    return xcd_range_of(n, (n + 7) / 8, split);
}

}  // namespace qs

// Development builds with -DQS_S4_TRACE=<workgroup> (tools/trace_s4.py): shader-clock stamps of that workgroup's wave 0 at every
// step, in a device array `arr` of 4096 (with its count `arr_n`); the kernel has `wave` and `lane`.  The stamp index lives in a
// register (a counter in memory would put a global load in front of every stamp).
#ifdef QS_S4_TRACE
#define QS_TRACE_SYMBOLS(arr)                  \
    __device__ unsigned long long arr[4096];   \
    __device__ unsigned arr##_n;
#define QS_TRACE_BEGIN \
    unsigned tr_n = 0; \
    const unsigned long long tr_real0 = __builtin_amdgcn_s_memrealtime();
#define QS_TRACE_STAMP(arr, tag)                                                                   \
    if (blockIdx.x == QS_S4_TRACE && wave == 0) {                                                  \
        if (lane == 0 && tr_n < 4096) arr[tr_n] = (__builtin_amdgcn_s_memtime() << 8) | (tag);     \
        ++tr_n;                                                                                    \
    }
#define QS_TRACE_DONE(arr)                                                                                       \
    if (blockIdx.x == QS_S4_TRACE && wave == 0 && lane == 0) {                                                   \
        arr##_n = tr_n;                                                                                          \
        arr[4095] = __builtin_amdgcn_s_memrealtime() - tr_real0;     /* 100 MHz ticks, entry to exit */           \
    }
// the exported pair arr_reset() / arr_read(dst), dst: device buffer of 4097 x 8 bytes: count, stamps
#define QS_TRACE_EXPORTS(arr)                                                                       \
    extern "C" int arr##_reset(void) {                                                              \
        unsigned zero = 0;                                                                          \
        return (int)hipMemcpyToSymbol(HIP_SYMBOL(qs::arr##_n), &zero, sizeof(zero));                \
    }                                                                                               \
    extern "C" int arr##_read(void* dst) {                                                          \
        unsigned n = 0;                                                                             \
        (void)hipMemcpyFromSymbol(&n, HIP_SYMBOL(qs::arr##_n), sizeof(n));                          \
        unsigned long long nn = n;                                                                  \
        (void)hipMemcpy(dst, &nn, 8, hipMemcpyHostToDevice);                                        \
        void* src = nullptr;                                                                        \
        (void)hipGetSymbolAddress(&src, HIP_SYMBOL(qs::arr));                                       \
        return (int)hipMemcpy((char*)dst + 8, src, 4096 * 8, hipMemcpyDeviceToDevice);              \
    }
#else
#define QS_TRACE_SYMBOLS(arr)
#define QS_TRACE_BEGIN
#define QS_TRACE_STAMP(arr, tag)
#define QS_TRACE_DONE(arr)
#define QS_TRACE_EXPORTS(arr)
#endif
