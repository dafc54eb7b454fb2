// What the three streamed pair contractions share (qs_pair_contract.hip, qs_pair_contract_antisym.hip,
// qs_pair_contract_exchange.hip): the closing reduce-scatter butterfly and the launch; and, for the two kernels that
// walk a packed triangle of (r, s), the double-buffered chunk loop, the map t <-> (r, s), a lane's cursor along the
// walk, the kernel arguments and the body of the C entry.
#pragma once

#include "qs_contract_common.h"
#include "qs_triangle.h"

namespace qs {

// ---- all three kernels

// Sum of v[j] over the 64 lanes for every j, N a power of two <= 64: butterfly stages 32 ... 1; while a lane carries
// more than one value a stage hands half of them to the partner lane.  Returns the index j of the finished sum left in
// v[0]: a function of the lane alone (lanes that agree in the bits of the halving stages hold the same one).
template <int CNT, int M, int N>
__device__ __forceinline__ int pair_close_stage(double (&v)[N], int lane) {
    if constexpr (M == 0) {
        return 0;
    } else if constexpr (CNT > 1) {
        constexpr int half = CNT / 2;
        const bool up = (lane & M) != 0;
#pragma unroll
        for (int j = 0; j < half; ++j) {
            const double keep = up ? v[j + half] : v[j];
            const double send = up ? v[j] : v[j + half];
            v[j] = keep + __shfl_xor(send, M);
        }
        return (up ? half : 0) + pair_close_stage<half, M / 2, N>(v, lane);
    } else {
        v[0] += __shfl_xor(v[0], M);
        return pair_close_stage<1, M / 2, N>(v, lane);
    }
}

template <int N>
__device__ __forceinline__ int pair_close(double (&v)[N], int lane) {
    return pair_close_stage<N, 32, N>(v, lane);
}

// One group on one kernel instantiation: `name` is the printf format of the instantiation's name with (form, G);
// `what_attr` and `what` label a failed LDS opt-in and a failed launch in qs_last_hip_error().
template <class Kern, class Args>
inline int pair_launch(Kern kern, const Args& g, size_t lds, PerDeviceLds& once, unsigned grid, hipStream_t s,
                       const char* what_attr, const char* what, const char* name, int form, int G) {
    if (int rc = opt_in_dynamic_lds((const void*)kern, lds, once, what_attr)) return rc;
    hipLaunchKernelGGL(kern, dim3(grid), dim3(256), lds, s, g);
    note_dispatch(name, form, G);
    return launch_status(what);
}

// ---- the two kernels on a packed triangle: DIAG = with its diagonal (r <= s) or strict (r < s)

// The walk of a workgroup over nsteps steps whose T values are staged in chunks of NS steps in two LDS buffers:
// stage(c) fills buffer c & 1 with chunk c (chunk c + 1 is staged while chunk c is consumed), fetch_next(st) issues the
// loads of step st, consume(buffer, ss, st) does the products of step st = c NS + ss -- after the next step's loads
// were issued.  The caller has fetched step 0.  (qs_pair_contract.hip has the same loop in place: through this template
// its shipped instantiations measured 1-5 % slower on the same registers)
template <int NS, class Stage, class Fetch, class Consume>
__device__ __forceinline__ void pair_chunk_walk(int nsteps, Stage&& stage, Fetch&& fetch_next, Consume&& consume) {
    const int nchunks = (nsteps + NS - 1) / NS;
    stage(0);
    __syncthreads();
    for (int c = 0; c < nchunks; ++c) {
        if (c + 1 < nchunks) stage(c + 1);
        const int s_hi = nsteps - c * NS < NS ? nsteps - c * NS : NS;
        for (int ss = 0; ss < s_hi; ++ss) {
            const int st = c * NS + ss;
            if (st + 1 < nsteps) fetch_next(st + 1);
            consume(c & 1, ss, st);
        }
        __syncthreads();
    }
}

constexpr int64_t kPairMaxL = 4096;    // l^2 <= 2^24 elements: every byte offset inside a row stays below 2^32

// Packed positions of a row = (pair) rows of U: l (l + 1) / 2 with the diagonal, l (l - 1) / 2 without.
template <bool DIAG>
__host__ __device__ constexpr int pair_count(int l) { return l * (DIAG ? l + 1 : l - 1) / 2; }

// (r, s) of packed position t < pair_count(l), row-major over the runs.  The strict triangle of l is the triangle with
// diagonal of l - 1 with s shifted by one.
template <bool DIAG>
__host__ __device__ __forceinline__ void pair_unpack(int t, int l, int& r, int& s) {
    const uint32_t n = (uint32_t)(DIAG ? l : l - 1);
    const uint32_t a = triangle_row((uint32_t)t, n);
    r = (int)a;
    s = (int)(a + (DIAG ? 0u : 1u) + ((uint32_t)t - triangle_row_start(a, n)));
}

// A lane's place in the walk: packed position t <-> (r, s).  Past the end of the triangle it parks on the first
// element of the triangle (re-read, dropped by the caller's select).  A step adds 64 to s and wraps into the following
// runs, so only the first position needs the map.
template <bool DIAG>
struct PairCursor {
    int t, r, s, l, n;
    __device__ __forceinline__ PairCursor(int t0, int l_) : t(t0), r(0), s(DIAG ? 0 : 1), l(l_), n(pair_count<DIAG>(l_)) {
        if (t < n) pair_unpack<DIAG>(t, l, r, s);
    }
    __device__ __forceinline__ bool term() const { return t < n; }           // the position is a term of the sum
    __device__ __forceinline__ unsigned offset() const { return t < n ? (unsigned)(r * l + s) : (DIAG ? 0u : 1u); }
    __device__ __forceinline__ void advance() {
        t += 64;
        if (t < n) {
            s += 64;
            while (s >= l) {
                s += r + (DIAG ? 1 : 2) - l;
                ++r;
            }
        }
    }
};

struct PairTriArgs {
    const double* U;
    const double* T;          // first amplitude of the group, [ng][l][l]
    double* S;                // first result of the group, [ng][l][l]
    int64_t ldu;
    int l, ng;                // ng: amplitudes of this launch, 1 ... G of the instantiation
};

// The two forms: both operands fp64 (0), or both complex128 (1); a real U against complex T is two fp64 columns per
// amplitude (the Python layer).  Negative = the pair is refused.
inline int pair_tri_form(int u_dtype, int t_dtype) {
    if (!dtype_ok(u_dtype) || !dtype_ok(t_dtype) || u_dtype != t_dtype) return QS_ERR_BAD_DTYPE;
    return u_dtype == QS_C128 ? 1 : 0;
}

// The form, or the refusal of the dtype pair / of the extents.
template <bool DIAG>
inline int pair_tri_query(int u_dtype, int t_dtype, int64_t l, int64_t K) {
    const int form = pair_tri_form(u_dtype, t_dtype);
    if (form < 0) return form;
    return l >= (DIAG ? 1 : 2) && l <= kPairMaxL && K >= 1 && K <= 65536 ? form : QS_ERR_BAD_EXTENT;
}

// Both workspace queries: the same refusals, else 0 (the triangle of a row is never split: every sum is closed inside
// its wave).
template <bool DIAG>
inline int64_t pair_tri_workspace(int u_dtype, int t_dtype, int64_t l, int64_t K) {
    const int form = pair_tri_query<DIAG>(u_dtype, t_dtype, l, K);
    return form < 0 ? form : 0;
}

// The body of both C entries: the refusals in the order of the ABI, then launch(form, args, grid, stream) for every group
// of the form's group size (shipped[form], or the tuning run's); a workgroup takes per_wg (pair) rows.
template <bool DIAG, class Launch>
inline int pair_tri_entry(int per_wg, const int (&shipped)[2], Launch&& launch, int u_dtype, int t_dtype, const void* U,
                          const void* T, void* S, int64_t l, int64_t K, int64_t ldu, int64_t work_elems, void* stream) {
    dispatch_reset();
    const int form = pair_tri_query<DIAG>(u_dtype, t_dtype, l, K);
    if (form < 0) return form;
    if (ldu < l * l || ldu > (int64_t(1) << 24)) return QS_ERR_BAD_EXTENT;
    if (!U || !T || !S) return QS_ERR_NULL_POINTER;
    const int64_t es = (int64_t)elem_size(t_dtype);
    if (!aligned(U, (size_t)es) || !aligned(T, (size_t)es) || !aligned(S, (size_t)es)) return QS_ERR_MISALIGNED;
    const int64_t s_bytes = K * l * l * es;
    if (overlaps(S, s_bytes, U, ((l * l - 1) * ldu + l * l) * es) || overlaps(S, s_bytes, T, s_bytes)) return QS_ERR_ALIAS;
    if (work_elems < 0) return QS_ERR_WORKSPACE;

    const int w = form + 1;
    PairTriArgs g{};
    g.U = (const double*)U;
    g.l = (int)l;
    g.ldu = ldu;
    const unsigned grid = (unsigned)cdiv(pair_count<DIAG>((int)l), per_wg);
    return for_each_group(K, group_size(g_tune.pair_contract_g, shipped[form]), [&](int64_t k0, int ng) {
        g.ng = ng;
        g.T = (const double*)T + k0 * l * l * w;
        g.S = (double*)S + k0 * l * l * w;
        return launch(form, g, grid, (hipStream_t)stream);
    });
}

}  // namespace qs
