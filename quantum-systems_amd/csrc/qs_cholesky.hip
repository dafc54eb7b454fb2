// Pivoted Cholesky decomposition of the two-body tensor, read in place.
//
// With G[(r,p),(q,s)] = u[p,q,r,s] (flat index first * m + second, n = m^2), Hermitian positive semidefinite for a
// positive interaction, G = V V^H and the stored vectors L_x = conj(V_x) (m x m, row x of a (capacity, n) buffer) give
//   u[p,q,r,s] = sum_x conj(L_x[r,p]) L_x[q,s].
// Left-looking: step j takes the pivot piv = (q*, s*) = argmax of the residual diagonal d (lowest flat index on ties),
// stops when d[piv] <= tau or when any d[i] is a NaN (dmax is then that NaN), and otherwise forms, for every i = (r, p),
//   L_j[i] = (u[s*, r, q*, p] - sum_{x<j} L_x[i] conj(L_x[piv])) / sqrt(d[piv]),    d[i] -= |L_j[i]|^2,   d[piv] = 0.
// u[s*, r, q*, p] is the conjugated pivot column (G is Hermitian): contiguous in p, no stride-m^3 gather.
//
// The sum over x is the whole cost: step j reads j n elements, a run of r steps n r^2 / 2, and nothing is reused
// between steps, so there is nothing for a matrix instruction to do.  A thread owns ONE element i and streams down x
// (row x of the buffer is n contiguous elements: every load of a wave is one contiguous run), the j coefficients
// conj(L_x[piv]) are staged in LDS once per workgroup (chunks of kChunk) and read as broadcasts, and the sum runs in
// four independent chains (x mod 4) closed in a fixed order: the bits depend on (u, tau) only -- not on the capacity,
// not on where a run was interrupted and resumed.
//
// Two plain launches per step, in stream order, no grid-wide barrier and no spin wait:
//   cholesky_pivot_kernel   one workgroup: argmax / min over the per-workgroup partial results of the launch before
//                           it, the stop decision, the pivot and sqrt(d[piv]) into the state words;
//   cholesky_update_kernel  the step, and the partial argmax / min of the new diagonal of its 256 elements.
// Pivot, rank and the stop flag live in device memory; once the flag is set every later launch returns at once.  The
// host enqueues kBlock steps, then reads the state back ONCE (the call blocks there) and goes on or returns.

#include <cmath>

#include "qs_common.h"

namespace qs {

constexpr int kChunk = 512;             // coefficients staged in LDS at a time (a multiple of 4)
constexpr int64_t kBlock = 64;          // steps enqueued between two read-backs of the state
constexpr int64_t kStateBytes = 64;     // the state words, then one Partial per workgroup

struct CholState {
    int64_t stop;       // sticky: set by the pivot launch that ends the run
    int64_t rank;       // vectors complete once the launches enqueued so far have run
    int64_t piv;        // this step's pivot
    double root;        // sqrt(d[piv])
    double dmax, dmin;  // extremes of the residual diagonal as the last pivot launch saw it
};

struct Partial {
    double vmax;
    int64_t imax;
    double vmin;
    int64_t pad;
};

struct CholArgs {
    const double* u;
    double* L;          // (capacity, n) elements
    double* d;          // n
    int64_t* pivots;    // capacity
    CholState* state;
    Partial* part;      // cdiv(n, 256)
    int64_t m, n, capacity;
    double tau;
};

// larger value wins, the lower index on equal values; a NaN beats every number, offered (v2 != v2) or held (no
// comparison with a held NaN is true), so one NaN among the candidates is the maximum of every reduction it enters
__device__ inline void take_max(double& v, int64_t& i, double v2, int64_t i2) {
    if (v2 != v2 || v2 > v || (v2 == v && i2 < i)) { v = v2; i = i2; }
}

// (max, argmax, min) of the workgroup's 256 candidates, valid in thread 0
__device__ inline void block_extremes(double& vmax, int64_t& imax, double& vmin) {
    __shared__ double s_max[256], s_min[256];
    __shared__ int64_t s_idx[256];
    const int tid = threadIdx.x;
    s_max[tid] = vmax; s_idx[tid] = imax; s_min[tid] = vmin;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if (tid < w) {
            take_max(vmax, imax, s_max[tid + w], s_idx[tid + w]);
            vmin = fmin(vmin, s_min[tid + w]);
            s_max[tid] = vmax; s_idx[tid] = imax; s_min[tid] = vmin;
        }
        __syncthreads();
    }
}

// Start of a call: clears the state, (fresh run) d[(r,p)] = Re u[p,r,r,p], and the partial extremes of d.
template <int W>
__global__ __launch_bounds__(256) void cholesky_start_kernel(const CholArgs g, const int fresh, const int64_t rank) {
    const int tid = threadIdx.x;
    const int64_t i = (int64_t)blockIdx.x * 256 + tid, n = g.n, m = g.m;
    if (blockIdx.x == 0 && tid == 0) {
        CholState s{};
        s.rank = rank;
        *g.state = s;
    }
    double v = -INFINITY, lo = INFINITY;
    if (i < n) {
        if (fresh) {
            const int64_t r = i / m, p = i - r * m;
            g.d[i] = g.u[(((p * m + r) * m + r) * m + p) * W];
        }
        v = lo = g.d[i];
    }
    int64_t idx = i < n ? i : n - 1;
    block_extremes(v, idx, lo);
    if (tid == 0) g.part[blockIdx.x] = Partial{v, idx, lo, 0};
}

// Step j: the pivot and the stop decision from the partial extremes.
__global__ __launch_bounds__(256) void cholesky_pivot_kernel(const CholArgs g, const int64_t j, const int64_t nblk) {
    if (g.state->stop) return;
    const int tid = threadIdx.x;
    double v = -INFINITY, lo = INFINITY;
    int64_t idx = g.n - 1;
    for (int64_t b = tid; b < nblk; b += 256) {
        const Partial p = g.part[b];
        take_max(v, idx, p.vmax, p.imax);
        lo = fmin(lo, p.vmin);
    }
    block_extremes(v, idx, lo);
    if (tid) return;
    CholState* s = g.state;
    s->dmax = v;
    s->dmin = lo;
    if (j >= g.capacity || !(v > g.tau)) {      // a NaN anywhere on the diagonal arrives here as v (take_max): it stops too
        s->stop = 1;
        s->rank = j;
        return;
    }
    s->piv = idx;
    s->root = sqrt(v);
    s->rank = j + 1;
    g.pivots[j] = idx;
}

// Step j: the new vector, the new diagonal and its partial extremes.  W doubles per element.
template <int W>
__global__ __launch_bounds__(256) void cholesky_update_kernel(const CholArgs g, const int64_t j) {
    __shared__ double coef[kChunk * W];
    if (g.state->stop) return;
    const int tid = threadIdx.x;
    const int64_t n = g.n, m = g.m, piv = g.state->piv;
    const double root = g.state->root;
    const int64_t i = (int64_t)blockIdx.x * 256 + tid;
    const bool ok = i < n;
    const int64_t ic = ok ? i : n - 1;          // lanes past the end read the last element and store nothing

    double acc[4][W];
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int w = 0; w < W; ++w) acc[a][w] = 0.0;

    auto term = [&](int a, const double* lx, int x) {
        if constexpr (W == 1) {
            acc[a][0] = __builtin_fma(lx[0], coef[x], acc[a][0]);
        } else {
            const double lr = lx[0], li = lx[1], cr = coef[2 * x], ci = coef[2 * x + 1];
            acc[a][0] = __builtin_fma(-li, ci, __builtin_fma(lr, cr, acc[a][0]));
            acc[a][1] = __builtin_fma(li, cr, __builtin_fma(lr, ci, acc[a][1]));
        }
    };

    for (int64_t c0 = 0; c0 < j; c0 += kChunk) {
        const int cn = (int)(j - c0 < kChunk ? j - c0 : kChunk);
        if (c0) __syncthreads();
        for (int x = tid; x < cn; x += 256) {       // conj(L_x[piv])
            const double* src = g.L + ((c0 + x) * n + piv) * W;
            coef[x * W] = src[0];
            if constexpr (W == 2) coef[x * 2 + 1] = -src[1];
        }
        __syncthreads();
        const double* col = g.L + (c0 * n + ic) * W;
        const int64_t pitch = n * W;
        int x = 0;
#pragma unroll 2
        for (; x + 4 <= cn; x += 4) {
#pragma unroll
            for (int a = 0; a < 4; ++a) term(a, col + (x + a) * pitch, x + a);
        }
        for (; x < cn; ++x) term(x & 3, col + x * pitch, x);      // kChunk is a multiple of 4: x & 3 is the chain of c0 + x
    }

    // the conjugated pivot column: u[s*, r, q*, p]
    const int64_t r = ic / m, p = ic - r * m, qs = piv / m, ss = piv - qs * m;
    const double* ue = g.u + (((ss * m + r) * m + qs) * m + p) * W;
    double val[W], dn = g.d[ic];
#pragma unroll
    for (int w = 0; w < W; ++w) {
        val[w] = (ue[w] - ((acc[0][w] + acc[1][w]) + (acc[2][w] + acc[3][w]))) / root;
        dn = __builtin_fma(-val[w], val[w], dn);
    }
    if (ic == piv) dn = 0.0;
    if (ok) {
        double* out = g.L + (j * n + i) * W;
#pragma unroll
        for (int w = 0; w < W; ++w) out[w] = val[w];
        g.d[i] = dn;
    }
    double v = ok ? dn : -INFINITY, lo = ok ? dn : INFINITY;
    int64_t idx = ic;
    block_extremes(v, idx, lo);
    if (tid == 0) g.part[blockIdx.x] = Partial{v, idx, lo, 0};
}

static inline bool cholesky_extents_ok(int64_t m, int64_t capacity) {
    if (m < 1 || m > 46340 || capacity < 1) return false;                    // m^2 <= 2^31 - 1
    return capacity <= INT64_MAX / (m * m * 16);                             // the buffer's bytes fit int64
}

}  // namespace qs

using namespace qs;

extern "C" {

int64_t qs_cholesky_two_body_workspace(int dtype, int64_t m, int64_t capacity) {
    if (!dtype_ok(dtype)) return QS_ERR_BAD_DTYPE;
    if (!cholesky_extents_ok(m, capacity)) return QS_ERR_BAD_EXTENT;
    return kStateBytes + cdiv(m * m, 256) * (int64_t)sizeof(Partial);
}

int64_t qs_cholesky_two_body_block(void) { return kBlock; }

int qs_cholesky_two_body(int dtype, const void* u, int64_t m, double tau, void* vectors, int64_t capacity,
                         int64_t* rank, double* diag, int64_t* pivots, double* extremes, void* work,
                         int64_t work_bytes, void* stream) {
    dispatch_reset();
    if (!dtype_ok(dtype)) return QS_ERR_BAD_DTYPE;
    if (!cholesky_extents_ok(m, capacity) || !(tau >= 0.0)) return QS_ERR_BAD_EXTENT;
    if (!u || !vectors || !rank || !diag || !pivots || !extremes || !work) return QS_ERR_NULL_POINTER;
    if (!aligned(rank, 8) || !aligned(extremes, 8)) return QS_ERR_MISALIGNED;
    const int64_t rank_in = *rank;
    if (rank_in < 0 || rank_in > capacity) return QS_ERR_BAD_EXTENT;
    if (!aligned(u, elem_size(dtype)) || !aligned(vectors, elem_size(dtype)) || !aligned(diag, 8) || !aligned(pivots, 8) ||
        !aligned(work, 16))
        return QS_ERR_MISALIGNED;
    if (work_bytes < qs_cholesky_two_body_workspace(dtype, m, capacity)) return QS_ERR_WORKSPACE;

    hipStream_t s = (hipStream_t)stream;
    hipStreamCaptureStatus capture = hipStreamCaptureStatusNone;
    if (int rc = hip_status(hipStreamIsCapturing(s, &capture), "hipStreamIsCapturing")) return rc;
    if (capture != hipStreamCaptureStatusNone)      // the state cannot be read back inside a capture
        return hip_status(hipErrorStreamCaptureUnsupported, "qs_cholesky_two_body on a capturing stream");
    const int64_t n = m * m, nblk = cdiv(n, 256);
    const CholArgs g{(const double*)u, (double*)vectors, diag, pivots, (CholState*)work,
                     (Partial*)((char*)work + kStateBytes), m, n, capacity, tau};
    const dim3 grid((unsigned)nblk), block(256);
    const bool cplx = dtype == QS_C128;
    const char* update_name = cplx ? "qs::cholesky_update_kernel<2>" : "qs::cholesky_update_kernel<1>";

    if (cplx) hipLaunchKernelGGL(cholesky_start_kernel<2>, grid, block, 0, s, g, rank_in == 0, rank_in);
    else hipLaunchKernelGGL(cholesky_start_kernel<1>, grid, block, 0, s, g, rank_in == 0, rank_in);
    note_dispatch(cplx ? "qs::cholesky_start_kernel<2>" : "qs::cholesky_start_kernel<1>");
    if (int rc = launch_status("cholesky start launch")) return rc;

    // steps rank_in ... capacity; the last one is the pivot launch alone, which ends the run on the capacity
    int64_t pivots_run = 0, updates_run = 0;
    int rc = QS_OK;
    CholState host{};
    for (int64_t j0 = rank_in; !rc && !host.stop; j0 += kBlock) {
        for (int64_t j = j0; !rc && j < j0 + kBlock && j <= capacity; ++j) {
            hipLaunchKernelGGL(cholesky_pivot_kernel, dim3(1), block, 0, s, g, j, nblk);
            ++pivots_run;
            rc = launch_status("cholesky pivot launch");
            if (rc || j == capacity) break;
            if (cplx) hipLaunchKernelGGL(cholesky_update_kernel<2>, grid, block, 0, s, g, j);
            else hipLaunchKernelGGL(cholesky_update_kernel<1>, grid, block, 0, s, g, j);
            ++updates_run;
            rc = launch_status("cholesky update launch");
        }
        if (rc) break;
        rc = hip_status(hipMemcpyAsync(&host, g.state, sizeof(CholState), hipMemcpyDeviceToHost, s), "hipMemcpyAsync(state)");
        if (!rc) rc = hip_status(hipStreamSynchronize(s), "hipStreamSynchronize");
    }
    // the record folds repeats of ONE name to "name xN": the alternating launches are noted kernel by kernel
    for (int64_t t = 0; t < pivots_run; ++t) note_dispatch("qs::cholesky_pivot_kernel");
    for (int64_t t = 0; t < updates_run; ++t) note_dispatch("%s", update_name);
    if (rc) return rc;
    *rank = host.rank;
    extremes[0] = host.dmax;
    extremes[1] = host.dmin;
    return QS_OK;
}

}  // extern "C"
