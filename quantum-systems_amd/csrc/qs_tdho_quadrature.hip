// Two-dimensional harmonic-oscillator Coulomb elements by exact quadrature: the same tensor as
// qs_tdho.hip, from a form with no cancellation, so it holds at any shell up to the limit below.
//
//   u[p,q,r,s] = delta(m_p + m_q, m_r + m_s) * sum_{g < R} wt_g F_pr(k_g) F_qs(k_g)
//
// F_pr(k) is the form factor of the orbital pair (p, r): with the circular quanta a = n + (|m| + m) / 2,
// b = n + (|m| - m) / 2 and x = k^2 / 4 it is a signed product D(a_p, a_r; x) D(b_p, b_r; x) of two orthonormal Laguerre
// functions D(a, a'; x) = sqrt(lo! / hi!) x^((hi - lo) / 2) exp(-x / 2) L_lo^(hi - lo)(x), |D| <= 1.  F_pr F_qs is
// exp(-k^2 / 2) times an even polynomial of degree <= 4 (R - 1) in k, R = the number of shells, so the 2R-point
// Gauss-Hermite rule is exact and its R positive nodes k_g = sqrt(2) t_g with wt_g = sqrt(2) w_g exp(t_g^2) suffice.
//
// Three launches in stream order, no atomics:
//   index     (one workgroup)  m of every orbital, and the orbitals grouped by m: for a row (p, q, r) the only
//                              non-zero columns s are the group of m_p + m_q - m_r
//   form      F[p][r][g] for every unordered pair once (from lo and hi), stored at (p, r) and at (r, p)
//   assemble  one workgroup per (p, q): the m table, the groups and, a chunk of rows r at a time, F[p][r][.] in LDS;
//             the chunk of the output is built in an LDS buffer that is all +0.0 except the conserving columns, then
//             leaves as one contiguous run of 16-byte stores; the touched entries are zeroed again.  The rows of the
//             panel F[q][.][.] are gathered through the caches: staged in LDS (46 KB at l = 253) the panel left two
//             workgroups to a CU and the kernel at 0.65 of this one's rate.
// The tensor is store-bound: l^4 doubles, of which at most R per row of l are not zero.
//
// qs_tdho_coulomb_vectors stops before the l^4: the same index and form launches, then one store kernel
// writes the factors themselves, u = sum_x L_x^T (x) L_x with R (2 (m_max - m_min) + 1) vectors of l^2 doubles.

#include <math.h>

#include "qs_common.h"

namespace qs {

static constexpr int TQ_MAXL = 2048;      // orbitals
static constexpr int TQ_MAXR = 32;        // shells = nodes
static constexpr int TQ_THREADS = 256;
// Geometry and store policy of the assembly, measured in DESIGN 3.19 (tools/build_variant.sh builds the other settings)
#ifndef QS_TQ_BUF_DOUBLES
#define QS_TQ_BUF_DOUBLES 2048
#endif
#ifndef QS_TQ_NONTEMPORAL
#define QS_TQ_NONTEMPORAL 0
#endif
static constexpr int TQ_BUF_DOUBLES = QS_TQ_BUF_DOUBLES;   // the output chunk of a workgroup: 16 KB of LDS
#ifndef QS_TQ_UNROLL
#define QS_TQ_UNROLL 4
#endif

struct QuadNodes { double v[TQ_MAXR]; };

// orbital index -> (n, m) in shell order: shells of 1, 2, 3, ... states, m ascending
__host__ __device__ inline void quad_shell_nm(int p, int& n, int& m) {
    int shell = 1;
    while (shell * (shell + 1) / 2 <= p) ++shell;
    m = -(shell - 1) + 2 * (p - shell * (shell - 1) / 2);
    n = (shell - 1 - abs(m)) / 2;
}

// psi_{N-1}(t) and psi_N(t): orthonormal Hermite functions, Gaussian included (nothing under- or overflows for N <= 64)
static void hermite_functions(double t, int N, double& lo, double& hi) {
    lo = 0.0;
    hi = 0.75112554446494248286 * exp(-0.5 * t * t);          // pi^(-1/4)
    for (int n = 0; n < N; ++n) {
        const double next = t * sqrt(2.0 / (n + 1)) * hi - sqrt(n / (n + 1.0)) * lo;
        lo = hi;
        hi = next;
    }
}

// The R positive nodes of the 2R-point Gauss-Hermite rule, ascending, as k = sqrt(2) t and wt = sqrt(2) w exp(t^2):
// neighbouring zeros of psi_N are more than pi / sqrt(2 N + 1) >= 0.27 apart, so a scan in steps of 1/64 brackets each,
// and Newton's iteration on psi_N (psi_N' = sqrt(2N) psi_{N-1} - t psi_N) finishes it, kept inside the bracket.
static void quadrature_nodes(int R, double* k, double* wt) {
    const int N = 2 * R;
    const double step = 1.0 / 64.0, top = sqrt(2.0 * N + 1.0) + step;
    double lo, hi, left;
    hermite_functions(0.0, N, lo, left);
    int found = 0;
    for (double a = 0.0; a < top && found < R; a += step) {
        double right;
        hermite_functions(a + step, N, lo, right);
        if ((left < 0.0) != (right < 0.0)) {
            double t = a + 0.5 * step, lo_t = a, hi_t = a + step;
            for (int it = 0; it < 60; ++it) {
                hermite_functions(t, N, lo, hi);
                if ((hi < 0.0) == (left < 0.0)) lo_t = t; else hi_t = t;
                double next = t - hi / (sqrt(2.0 * N) * lo - t * hi);
                if (!(next > lo_t && next < hi_t)) next = 0.5 * (lo_t + hi_t);
                const bool done = fabs(next - t) <= 2e-16 * t;
                t = next;
                if (done) break;
            }
            hermite_functions(t, N, lo, hi);
            k[found] = 1.41421356237309504880 * t;
            wt[found] = 1.41421356237309504880 / (N * lo * lo);     // w = 1 / (N p_{N-1}(t)^2), p orthonormal
            ++found;
        }
        left = right;
    }
}

// D(a, b; x), x > 0: the prefactor sqrt(x^al / al!) exp(-x / 2) as a product (inside fp64 range for al <= 31 at every
// node), then the three-term recurrence of the Laguerre polynomials in orthonormal form
__device__ inline double quad_displacement(int a, int b, double x) {
    const int lo = a < b ? a : b, al = a < b ? b - a : a - b;
    double prod = 1.0;
    for (int j = 1; j <= al; ++j) prod *= x / j;
    double prev = 0.0, cur = sqrt(prod) * exp(-0.5 * x);
    for (int n = 0; n < lo; ++n) {
        const double next = ((2 * n + 1 + al - x) * cur - sqrt((double)(n * (n + al))) * prev) /
                            sqrt((double)((n + 1) * (n + 1 + al)));
        prev = cur;
        cur = next;
    }
    return cur;
}

__device__ inline void quad_orbital(const int* __restrict__ nm_table, int l, int p, int& n, int& m) {
    if (nm_table) { n = nm_table[p]; m = nm_table[l + p]; }
    else quad_shell_nm(p, n, m);
}

__device__ inline int quad_clamp(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

// index[0 .. l) = m, index[l .. 2l) = the orbitals sorted by (key, index), index[2l .. 2l + 2R) = where each key starts;
// key = m + R - 1 in [0, 2R - 2] (clamped: a table that breaks its max_shell reads wrong numbers, never out of bounds)
__global__ __launch_bounds__(TQ_THREADS) void tdho_quad_index_kernel(int* __restrict__ index, const int* __restrict__ nm_table,
                                                                    int l, int R) {
    __shared__ int s_key[TQ_MAXL];
    for (int s = threadIdx.x; s < l; s += blockDim.x) {
        int n, m;
        quad_orbital(nm_table, l, s, n, m);
        index[s] = m;
        s_key[s] = quad_clamp(m + R - 1, 0, 2 * R - 2);
    }
    __syncthreads();
    for (int s = threadIdx.x; s < l; s += blockDim.x) {
        const int key = s_key[s];
        int rank = 0;
        for (int t = 0; t < l; ++t) rank += (s_key[t] < key || (s_key[t] == key && t < s)) ? 1 : 0;
        index[l + rank] = s;
    }
    for (int k = threadIdx.x; k < 2 * R; k += blockDim.x) {
        int below = 0;
        for (int t = 0; t < l; ++t) below += s_key[t] < k ? 1 : 0;
        index[2 * l + k] = below;
    }
}

// one thread per (p, r >= p, g)
__global__ __launch_bounds__(TQ_THREADS) void tdho_quad_form_kernel(double* __restrict__ F, const int* __restrict__ nm_table,
                                                                   QuadNodes k, int l, int R) {
    const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= (int64_t)l * l * R) return;
    const int g = (int)(idx % R);
    const int64_t pr = idx / R;
    const int p = (int)(pr / l), r = (int)(pr % l);
    if (r < p) return;
    int n_p, m_p, n_r, m_r;
    quad_orbital(nm_table, l, p, n_p, m_p);
    quad_orbital(nm_table, l, r, n_r, m_r);
    const int a_p = quad_clamp(n_p + (abs(m_p) + m_p) / 2, 0, R - 1), b_p = quad_clamp(n_p + (abs(m_p) - m_p) / 2, 0, R - 1);
    const int a_r = quad_clamp(n_r + (abs(m_r) + m_r) / 2, 0, R - 1), b_r = quad_clamp(n_r + (abs(m_r) - m_r) / 2, 0, R - 1);
    const double x = 0.25 * k.v[g] * k.v[g];
    const int flips = n_p + n_r + (abs(a_p - a_r) + abs(b_p - b_r) - abs(m_p - m_r)) / 2;
    const double d = quad_displacement(a_p, a_r, x) * quad_displacement(b_p, b_r, x);
    const double f = (flips & 1) ? -d : d;
    F[((int64_t)p * l + r) * R + g] = f;
    F[((int64_t)r * l + p) * R + g] = f;
}

// Workgroup (p - p_lo, q): out[p - p_lo, q, :, :], rows_per_chunk rows r at a time.  Half-waves take rows, their lanes the
// conserving columns of the row; every element of the chunk is stored exactly once, 16 bytes per lane.
__global__ __launch_bounds__(TQ_THREADS) void tdho_quad_assemble_kernel(double* __restrict__ out, const double* __restrict__ F,
                                                                       const int* __restrict__ index, QuadNodes wt, int l, int R,
                                                                       int p_lo, int rows_per_chunk) {
    extern __shared__ double s_mem[];
    double* s_buf = s_mem;                                 // [rows_per_chunk][l]
    double* s_fp = s_buf + (int64_t)rows_per_chunk * l;    // [rows_per_chunk][R]
    double* s_w = s_fp + rows_per_chunk * R;               // [R]
    int* s_m = (int*)(s_w + R);                            // [l]
    int* s_cols = s_m + l;                                 // [l]
    int* s_start = s_cols + l;                             // [2R]

    const int tid = threadIdx.x, lane = tid & 31, hw = tid >> 5, nhw = blockDim.x >> 5;
    const int p = p_lo + (int)(blockIdx.x / (unsigned)l), q = (int)(blockIdx.x % (unsigned)l);
    const double* __restrict__ Fp = F + (int64_t)p * l * R;
    const double* __restrict__ Fq = F + (int64_t)q * l * R;

    for (int i = tid; i < 2 * l; i += blockDim.x) s_m[i] = index[i];             // m and the sorted orbitals
    for (int i = tid; i < 2 * R; i += blockDim.x) s_start[i] = index[2 * l + i];
    for (int g = tid; g < R; g += blockDim.x) s_w[g] = wt.v[g];
    for (int i = tid; i < rows_per_chunk * l; i += blockDim.x) s_buf[i] = 0.0;
    __syncthreads();
    const int m_pq = s_m[p] + s_m[q];
    double* __restrict__ dst_pq = out + (int64_t)blockIdx.x * l * l;

    for (int r0 = 0; r0 < l; r0 += rows_per_chunk) {
        const int nr = l - r0 < rows_per_chunk ? l - r0 : rows_per_chunk;
        for (int i = tid; i < nr * R; i += blockDim.x) s_fp[i] = Fp[(int64_t)r0 * R + i];
        __syncthreads();
        for (int pass = 0; pass < 2; ++pass) {
            // pass 0 fills the conserving entries of the chunk; pass 1, after the stores, zeroes them again
            for (int j = hw; j < nr; j += nhw) {
                const int M = m_pq - s_m[r0 + j], key = M + R - 1;
                if (key < 0 || key > 2 * R - 2) continue;
                for (int i = s_start[key] + lane; i < s_start[key + 1]; i += 32) {
                    const int s = s_cols[i];
                    if (s_m[s] != M) continue;
                    double acc = 0.0;
                    if (pass == 0) {
                        const double* fp = s_fp + j * R;
                        const double* __restrict__ fq = Fq + (int64_t)s * R;
#pragma unroll QS_TQ_UNROLL
                        for (int g = 0; g < R; ++g) acc = fma(fp[g] * fq[g], s_w[g], acc);
                    }
                    s_buf[j * l + s] = acc;
                }
            }
            __syncthreads();
            if (pass == 1) break;
            // the chunk is contiguous in the output: one run of n doubles, a single element ahead of it where the
            // run starts on an odd double, one behind it where an odd count is left
            double* __restrict__ dst = dst_pq + (int64_t)r0 * l;
            const int n = nr * l;
            const int head = (int)(((uintptr_t)dst >> 3) & 1);
            const int pairs = (n - head) >> 1;
            for (int i = tid; i < pairs; i += blockDim.x) {
                double2 v;
                v.x = s_buf[head + 2 * i];
                v.y = s_buf[head + 2 * i + 1];
#if QS_TQ_NONTEMPORAL
                typedef double quad_v2 __attribute__((ext_vector_type(2)));
                quad_v2 nt = {v.x, v.y};
                __builtin_nontemporal_store(nt, (quad_v2*)(dst + head + 2 * i));
#else
                *(double2*)(dst + head + 2 * i) = v;
#endif
            }
            if (tid == 0 && head) dst[0] = s_buf[0];
            if (tid == 32 && ((n - head) & 1)) dst[n - 1] = s_buf[n - 1];
            __syncthreads();
        }
    }
}

// Coulomb vectors: u[p,q,r,s] = sum_x M_x[p,r] L_x[q,s] with x = j R + g, mu_j = j - (m_max - m_min),
//   L_x[q][s] = sqrt(wt_g) F_qs[g]  where m_s - m_q == mu_j,  +0.0 elsewhere;  M_x = L_x^T.
// Workgroup (chunk, x - x_lo): TV_PAIRS * TQ_THREADS 16-byte stores of the vector's run of l^2 doubles, which starts on
// an odd double for every other vector of an odd l: one 8-byte store ahead of the pairs there, one behind them where an
// odd count is left.  Every element is stored exactly once, no atomics; mu and g are uniform over the workgroup.  The
// span m_max - m_min is read off the group starts of the index (a ballot over the 2R - 1 keys, per wave); F is gathered
// through the caches: each of its l^2 R numbers is read once over the whole rank.
static constexpr int TV_PAIRS = 4;

__device__ inline double quad_vector_element(const double* __restrict__ F, const int* __restrict__ m, int l, int R, int g,
                                             int mu, double sw, int q, int s) {
    return m[s] - m[q] == mu ? sw * F[((int64_t)q * l + s) * R + g] : 0.0;
}

__global__ __launch_bounds__(TQ_THREADS) void tdho_quad_vectors_kernel(double* __restrict__ out, const double* __restrict__ F,
                                                                      const int* __restrict__ index, QuadNodes sw, int l, int R,
                                                                      int x_lo) {
    const int tid = threadIdx.x, key = tid & 63;
    const int* __restrict__ start = index + 2 * l;
    const unsigned long long filled = __ballot(key <= 2 * R - 2 && start[key + 1] > start[key]);
    const int span = (63 - __clzll(filled)) - (__ffsll(filled) - 1);          // l >= 1: some key is filled
    const int x = x_lo + (int)blockIdx.y, j = x / R, g = x - j * R, mu = j - span;
    const double w = sw.v[g];

    double* __restrict__ dst = out + (int64_t)blockIdx.y * l * l;
    const int n = l * l;
    const int head = (int)(((uintptr_t)dst >> 3) & 1);
    const int pairs = (n - head) >> 1;
#pragma unroll
    for (int t = 0; t < TV_PAIRS; ++t) {
        const int i = ((int)blockIdx.x * TV_PAIRS + t) * TQ_THREADS + tid;
        if (i >= pairs) break;
        const int e = head + 2 * i;
        const int q0 = e / l, s0 = e - q0 * l;
        const int wrap = s0 + 1 == l ? 1 : 0;
        const int q1 = q0 + wrap, s1 = wrap ? 0 : s0 + 1;
        double2 v;
        v.x = quad_vector_element(F, index, l, R, g, mu, w, q0, s0);
        v.y = quad_vector_element(F, index, l, R, g, mu, w, q1, s1);
        *(double2*)(dst + e) = v;
    }
    if (blockIdx.x == 0) {
        if (tid == 0 && head) dst[0] = quad_vector_element(F, index, l, R, g, mu, w, 0, 0);
        if (tid == 32 && ((n - head) & 1)) dst[n - 1] = quad_vector_element(F, index, l, R, g, mu, w, l - 1, l - 1);
    }
}

// shells of the table-less form: the shell of the last orbital
static int shells_of(int64_t l) {
    int n, m;
    quad_shell_nm((int)l - 1, n, m);
    return 2 * n + abs(m) + 1;
}

static int64_t quad_workspace_bytes(int64_t l, int64_t R) {
    const int64_t bytes = 8 * l * l * R + 4 * (2 * l + 2 * R);
    return (bytes + 15) & ~int64_t(15);
}

static int rows_per_chunk(int64_t l) {
    const int64_t rc = TQ_BUF_DOUBLES / l;
    return (int)(rc < 1 ? 1 : (rc > l ? l : rc));
}

// m_max - m_min of a HOST table (n of every orbital, then m of every orbital), or of the shell order
static int64_t m_span_of(const int* table, int64_t l) {
    int lo = 0, hi = 0;
    for (int64_t p = 0; p < l; ++p) {
        int n, m;
        if (table) m = table[l + p]; else quad_shell_nm((int)p, n, m);
        if (p == 0 || m < lo) lo = m;
        if (p == 0 || m > hi) hi = m;
    }
    return (int64_t)hi - lo;
}

// the index and the form factors of a table in the workspace: F (l, l, R), then the index
static int launch_form_factors(void* workspace, const int* table, int L, int R, const QuadNodes& k, hipStream_t s) {
    double* F = (double*)workspace;
    int* index = (int*)(F + (int64_t)L * L * R);
    hipLaunchKernelGGL(tdho_quad_index_kernel, dim3(1), dim3(TQ_THREADS), 0, s, index, table, L, R);
    if (int rc = launch_status("tdho_quad_index launch")) return rc;
    note_dispatch("tdho_quad_index_kernel");
    hipLaunchKernelGGL(tdho_quad_form_kernel, dim3((unsigned)cdiv((int64_t)L * L * R, TQ_THREADS)), dim3(TQ_THREADS), 0, s, F,
                       table, k, L, R);
    if (int rc = launch_status("tdho_quad_form launch")) return rc;
    note_dispatch("tdho_quad_form_kernel");
    return QS_OK;
}

}  // namespace qs

using namespace qs;

extern "C" {

int qs_tdho_quadrature_nodes(int64_t max_shell, double* k_out, double* w_out) {
    if (!k_out || !w_out) return QS_ERR_NULL_POINTER;
    if (max_shell < 1 || max_shell > TQ_MAXR) return QS_ERR_BAD_EXTENT;
    if (!aligned(k_out, 8) || !aligned(w_out, 8)) return QS_ERR_MISALIGNED;
    quadrature_nodes((int)max_shell, k_out, w_out);
    return QS_OK;
}

int qs_tdho_coulomb_quadrature_workspace(int64_t l, int64_t max_shell, int64_t* bytes) {
    if (!bytes) return QS_ERR_NULL_POINTER;
    if (l < 1 || l > TQ_MAXL) return QS_ERR_BAD_EXTENT;
    if (max_shell <= 0) {
        if (l > TQ_MAXR * (TQ_MAXR + 1) / 2) return QS_ERR_BAD_EXTENT;
        max_shell = shells_of(l);
    }
    if (max_shell > TQ_MAXR) return QS_ERR_BAD_EXTENT;
    *bytes = quad_workspace_bytes(l, max_shell);
    return QS_OK;
}

int qs_tdho_coulomb_quadrature(void* out, const void* nm_table, int64_t l, int64_t max_shell, int64_t p_lo, int64_t p_hi,
                               void* workspace, int64_t workspace_bytes, void* stream) {
    dispatch_reset();
    if (!out || !workspace) return QS_ERR_NULL_POINTER;
    if (l < 1 || l > TQ_MAXL || p_lo < 0 || p_hi > l || p_lo >= p_hi) return QS_ERR_BAD_EXTENT;
    if (!nm_table) {
        if (l > TQ_MAXR * (TQ_MAXR + 1) / 2) return QS_ERR_BAD_EXTENT;       // more than 32 shells
        max_shell = shells_of(l);
    }
    if (max_shell < 1 || max_shell > TQ_MAXR) return QS_ERR_BAD_EXTENT;
    if (!aligned(out, 8) || !aligned(nm_table, 4) || !aligned(workspace, 16)) return QS_ERR_MISALIGNED;
    if (workspace_bytes < quad_workspace_bytes(l, max_shell)) return QS_ERR_WORKSPACE;

    const int R = (int)max_shell, L = (int)l;
    QuadNodes k, wt;
    quadrature_nodes(R, k.v, wt.v);
    for (int g = R; g < TQ_MAXR; ++g) k.v[g] = wt.v[g] = 0.0;
    double* F = (double*)workspace;
    int* index = (int*)(F + l * l * R);
    const int* table = (const int*)nm_table;
    hipStream_t s = (hipStream_t)stream;

    if (int rc = launch_form_factors(workspace, table, L, R, k, s)) return rc;

    const int rc_rows = rows_per_chunk(l);
    // at most 16 KB of chunk, 12 KB of F[p] rows and 17 KB of tables: under 64 KB at every extent
    const size_t lds = sizeof(double) * ((size_t)rc_rows * l + (size_t)rc_rows * R + R) + sizeof(int) * (2 * l + 2 * R);
    const unsigned grid = (unsigned)((p_hi - p_lo) * l);
    hipLaunchKernelGGL(tdho_quad_assemble_kernel, dim3(grid), dim3(TQ_THREADS), lds, s, (double*)out, F, index, wt, L, R,
                       (int)p_lo, rc_rows);
    note_dispatch("tdho_quad_assemble_kernel");
    return launch_status("tdho_quad_assemble launch");
}

int qs_tdho_coulomb_vectors_workspace(int64_t l, int64_t max_shell, int64_t* bytes) {
    return qs_tdho_coulomb_quadrature_workspace(l, max_shell, bytes);
}

int qs_tdho_coulomb_vectors_rank(const void* nm_table_host, int64_t l, int64_t max_shell, int64_t* rank) {
    if (!rank) return QS_ERR_NULL_POINTER;
    if (l < 1 || l > TQ_MAXL) return QS_ERR_BAD_EXTENT;
    if (!nm_table_host) {
        if (l > TQ_MAXR * (TQ_MAXR + 1) / 2) return QS_ERR_BAD_EXTENT;
        max_shell = shells_of(l);
    }
    if (max_shell < 1 || max_shell > TQ_MAXR) return QS_ERR_BAD_EXTENT;
    if (!aligned(nm_table_host, 4)) return QS_ERR_MISALIGNED;
    const int64_t span = m_span_of((const int*)nm_table_host, l);
    if (span > 2 * (max_shell - 1)) return QS_ERR_BAD_EXTENT;                // a table that breaks its max_shell
    *rank = max_shell * (2 * span + 1);
    return QS_OK;
}

int qs_tdho_coulomb_vectors(void* out, const void* nm_table, int64_t l, int64_t max_shell, int64_t x_lo, int64_t x_hi,
                            void* workspace, int64_t workspace_bytes, void* stream) {
    dispatch_reset();
    if (!out || !workspace) return QS_ERR_NULL_POINTER;
    if (l < 1 || l > TQ_MAXL || x_lo < 0 || x_lo >= x_hi) return QS_ERR_BAD_EXTENT;
    if (!nm_table) {
        if (l > TQ_MAXR * (TQ_MAXR + 1) / 2) return QS_ERR_BAD_EXTENT;       // more than 32 shells
        max_shell = shells_of(l);
    }
    if (max_shell < 1 || max_shell > TQ_MAXR) return QS_ERR_BAD_EXTENT;
    // the rank of the shell order; under a table, which lives on the device, the most its max_shell allows: vectors
    // past the table's own rank (qs_tdho_coulomb_vectors_rank) are all +0.0
    const int64_t span = nm_table ? 2 * (max_shell - 1) : m_span_of(nullptr, l);
    if (x_hi > max_shell * (2 * span + 1)) return QS_ERR_BAD_EXTENT;
    if (!aligned(out, 8) || !aligned(nm_table, 4) || !aligned(workspace, 16)) return QS_ERR_MISALIGNED;
    if (workspace_bytes < quad_workspace_bytes(l, max_shell)) return QS_ERR_WORKSPACE;

    const int R = (int)max_shell, L = (int)l;
    QuadNodes k, sw;
    quadrature_nodes(R, k.v, sw.v);
    for (int g = 0; g < R; ++g) sw.v[g] = sqrt(sw.v[g]);
    for (int g = R; g < TQ_MAXR; ++g) k.v[g] = sw.v[g] = 0.0;
    const double* F = (const double*)workspace;
    const int* index = (const int*)(F + l * l * R);
    hipStream_t s = (hipStream_t)stream;
    if (int rc = launch_form_factors(workspace, (const int*)nm_table, L, R, k, s)) return rc;

    const int64_t chunks = cdiv(l * l / 2, (int64_t)TV_PAIRS * TQ_THREADS);
    hipLaunchKernelGGL(tdho_quad_vectors_kernel, dim3((unsigned)(chunks < 1 ? 1 : chunks), (unsigned)(x_hi - x_lo)),
                       dim3(TQ_THREADS), 0, s, (double*)out, F, index, sw, L, R, (int)x_lo);
    note_dispatch("tdho_quad_vectors_kernel");
    return launch_status("tdho_quad_vectors launch");
}

}  // extern "C"
