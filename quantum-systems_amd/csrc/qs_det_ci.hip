// H c on Slater determinants (direct configuration interaction), its diagonal and the one- and two-body (transition)
// densities of its vectors.
//   H = sum_pq ht[p,q] a+_p a_q + 1/4 sum_pqrs ut[p,q,r,s] a+_p a+_q a_s a_r,   ut[p,q,r,s] = <pq|rs> - <pq|sr>
// A determinant is a 64-bit occupation mask over m <= 63 orthonormal spin orbitals (bit p = orbital p occupied); the
// space is an ascending, duplicate-free list dets[dim] of masks with N bits each -- the full space, a spin sector, an
// excitation-truncated space or any other subset.  A connection whose target is not in the list contributes nothing:
// the Hamiltonian of a subset is the projection of the full one.
//
//   D[I]        = <I|H|I> = sum_{i in I} ht[i,i] + sum_{i<j in I} ut[i,j,i,j]                        (real)
//   sigma[k, I] = D[I] c[k,I] + sum_{p in I, q not in I} s (ht[p,q] + sum_{j in I, j != p} ut[p,j,q,j]) c[k, I-p+q]
//                             + sum_{p1<p2 in I, q1<q2 not in I} s ut[p1,p2,q1,q2] c[k, I-p1-p2+q1+q2]
//   rho[q, p]   = sum_I conj(c[I]) s c[I-p+q]                                                        (p in I, q not in I or q = p)
// s = (-1)^(occupied orbitals strictly between the moved ones): one popcount of the mask between p and q for a single
// excitation; for a double, that of p1 -> q1 on I times that of p2 -> q2 on the intermediate I-p1+q1.
//
// sigma is the GATHER form: the thread that owns I walks I's excitations with bit arithmetic (lowest set bit of the
// occupied / of the empty mask, no occupation lists, so nothing is indexed in registers), finds the target by binary
// search in dets, forms the matrix element from ht (a copy in LDS) and ut, and feeds the running sums of the G vectors
// of the launch.  c is stored with the vectors of one determinant adjacent (c[J * ldc + k]): the G values one
// connection needs come from one or two cache lines.  ut, dets and c are gathers meant to stay in L2 / MALL.
// One thread per determinant, 64 threads per workgroup: all lanes run the same trip counts (N and m - N are uniform),
// a space below one wave or off a multiple of 64 only leaves lanes idle, and nothing depends on K.
//
// Reproducible: no atomics, every product an explicit fma, the order of a determinant's sum is the order of the walk
// above (fixed by I and dets), and the chain of vector k never sees another vector: sigma[k] has the same bits alone, at
// any position in any batch and on any instantiation (a partial last group takes the smallest one that holds it).
// The densities map one workgroup to each output -- (p, q) of rho, the unique (p < q, r < s) of gamma2 --, stride over
// dets and close with one butterfly and a fixed sum over the four waves.  They take a bra and a ket vector:
//   rho[q, p]          = sum_IJ conj(bra[I]) <I| a+_p a_q |J> ket[J]
//   gamma2[p, q, r, s] = sum_IJ conj(bra[I]) <I| a+_p a+_q a_s a_r |J> ket[J]
// so that <bra|H|ket> = sum_pq ht[p,q] rho[q,p] + 1/4 sum_pqrs ut[p,q,r,s] gamma2[p,q,r,s]; bra = ket is a state's density.

#include "qs_contract_common.h"
#include "qs_strings.h"

namespace qs {

constexpr int kDcBlock = 64;           // determinants (threads) per workgroup of sigma and of the diagonal
constexpr int kDcRhoBlock = 256;       // threads of the density's workgroup
// Shipped group size per form {fp64, complex128}: the largest G whose code object has no scratch and no spills; the
// sweep of tools/det_ci_bench.py is monotone in G in both forms (profiles/r10_det_ci.txt).
constexpr int kDcGroup[2] = {8, 8};

struct DcArgs {
    const double* ht;         // (m, m)
    const double* ut;         // (m, m, m, m), anti-symmetrised
    const int64_t* dets;      // [dim], ascending
    const double* D;          // [dim]
    const double* c;          // first vector of the group: element (J, g) at c[J * ldc + g]
    double* sigma;            // first vector of the group: element (g, I) at sigma[g * dim + I]
    int64_t dim, ldc;
    int m, ng;                // ng = vectors of this launch, 1 ... G of the instantiation
};

// acc[g] += e * c[J, g] for the launch's vectors; CW = doubles per element
template <int CW, int G>
__device__ __forceinline__ void dc_feed(double (&acc)[G * CW], const double (&e)[CW], const double* __restrict__ cj, int ng) {
#pragma unroll
    for (int g = 0; g < G; ++g) {
        if (g < ng) {
            if constexpr (CW == 1) {
                acc[g] = fma(e[0], cj[g], acc[g]);
            } else {
                const double cr = cj[2 * g], ci = cj[2 * g + 1];
                acc[2 * g] = fma(-e[CW - 1], ci, fma(e[0], cr, acc[2 * g]));
                acc[2 * g + 1] = fma(e[CW - 1], cr, fma(e[0], ci, acc[2 * g + 1]));
            }
        }
    }
}

template <int CW, int G>
__global__ __launch_bounds__(kDcBlock) void det_ci_sigma_kernel(const DcArgs a) {
    extern __shared__ __attribute__((aligned(16))) double dc_ht[];
    const int m = a.m;
    for (int idx = threadIdx.x; idx < m * m * CW; idx += kDcBlock) dc_ht[idx] = a.ht[idx];
    __syncthreads();
    const int64_t row = (int64_t)blockIdx.x * kDcBlock + threadIdx.x;
    if (row >= a.dim) return;

    const int64_t* __restrict__ dets = a.dets;
    const double* __restrict__ ut = a.ut;
    const uint64_t I = (uint64_t)dets[row] & (dc_bit(m) - 1);          // a bit at or above m would index past ut
    const uint64_t empty = ~I & (dc_bit(m) - 1);

    double acc[G * CW];
#pragma unroll
    for (int j = 0; j < G * CW; ++j) acc[j] = 0.0;
    {
        double d[CW];
        d[0] = a.D[row];
        if constexpr (CW == 2) d[1] = 0.0;
        dc_feed<CW, G>(acc, d, a.c + row * a.ldc * CW, a.ng);
    }

    // single excitations p -> q
    for (uint64_t po = I; po; po &= po - 1) {
        const int p = dc_lowest(po);
        const uint64_t rest = I ^ dc_bit(p);
        for (uint64_t vq = empty; vq; vq &= vq - 1) {
            const int q = dc_lowest(vq);
            const int64_t pos = dc_find(dets, a.dim, rest | dc_bit(q));
            if (pos < 0) continue;
            double e[CW];
#pragma unroll
            for (int w = 0; w < CW; ++w) e[w] = dc_ht[(p * m + q) * CW + w];
            for (uint64_t oj = rest; oj; oj &= oj - 1) {
                const int j = dc_lowest(oj);
                const double* x = ut + (size_t)(((p * m + j) * m + q) * m + j) * CW;
#pragma unroll
                for (int w = 0; w < CW; ++w) e[w] += x[w];
            }
            if (__popcll((unsigned long long)(I & dc_between(p, q))) & 1) {
#pragma unroll
                for (int w = 0; w < CW; ++w) e[w] = -e[w];
            }
            dc_feed<CW, G>(acc, e, a.c + pos * a.ldc * CW, a.ng);
        }
    }

    // double excitations p1 < p2 -> q1 < q2
    for (uint64_t po1 = I; po1; po1 &= po1 - 1) {
        const int p1 = dc_lowest(po1);
        for (uint64_t po2 = po1 & (po1 - 1); po2; po2 &= po2 - 1) {
            const int p2 = dc_lowest(po2);
            const uint64_t rest = I ^ dc_bit(p1) ^ dc_bit(p2);
            for (uint64_t vq1 = empty; vq1; vq1 &= vq1 - 1) {
                const int q1 = dc_lowest(vq1);
                const uint64_t mid = I ^ dc_bit(p1) ^ dc_bit(q1);
                const int s1 = __popcll((unsigned long long)(I & dc_between(p1, q1)));
                for (uint64_t vq2 = vq1 & (vq1 - 1); vq2; vq2 &= vq2 - 1) {
                    const int q2 = dc_lowest(vq2);
                    const int64_t pos = dc_find(dets, a.dim, rest | dc_bit(q1) | dc_bit(q2));
                    if (pos < 0) continue;
                    const double* x = ut + (size_t)(((p1 * m + p2) * m + q1) * m + q2) * CW;
                    const bool minus = ((s1 + __popcll((unsigned long long)(mid & dc_between(p2, q2)))) & 1) != 0;
                    double e[CW];
#pragma unroll
                    for (int w = 0; w < CW; ++w) e[w] = minus ? -x[w] : x[w];
                    dc_feed<CW, G>(acc, e, a.c + pos * a.ldc * CW, a.ng);
                }
            }
        }
    }

#pragma unroll
    for (int g = 0; g < G; ++g) {
        if (g < a.ng) {
#pragma unroll
            for (int w = 0; w < CW; ++w) a.sigma[((int64_t)g * a.dim + row) * CW + w] = acc[g * CW + w];
        }
    }
}

template <int CW>
__global__ __launch_bounds__(kDcBlock) void det_ci_diagonal_kernel(const double* __restrict__ ht, const double* __restrict__ ut,
                                                                   const int64_t* __restrict__ dets, double* __restrict__ D,
                                                                   int m, int64_t dim) {
    const int64_t row = (int64_t)blockIdx.x * kDcBlock + threadIdx.x;
    if (row >= dim) return;
    const uint64_t I = (uint64_t)dets[row] & (dc_bit(m) - 1);
    double d = 0.0;
    for (uint64_t po = I; po; po &= po - 1) {
        const int p = dc_lowest(po);
        d += ht[(size_t)(p * m + p) * CW];
    }
    for (uint64_t po = I; po; po &= po - 1) {
        const int p = dc_lowest(po);
        for (uint64_t oq = po & (po - 1); oq; oq &= oq - 1) {
            const int q = dc_lowest(oq);
            d += ut[(size_t)(((p * m + q) * m + p) * m + q) * CW];
        }
    }
    D[row] = d;
}

// Close a 256-thread workgroup's sums: the xor butterfly inside each wave, lane 0 to LDS, then (dc_total, threads
// 0 ... CW - 1) the four waves in their fixed order.
template <int CW>
__device__ __forceinline__ void dc_close(double (&acc)[CW], double (&part)[kDcRhoBlock / 64][CW]) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int w = 0; w < CW; ++w) {
#pragma unroll
        for (int mask = 32; mask >= 1; mask >>= 1) acc[w] += __shfl_xor(acc[w], mask);
        if (lane == 0) part[wave][w] = acc[w];
    }
    __syncthreads();
}

template <int CW>
__device__ __forceinline__ double dc_total(const double (&part)[kDcRhoBlock / 64][CW], int w) {
    double s = part[0][w];
#pragma unroll
    for (int v = 1; v < kDcRhoBlock / 64; ++v) s += part[v][w];
    return s;
}

// One workgroup per (p, q) = (blockIdx / m, blockIdx % m): thread t takes determinants t, t + 256, ... as the bra
// determinant I (p in I, q not in I or q = p) and looks J = I - p + q up.  bra == ket is the density of one vector.
template <int CW>
__global__ __launch_bounds__(kDcRhoBlock) void det_ci_density1_kernel(const int64_t* __restrict__ dets, const double* bra,
                                                                      const double* ket, double* __restrict__ rho, int m,
                                                                      int64_t dim) {
    __shared__ double part[kDcRhoBlock / 64][CW];
    const int p = blockIdx.x / m, q = blockIdx.x % m;
    const int tid = threadIdx.x;
    const uint64_t between = dc_between(p, q);
    double acc[CW];
#pragma unroll
    for (int w = 0; w < CW; ++w) acc[w] = 0.0;
    for (int64_t i = tid; i < dim; i += kDcRhoBlock) {
        const uint64_t I = (uint64_t)dets[i];
        if (!(I & dc_bit(p))) continue;
        int64_t pos = i;
        if (p != q) {
            if (I & dc_bit(q)) continue;
            pos = dc_find(dets, dim, I ^ dc_bit(p) ^ dc_bit(q));
            if (pos < 0) continue;
        }
        const bool minus = (__popcll((unsigned long long)(I & between)) & 1) != 0;
        if constexpr (CW == 1) {
            const double b = minus ? -ket[pos] : ket[pos];
            acc[0] = fma(bra[i], b, acc[0]);
        } else {
            const double ar = bra[2 * i], ai = bra[2 * i + 1];
            const double br = minus ? -ket[2 * pos] : ket[2 * pos], bi = minus ? -ket[2 * pos + 1] : ket[2 * pos + 1];
            acc[0] = fma(ai, bi, fma(ar, br, acc[0]));                  // conj(a) b
            acc[CW - 1] = fma(-ai, br, fma(ar, bi, acc[CW - 1]));
        }
    }
    dc_close<CW>(acc, part);
    if (tid < CW) rho[(size_t)(q * m + p) * CW + tid] = dc_total<CW>(part, tid);
}

// (a, b) with a < b of the idx-th pair of m orbitals, pairs counted (0,1), (0,2), ..., (0,m-1), (1,2), ...
__device__ __forceinline__ void dc_pair(int idx, int m, int& a, int& b) {
    a = 0;
    while (idx >= m - 1 - a) {
        idx -= m - 1 - a;
        ++a;
    }
    b = a + 1 + idx;
}

// Two-body density.  One workgroup per unique quadruple (p < q, r < s) = pairs (blockIdx / npair, blockIdx % npair):
// thread t takes determinants t, t + 256, ... as the ket determinant J (r, s in J), applies a_r, a_s, a+_q, a+_p with
//   a_x |K> = (-1)^popcount(K & (2^x - 1)) |K - x>     (a+_x: the same sign on the state it fills)
// on the running mask (p, q may coincide with r, s), looks I = J - r - s + p + q up and adds conj(bra[I]) sign ket[J].
// The four copies gamma[pqrs] = -gamma[qprs] = -gamma[pqsr] = gamma[qpsr] come from one sum: the anti-symmetry is exact.
// Elements with p = q or r = s are not touched here: the entry zeroes the whole output first, on the same stream.
template <int CW>
__global__ __launch_bounds__(kDcRhoBlock) void det_ci_density2_kernel(const int64_t* __restrict__ dets, const double* bra,
                                                                      const double* ket, double* __restrict__ gamma2, int m,
                                                                      int npair, int64_t dim) {
    __shared__ double part[kDcRhoBlock / 64][CW];
    int p, q, r, s;
    dc_pair((int)(blockIdx.x / (unsigned)npair), m, p, q);
    dc_pair((int)(blockIdx.x % (unsigned)npair), m, r, s);
    const int tid = threadIdx.x;
    const uint64_t out_bits = dc_bit(r) | dc_bit(s), in_bits = dc_bit(p) | dc_bit(q);
    const uint64_t below_r = dc_bit(r) - 1, below_s = dc_bit(s) - 1, below_q = dc_bit(q) - 1, below_p = dc_bit(p) - 1;
    double acc[CW];
#pragma unroll
    for (int w = 0; w < CW; ++w) acc[w] = 0.0;
    for (int64_t i = tid; i < dim; i += kDcRhoBlock) {
        const uint64_t J = (uint64_t)dets[i];
        if ((J & out_bits) != out_bits) continue;
        const uint64_t J1 = J ^ dc_bit(r);                            // a_r |J>
        const uint64_t J2 = J1 ^ dc_bit(s);                           // a_s a_r |J>
        if (J2 & in_bits) continue;
        const uint64_t J3 = J2 | dc_bit(q);                           // a+_q a_s a_r |J>
        const int64_t pos = dc_find(dets, dim, J3 | dc_bit(p));
        if (pos < 0) continue;
        const int flips = __popcll((unsigned long long)(J & below_r)) + __popcll((unsigned long long)(J1 & below_s)) +
                          __popcll((unsigned long long)(J2 & below_q)) + __popcll((unsigned long long)(J3 & below_p));
        const bool minus = (flips & 1) != 0;
        if constexpr (CW == 1) {
            const double b = minus ? -ket[i] : ket[i];
            acc[0] = fma(bra[pos], b, acc[0]);
        } else {
            const double ar = bra[2 * pos], ai = bra[2 * pos + 1];
            const double br = minus ? -ket[2 * i] : ket[2 * i], bi = minus ? -ket[2 * i + 1] : ket[2 * i + 1];
            acc[0] = fma(ai, bi, fma(ar, br, acc[0]));                  // conj(a) b
            acc[CW - 1] = fma(-ai, br, fma(ar, bi, acc[CW - 1]));
        }
    }
    dc_close<CW>(acc, part);
    if (tid < CW) {
        const double v = dc_total<CW>(part, tid);
        const size_t mm = (size_t)m;
        gamma2[(((p * mm + q) * mm + r) * mm + s) * CW + tid] = v;
        gamma2[(((q * mm + p) * mm + r) * mm + s) * CW + tid] = -v;
        gamma2[(((p * mm + q) * mm + s) * mm + r) * CW + tid] = -v;
        gamma2[(((q * mm + p) * mm + s) * mm + r) * CW + tid] = v;
    }
}

// CW (doubles per element) of a dtype as a constant: f(std::integral_constant<int, CW>)
template <class F>
static auto dc_with_width(int dtype, F&& f) {
    return with_form(dtype == QS_F64 ? 0 : 1, [&](auto FORM) { return f(std::integral_constant<int, form_widths(FORM).aw>{}); });
}

// One group of a.ng vectors on the smallest instantiation that holds it.
template <int CW>
static void dc_launch(const DcArgs& a, hipStream_t s) {
    const unsigned grid = (unsigned)cdiv(a.dim, kDcBlock);
    with_group(a.ng, [&](auto G) {
        hipLaunchKernelGGL((det_ci_sigma_kernel<CW, G>), dim3(grid), dim3(kDcBlock), (size_t)a.m * a.m * CW * sizeof(double), s, a);
        note_dispatch("qs::det_ci_sigma_kernel<%d, %d>", CW, (int)G);
    });
}

// 0 = fp64, 1 = complex128, negative = the pair is refused
static inline int dc_form(int h_dtype, int c_dtype) {
    if (!dtype_ok(h_dtype) || !dtype_ok(c_dtype) || h_dtype != c_dtype) return QS_ERR_BAD_DTYPE;
    return h_dtype == QS_C128 ? 1 : 0;
}

static inline bool dc_extents_ok(int64_t m, int64_t N, int64_t dim, int64_t K) {
    return m >= 1 && m <= 63 && N >= 1 && N <= m && dim >= 1 && dim <= 0x7fffffffLL && K >= 1;
}

// The form's group size: the shipped one, or the tuning run's (det_ci_g = 1, 2, 4, 8).
static inline int dc_group(int form) { return group_size(g_tune.det_ci_g, kDcGroup[form]); }

// The checks the three density entries share, in the order of the other entries; out_elems elements of the form.
static int dc_density_refusal(int c_dtype, const int64_t* dets, const void* bra, const void* ket, const void* out,
                              int64_t out_elems, int64_t m, int64_t N, int64_t dim) {
    if (!dtype_ok(c_dtype)) return QS_ERR_BAD_DTYPE;
    if (!dc_extents_ok(m, N, dim, 1)) return QS_ERR_BAD_EXTENT;
    if (!dets || !bra || !ket || !out) return QS_ERR_NULL_POINTER;
    const int64_t es = (int64_t)elem_size(c_dtype);
    if (!aligned(dets, 8) || !aligned(bra, (size_t)es) || !aligned(ket, (size_t)es) || !aligned(out, (size_t)es))
        return QS_ERR_MISALIGNED;
    if (overlaps(out, out_elems * es, dets, dim * 8) || overlaps(out, out_elems * es, bra, dim * es) ||
        overlaps(out, out_elems * es, ket, dim * es))
        return QS_ERR_ALIAS;
    return QS_OK;
}

static int dc_density1(int c_dtype, const int64_t* dets, const void* bra, const void* ket, void* rho, int64_t m, int64_t N,
                       int64_t dim, void* stream) {
    dispatch_reset();
    const int rc = dc_density_refusal(c_dtype, dets, bra, ket, rho, m * m, m, N, dim);
    if (rc) return rc;
    const unsigned grid = (unsigned)(m * m);
    hipStream_t s = (hipStream_t)stream;
    dc_with_width(c_dtype, [&](auto CW) {
        hipLaunchKernelGGL((det_ci_density1_kernel<CW>), dim3(grid), dim3(kDcRhoBlock), 0, s, dets, (const double*)bra, (const double*)ket, (double*)rho, (int)m, dim);
        note_dispatch("qs::det_ci_density1_kernel<%d>", (int)CW);
    });
    return launch_status("determinant CI density launch");
}

}  // namespace qs

using namespace qs;

extern "C" {

int64_t qs_det_ci_workspace(int h_dtype, int c_dtype, int64_t m, int64_t N, int64_t dim, int64_t K) {
    const int form = dc_form(h_dtype, c_dtype);
    if (form < 0) return form;
    if (!dc_extents_ok(m, N, dim, K)) return QS_ERR_BAD_EXTENT;
    return 0;          // every sum is closed inside its thread
}

int qs_det_ci_diagonal(int h_dtype, const void* ht, const void* ut, const int64_t* dets, double* D, int64_t m, int64_t N,
                       int64_t dim, void* stream) {
    dispatch_reset();
    if (!dtype_ok(h_dtype)) return QS_ERR_BAD_DTYPE;
    if (!dc_extents_ok(m, N, dim, 1)) return QS_ERR_BAD_EXTENT;
    if (!ht || !ut || !dets || !D) return QS_ERR_NULL_POINTER;
    const int64_t es = (int64_t)elem_size(h_dtype);
    if (!aligned(ht, (size_t)es) || !aligned(ut, (size_t)es) || !aligned(dets, 8) || !aligned(D, 8)) return QS_ERR_MISALIGNED;
    const int64_t d_bytes = dim * 8;
    if (overlaps(D, d_bytes, ht, m * m * es) || overlaps(D, d_bytes, ut, m * m * m * m * es) ||
        overlaps(D, d_bytes, dets, dim * 8))
        return QS_ERR_ALIAS;
    const unsigned grid = (unsigned)cdiv(dim, kDcBlock);
    hipStream_t s = (hipStream_t)stream;
    dc_with_width(h_dtype, [&](auto CW) {
        hipLaunchKernelGGL((det_ci_diagonal_kernel<CW>), dim3(grid), dim3(kDcBlock), 0, s, (const double*)ht, (const double*)ut, dets, D, (int)m, dim);
        note_dispatch("qs::det_ci_diagonal_kernel<%d>", (int)CW);
    });
    return launch_status("determinant CI diagonal launch");
}

int qs_det_ci_sigma(int h_dtype, int c_dtype, const void* ht, const void* ut, const int64_t* dets, const double* D,
                    const void* c, void* sigma, int64_t m, int64_t N, int64_t dim, int64_t K, int64_t ldc, void* work,
                    int64_t work_elems, void* stream) {
    dispatch_reset();
    (void)work;
    const int form = dc_form(h_dtype, c_dtype);
    if (form < 0) return form;
    if (!dc_extents_ok(m, N, dim, K) || ldc < K) return QS_ERR_BAD_EXTENT;
    if (!ht || !ut || !dets || !D || !c || !sigma) return QS_ERR_NULL_POINTER;
    const int64_t es = (int64_t)elem_size(c_dtype);
    if (!aligned(ht, (size_t)es) || !aligned(ut, (size_t)es) || !aligned(dets, 8) || !aligned(D, 8) || !aligned(c, (size_t)es) ||
        !aligned(sigma, (size_t)es))
        return QS_ERR_MISALIGNED;
    const int64_t s_bytes = K * dim * es;
    if (overlaps(sigma, s_bytes, ht, m * m * es) || overlaps(sigma, s_bytes, ut, m * m * m * m * es) ||
        overlaps(sigma, s_bytes, dets, dim * 8) || overlaps(sigma, s_bytes, D, dim * 8) ||
        overlaps(sigma, s_bytes, c, ((dim - 1) * ldc + K) * es))
        return QS_ERR_ALIAS;
    if (work_elems < qs_det_ci_workspace(h_dtype, c_dtype, m, N, dim, K)) return QS_ERR_WORKSPACE;

    const int cw = form_widths(form).aw;
    DcArgs a{};
    a.ht = (const double*)ht; a.ut = (const double*)ut; a.dets = dets; a.D = D;
    a.dim = dim; a.ldc = ldc; a.m = (int)m;
    hipStream_t s = (hipStream_t)stream;
    return for_each_group(K, dc_group(form), [&](int64_t k0, int ng) {
        a.ng = ng;
        a.c = (const double*)c + k0 * cw;
        a.sigma = (double*)sigma + k0 * dim * cw;
        dc_with_width(c_dtype, [&](auto CW) { dc_launch<CW>(a, s); });
        return launch_status("determinant CI sigma launch");
    });
}

int qs_det_ci_density1(int c_dtype, const int64_t* dets, const void* c, void* rho, int64_t m, int64_t N, int64_t dim,
                       void* stream) {
    return dc_density1(c_dtype, dets, c, c, rho, m, N, dim, stream);
}

int qs_det_ci_transition_density1(int c_dtype, const int64_t* dets, const void* bra, const void* ket, void* rho, int64_t m,
                                  int64_t N, int64_t dim, void* stream) {
    return dc_density1(c_dtype, dets, bra, ket, rho, m, N, dim, stream);
}

int qs_det_ci_density2(int c_dtype, const int64_t* dets, const void* bra, const void* ket, void* gamma2, int64_t m, int64_t N,
                       int64_t dim, void* stream) {
    dispatch_reset();
    const int64_t elems = m * m * m * m;
    int rc = dc_density_refusal(c_dtype, dets, bra, ket, gamma2, elems, m, N, dim);
    if (rc) return rc;
    hipStream_t s = (hipStream_t)stream;
    // the elements with p = q or r = s (all of them at N = 1 or m = 1) are exact zeros
    rc = hip_status(hipMemsetAsync(gamma2, 0, (size_t)elems * elem_size(c_dtype), s), "determinant CI two-body density fill");
    if (rc || N < 2) return rc;
    const int64_t npair = m * (m - 1) / 2;                             // <= 1953: the grid is at most 3 814 209
    const unsigned grid = (unsigned)(npair * npair);
    dc_with_width(c_dtype, [&](auto CW) {
        hipLaunchKernelGGL((det_ci_density2_kernel<CW>), dim3(grid), dim3(kDcRhoBlock), 0, s, dets, (const double*)bra, (const double*)ket, (double*)gamma2, (int)m, (int)npair, dim);
        note_dispatch("qs::det_ci_density2_kernel<%d>", (int)CW);
    });
    return launch_status("determinant CI two-body density launch");
}

}  // extern "C"
