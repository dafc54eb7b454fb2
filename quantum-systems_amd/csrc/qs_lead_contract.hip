// Leading-index contraction with a few rows, and the per-index four-index transform built on it.
//
//   T[i, x] = sum_a A[i, a] * B[a, x]        1 <= m <= 32 rows i, any k, any n, B row-major with ldb >= n
//
// is the first step of a transform to an orbital BLOCK (a handful of occupied orbitals against the L x L^3 tensor):
// about 2 m flop per 8-byte element of B, i.e. one read of B at HBM rate and nothing else.  Streaming VALU kernel in the
// spirit of qs_mean_field.hip: a lane owns ONE 16-byte item of x (two fp64 columns, or one complex element) and keeps
// the R running sums of its item in registers (R = 4 / 8 / 16 / 32 rows, zero rows of A as padding); it streams
// a = 0 ... k-1 with kLcDepth rows of B in flight -- row a + kLcDepth is issued before the FMAs of row a.  A is
// wave-uniform: staged in LDS once per workgroup ([a][R], zero padded; chunks of a when it does not fit 64 KB) and read
// as broadcasts.  No split over a, no cross-lane reduction, no atomics, no workspace: every output element is one fma
// chain over ascending a in one lane, so row i of an m-row call has the bits of the 1-row call on that row, and column x
// depends neither on n nor on the grid.
//
// Global items are raw buffer loads (qs_fast_items.h): scalar base of (block, row a), range = what is left of B from
// there, so nothing outside B is fetched (rows a >= k of the software pipeline's tail come back as zeros without a
// fetch).  16-byte items at 8-byte-aligned addresses for odd n / ldb; the last item of an odd-n row straddles into the
// next row (or into the surplus columns of a wider buffer): that half is dropped with a select, never multiplied.

#include "qs_contract_common.h"

namespace qs {

constexpr int kLcDepth = 8;                    // rows of B in flight per lane
constexpr unsigned kLcRoom = 1u << 30;         // cap of a buffer range in bytes = the offset of a lane that must not fetch
constexpr int64_t kLcLdsBytes = 64 * 1024;     // LDS of one workgroup for the rows of A

struct LcArgs {
    const double* A;
    const double* B;
    double* T;
    int64_t n, lda, ldb, ldt;
    int m, k, kc;               // kc: rows a per LDS chunk (a multiple of kLcDepth)
};

// FORM 0: A, B, T real; 1: all complex128; 2: real B, complex A and T (two real accumulations per element of B).
template <int FORM, int R>
__global__ __launch_bounds__(256) void lead_contract_kernel(const LcArgs g) {
    constexpr auto W = form_widths(FORM);      // B is the tensor, A the coefficients
    constexpr int BW = W.uw, AW = W.aw, CPI = W.cpi;
    constexpr int NACC = FORM == 2 ? 4 : 2;    // running sums (doubles) per row
    constexpr int D = kLcDepth;
    extern __shared__ __attribute__((aligned(16))) double lc_lds[];     // [kc][R][AW]

    const int tid = threadIdx.x, k = g.k;
    const int64_t xb = (int64_t)blockIdx.x * (256 * CPI), x0 = xb + (int64_t)tid * CPI;
    const bool colok = x0 < g.n, full = x0 + 1 < g.n;
    const unsigned off = colok ? (unsigned)tid * 16u : kLcRoom;
    const uint64_t row_bytes = (uint64_t)g.ldb * (BW * 8);
    const uint64_t b0 = uniform64(reinterpret_cast<uint64_t>(g.B) + (uint64_t)xb * (BW * 8));
    const uint64_t bend = uniform64(reinterpret_cast<uint64_t>(g.B) + ((uint64_t)(k - 1) * g.ldb + g.n) * (BW * 8));

    auto fetch = [&](int a) {
        const uint64_t base = b0 + (uint64_t)a * row_bytes;
        const unsigned left = bytes_left(bend, base);
        return FastItem<true>::load(base, left < kLcRoom ? left : kLcRoom, off);
    };

    double acc[R][NACC];
#pragma unroll
    for (int i = 0; i < R; ++i)
#pragma unroll
        for (int w = 0; w < NACC; ++w) acc[i][w] = 0.0;

    f64x2 ring[D];
#pragma unroll
    for (int j = 0; j < D; ++j) ring[j] = fetch(j);

    const int kpad = (k + D - 1) / D * D;
    for (int c0 = 0; c0 < kpad; c0 += g.kc) {
        const int cn = kpad - c0 < g.kc ? kpad - c0 : g.kc;
        if (c0) __syncthreads();
        for (int idx = tid; idx < cn * R; idx += 256) {
            const int i = idx % R, a = c0 + idx / R;
            const bool ok = i < g.m && a < k;
#pragma unroll
            for (int w = 0; w < AW; ++w) lc_lds[(size_t)idx * AW + w] = ok ? g.A[((int64_t)i * g.lda + a) * AW + w] : 0.0;
        }
        __syncthreads();

        for (int a0 = 0; a0 < cn; a0 += D) {
#pragma unroll
            for (int j = 0; j < D; ++j) {
                f64x2 v = ring[j];
                ring[j] = fetch(c0 + a0 + j + D);
                if (FORM != 1 && !full) v.y = 0.0;            // odd n: the item's second half is not this row's
                const double* ar = lc_lds + (size_t)(a0 + j) * (R * AW);
#pragma unroll
                for (int i = 0; i < R; ++i) {
                    if (FORM == 0) {
                        const double c = ar[i];
                        acc[i][0] = __builtin_fma(c, v.x, acc[i][0]);
                        acc[i][1] = __builtin_fma(c, v.y, acc[i][1]);
                    } else if (FORM == 1) {
                        const double cr = ar[2 * i], ci = ar[2 * i + 1];
                        acc[i][0] = __builtin_fma(-ci, v.y, __builtin_fma(cr, v.x, acc[i][0]));
                        acc[i][1] = __builtin_fma(ci, v.x, __builtin_fma(cr, v.y, acc[i][1]));
                    } else {
                        const double cr = ar[2 * i], ci = ar[2 * i + 1];
                        acc[i][0] = __builtin_fma(cr, v.x, acc[i][0]);
                        acc[i][1] = __builtin_fma(ci, v.x, acc[i][1]);
                        acc[i][NACC - 2] = __builtin_fma(cr, v.y, acc[i][NACC - 2]);
                        acc[i][NACC - 1] = __builtin_fma(ci, v.y, acc[i][NACC - 1]);
                    }
                }
            }
        }
    }

    if (!colok) return;
#pragma unroll
    for (int i = 0; i < R; ++i) {
        if (i >= g.m) continue;
        double* t = g.T + ((int64_t)i * g.ldt + x0) * AW;
        if (FORM == 1 || (FORM == 0 && full && (reinterpret_cast<uintptr_t>(t) & 15) == 0)) {
            f64x2 o;
            o.x = acc[i][0]; o.y = acc[i][1];
            *reinterpret_cast<f64x2*>(t) = o;
        } else if (FORM == 0) {
            t[0] = acc[i][0];
            if (full) t[1] = acc[i][1];
        } else {
            f64x2 o;
            o.x = acc[i][0]; o.y = acc[i][1];
            *reinterpret_cast<f64x2*>(t) = o;
            if (full) {
                o.x = acc[i][NACC - 2]; o.y = acc[i][NACC - 1];
                *reinterpret_cast<f64x2*>(t + 2) = o;
            }
        }
    }
}

template <int FORM, int R>
static int lc_launch(LcArgs g, hipStream_t s) {
    constexpr int AW = form_widths(FORM).aw, CPI = form_widths(FORM).cpi;
    const int64_t kpad = cdiv(g.k, kLcDepth) * kLcDepth;
    const int64_t fit = kLcLdsBytes / (R * AW * 8) / kLcDepth * kLcDepth;
    g.kc = (int)(kpad < fit ? kpad : fit);
    const int64_t grid = cdiv(cdiv(g.n, CPI), 256);         // from n only
    if (grid > INT32_MAX) return QS_ERR_BAD_EXTENT;
    hipLaunchKernelGGL((lead_contract_kernel<FORM, R>), dim3((unsigned)grid), dim3(256), (size_t)g.kc * R * AW * 8, s, g);
    note_dispatch("qs::lead_contract_kernel<%d, %d>", FORM, R);
    return launch_status("lead contraction launch");
}

template <int FORM>
static int lc_rows(const LcArgs& g, hipStream_t s) {
    if (g.m <= 4) return lc_launch<FORM, 4>(g, s);
    if (g.m <= 8) return lc_launch<FORM, 8>(g, s);
    if (g.m <= 16) return lc_launch<FORM, 16>(g, s);
    return lc_launch<FORM, 32>(g, s);
}

// the arguments as the entry validated them
static int lead_contract(int form, const void* A, const void* B, void* T, int64_t m, int64_t n, int64_t k, int64_t lda,
                         int64_t ldb, int64_t ldt, hipStream_t s) {
    LcArgs g{(const double*)A, (const double*)B, (double*)T, n, lda, ldb, ldt, (int)m, (int)k, 0};
    return with_form(form, [&](auto F) { return lc_rows<F>(g, s); });
}

// Complex A (m x k) against a REAL B through the tiled products (the rows beyond the lead kernel): the real product
// [Re A; Im A] (2m x k) . B panel -> planar rows, interleaved into T by a copy kernel.  `planar` holds 2m x w doubles.
__global__ __launch_bounds__(256) void lc_split_kernel(const double* __restrict__ A, double* __restrict__ P, int m, int k) {
    const int idx = blockIdx.x * 256 + threadIdx.x;
    if (idx >= m * k * 2) return;
    const int w = idx & 1, e = idx >> 1, i = e / k, a = e - i * k;
    P[(size_t)(2 * i + w) * k + a] = A[idx];
}

__global__ __launch_bounds__(256) void lc_interleave_kernel(const double* __restrict__ P, double* __restrict__ T, int m,
                                                            int64_t w, int64_t ldt) {
    const int64_t x = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (x >= w) return;
    for (int i = 0; i < m; ++i) {
        f64x2 o;
        o.x = P[(size_t)(2 * i) * w + x]; o.y = P[(size_t)(2 * i + 1) * w + x];
        *reinterpret_cast<f64x2*>(T + ((int64_t)i * ldt + x) * 2) = o;
    }
}

static inline int64_t even_up(int64_t x) { return (x + 1) & ~int64_t(1); }
static inline char* at(void* base, int64_t elems, size_t es) { return (char*)base + (size_t)elems * es; }

static inline bool blocks_extents_ok(int64_t L, int64_t M0, int64_t M1, int64_t M2, int64_t M3) {
    return extents_ok(L, 1) && M0 >= 1 && M0 <= L && M1 >= 1 && M1 <= L && M2 >= 1 && M2 <= L && M3 >= 1 && M3 <= L;
}

}  // namespace qs

using namespace qs;

extern "C" {

int qs_lead_contract(int a_dtype, int b_dtype, const void* A, const void* B, void* T, int64_t m, int64_t n, int64_t k,
                     int64_t lda, int64_t ldb, int64_t ldt, void* stream) {
    dispatch_reset();
    const int form = tensor_form(b_dtype, a_dtype);
    if (form < 0) return form;
    if (m < 1 || m > 32 || n < 1 || k < 1 || k > INT32_MAX || lda < k || ldb < n || ldt < n) return QS_ERR_BAD_EXTENT;
    if (!A || !B || !T) return QS_ERR_NULL_POINTER;
    const int64_t aes = (int64_t)elem_size(a_dtype), bes = (int64_t)elem_size(b_dtype);
    if (!aligned(A, (size_t)aes) || !aligned(B, (size_t)bes) || !aligned(T, (size_t)aes)) return QS_ERR_MISALIGNED;
    const int64_t tb = ((m - 1) * ldt + n) * aes;
    if (overlaps(T, tb, A, ((m - 1) * lda + k) * aes) || overlaps(T, tb, B, ((k - 1) * ldb + n) * bes)) return QS_ERR_ALIAS;
    return lead_contract(form, A, B, T, m, n, k, lda, ldb, ldt, (hipStream_t)stream);
}

int64_t qs_transform_two_body_blocks_workspace(int u_dtype, int c_dtype, int64_t L, int64_t M0, int64_t M1, int64_t M2,
                                               int64_t M3) {
    const int form = tensor_form(u_dtype, c_dtype);
    if (form < 0) return form;
    if (!blocks_extents_ok(L, M0, M1, M2, M3)) return QS_ERR_BAD_EXTENT;
    return (even_up(L * (M0 + M2)) + M0 * L * L * L + M0 * M1 * L * L) * (int64_t)elem_size(c_dtype);
}

int qs_transform_two_body_blocks(int u_dtype, int c_dtype, const void* u, const void* Ct0, const void* Ct1,
                                 const void* C2, const void* C3, void* out, void* work, int64_t work_bytes, int64_t L,
                                 int64_t M0, int64_t M1, int64_t M2, int64_t M3, void* stream) {
    dispatch_reset();
    const int form = tensor_form(u_dtype, c_dtype);
    if (form < 0) return form;
    if (!blocks_extents_ok(L, M0, M1, M2, M3)) return QS_ERR_BAD_EXTENT;
    if (!u || !Ct0 || !Ct1 || !C2 || !C3 || !out || !work) return QS_ERR_NULL_POINTER;
    const size_t es = elem_size(c_dtype), ues = elem_size(u_dtype);
    if (!aligned(u, ues) || !aligned(Ct0, es) || !aligned(Ct1, es) || !aligned(C2, es) || !aligned(C3, es) ||
        !aligned(out, es) || !aligned(work, 16))
        return QS_ERR_MISALIGNED;
    const int64_t need = qs_transform_two_body_blocks_workspace(u_dtype, c_dtype, L, M0, M1, M2, M3);
    const int64_t ob = M0 * M1 * M2 * M3 * (int64_t)es, L3 = L * L * L;
    if (overlaps(out, ob, u, L3 * L * (int64_t)ues) || overlaps(out, ob, work, need) ||
        overlaps(work, need, u, L3 * L * (int64_t)ues) || overlaps(out, ob, Ct0, M0 * L * (int64_t)es) ||
        overlaps(out, ob, Ct1, M1 * L * (int64_t)es) || overlaps(out, ob, C2, L * M2 * (int64_t)es) ||
        overlaps(out, ob, C3, L * M3 * (int64_t)es))
        return QS_ERR_ALIAS;
    if (work_bytes < need) return QS_ERR_WORKSPACE;
    hipStream_t s = (hipStream_t)stream;

    // T1 (M0, L, L, L) -> T2 (M0, M1, L, L) -> T3 (M0, M1, L, M3) in T1's place (M1 M3 <= L^2) -> out
    void* C2T = work;                       // (M2, L), then M0 L elements for the split rows of Ct0 (mixed form)
    void* T1 = at(work, even_up(L * (M0 + M2)), es);
    void* T2 = at(T1, M0 * L3, es);
    void* T3 = T1;

    // a: the leading index, one read of u
    int rc;
    if (M0 <= g_tune.lead_rows_max) {
        rc = lead_contract(form, Ct0, u, T1, M0, L3, L, L, L3, L3, s);
    } else if (form != 2) {
        // (n = L^3 when it fits 32 bits, else one product per second index)
        rc = L <= 1024 ? gemm(packed(c_dtype, Ct0, u, T1, M0, L3, L), s)
                       : gemm(Product{c_dtype, (const double*)Ct0, (const double*)u, (double*)T1, M0, L * L, L, L, L3, L3,
                                      L, 0, L * L, L * L, 0}, s);
    } else {
        // real u, complex rows: the real product [Re Ct0; Im Ct0] . u on panels of up to M1 second indices, planar in
        // T2's place (2 M0 x w doubles, w <= M1 L^2), interleaved into T1
        double* split = (double*)at(C2T, L * M2, es);
        const int64_t slices = M1 * L * L <= INT32_MAX ? M1 : 1;
        hipLaunchKernelGGL(lc_split_kernel, dim3((unsigned)cdiv(M0 * L * 2, 256)), dim3(256), 0, s, (const double*)Ct0,
                           split, (int)M0, (int)L);
        note_dispatch("qs::lc_split_kernel");
        rc = launch_status("coefficient split launch");
        for (int64_t b0 = 0; !rc && b0 < L; b0 += slices) {
            const int64_t w = (L - b0 < slices ? L - b0 : slices) * L * L;
            rc = gemm(Product{QS_F64, split, (const double*)u + b0 * L * L, (double*)T2, 2 * M0, w, L, L, L3, w, 1, 0, 0, 0, 0}, s);
            if (rc) break;
            hipLaunchKernelGGL(lc_interleave_kernel, dim3((unsigned)cdiv(w, 256)), dim3(256), 0, s, (const double*)T2,
                               (double*)T1 + b0 * L * L * 2, (int)M0, w, L3);
            note_dispatch("qs::lc_interleave_kernel");
            rc = launch_status("interleave launch");
        }
    }
    if (rc) return rc;
    // b: T2[p] (M1 x L^2) = Ct1 . T1[p] (L x L^2)
    rc = gemm(packed(c_dtype, Ct1, T1, T2, M1, L * L, L, M0), s);
    if (rc) return rc;
    // d: T3 (M0 M1 L x M3) = T2 (M0 M1 L x L) . C3
    rc = gemm(packed(c_dtype, T2, C3, T3, M0 * M1 * L, M3, L), s);
    if (rc) return rc;
    // c: out[pq] (M2 x M3) = C2^T . T3[pq] (L x M3)
    rc = transpose_small(c_dtype, C2, C2T, L, M2, s);
    if (rc) return rc;
    return gemm(packed(c_dtype, C2T, T3, out, M2, M3, L, M0 * M1), s);
}

}  // extern "C"
