// Spin-free configuration interaction on alpha and beta occupation strings (Knowles-Handy): H c with the two-body part
// as ONE dense product on the library's product dispatcher.
//   H = sum_pr k[p,r] E_pr + sum_(pr),(qs) W[(pr),(qs)] E_pr E_qs,      E_pq = sum_spin a+_p,spin a_q,spin
//   k[p,r] = ht[p,r] - 1/2 sum_q ut[p,q,q,r],      W[(pr),(qs)] = 1/2 ut[p,q,r,s]   (ut = <pq|rs>, NOT anti-symmetrised)
// A state is c[Ia, Ib] (Ib fastest) over a list of na alpha and a list of nb beta strings: ascending 64-bit masks over
// m <= 63 SPATIAL orbitals; the determinant is all alpha creators first, ascending within each spin, so E_pq acts on one
// string at a time with that string's own sign.  The lists are data: a replacement whose target is missing contributes
// nothing.
//
// The replacement table of a list is T[K, p * m + q] (int32): +-(index of J + 1) where <K|E_pq|J> = +-1, i.e.
// J = K - p + q with p in K and q not in K or q = p, sign (-1)^(bits of K strictly between p and q); 0 where the
// replacement is empty or its target is not in the list.  It is the only place a string is searched for.
//
// One sigma per group of K vectors, three steps, no atomics:
//   expand : D[(qs), k, Ka, Kb] = (E_qs c_k)[Ka, Kb] = sgn c_k[Ta[Ka,qs], Kb] + sgn c_k[Ka, Tb[Kb,qs]]     (m^2 x K dim)
//   product: G = W . D                                                            gemm(Product{...}), qs_gemm.hip
//   fold   : sigma_k[Ia, Ib] = sum_pr ( sgn X[(pr), k, Ta[Ia,pr], Ib] + sgn X[(pr), k, Ia, Tb[Ib,pr]] ),
//            X[(pr), k, K] = G[(pr), k, K] + k[p,r] c_k[K]
// expand and fold are streams of m^2 K dim elements.  A workgroup owns one alpha string Ia and a tile of up to 256
// consecutive beta strings, thread t the string Ib = tile + t: the alpha part reads and writes whole contiguous rows,
// and its table entry Ta[Ia, pq] has a wave-uniform address (Ia comes from the workgroup's index, pq from the loop
// counter), so it is a scalar load.  The beta part gathers inside the one row c[Ia, :] of nb elements; its table
// entries are staged through LDS in chunks of 16 columns, read from T row-wise (64 contiguous bytes per string) and
// stored column-wise, so that a lane reads its own entry without a bank conflict.
// The fold's sum has a fixed order -- pr ascending, alpha before beta, every product an explicit fma --, skips the
// table's zeros, and never sees another vector: repeating a call gives the same bits.  (The PRODUCT is chosen by its
// extents, so sigma_k alone and sigma_k in a batch agree to rounding, not bit for bit.)
// A table entry that points at or past the end of its list is treated as 0: a wrong table gives wrong numbers, never
// an access outside the arguments.

#include <initializer_list>

#include "qs_contract_common.h"
#include "qs_strings.h"

namespace qs {

constexpr int kScChunk = 16;          // table columns staged per step
constexpr int kScBlock = 256;         // most beta strings (threads) of a workgroup; 64 or 128 for shorter lists
constexpr int kScRhoBlock = 256;      // threads of the density's and of the diagonal's workgroup
// Shipped byte budget of the D and G of one qs_string_ci_sigma call: qs_string_ci_group() splits a batch by it when
// the caller passes 0 (kernels.STRING_CI_BYTES passes its own).  Not measured yet.  Also the budget of
// the two panels of one pass of qs_string_ci_density2 and of qs_string_ci_density2_spin (3.13), and of
// the D_p and G_p of one pass of qs_string_ci_sigma_rows and of qs_string_ci_sigma_sym (3.12).
constexpr int64_t kScBytes = int64_t(2) << 30;

struct ScArgs {
    const int32_t* ta;        // (na, m^2); the kernels read it through an argument of their own (string_ci_expand_kernel)
    const int32_t* tb;        // (nb, m^2)
    const double* c;          // (K, na, nb)
    const double* kk;         // (m, m), fold only
    const double* G;          // the panel G_p of the pass, (m^2, K, pdim), fold only
    double* out;              // sigma (K, na, nb); the fold writes it through an argument of its own
    int64_t na, nb;
    unsigned ntile;           // tiles of blockDim.x beta strings
    int m2, K;
};

// The workgroup's chunk of the beta table, columns pq0 ... pq0 + 15 of its strings: sc_tb[j][r] = Tb[ib0 + r, pq0 + j].
__device__ __forceinline__ void sc_stage(int32_t* sc_tb, const int32_t* __restrict__ tb, int64_t ib0, int64_t nb, int pq0,
                                         int m2) {
    const int B = blockDim.x;
    for (int idx = threadIdx.x; idx < B * kScChunk; idx += B) {
        const int r = idx / kScChunk, j = idx % kScChunk;
        const int64_t row = ib0 + r;
        const int pq = pq0 + j;
        sc_tb[j * (B + 1) + r] = (row < nb && pq < m2) ? tb[row * m2 + pq] : 0;
    }
}

// index behind a table entry e != 0, or -1 when it points past the n strings of the list
__device__ __forceinline__ int64_t sc_target(int32_t e, int64_t n) {
    const int64_t j = (int64_t)(e < 0 ? -e : e) - 1;
    return j < n ? j : -1;
}

// (E_pq c)[Ia, Ib] from the two table entries of (Ia, pq) and (Ib, pq)
template <int CW>
__device__ __forceinline__ void sc_replaced(double (&v)[CW], const double* __restrict__ c, int32_t ea, int32_t eb, int64_t ia,
                                            int64_t ib, int64_t na, int64_t nb) {
    const int64_t ja = ea ? sc_target(ea, na) : -1, jb = eb ? sc_target(eb, nb) : -1;
#pragma unroll
    for (int w = 0; w < CW; ++w) v[w] = 0.0;
    if (ja >= 0) {
        const double* x = c + (ja * nb + ib) * CW;
#pragma unroll
        for (int w = 0; w < CW; ++w) v[w] = ea < 0 ? -x[w] : x[w];
    }
    if (jb >= 0) {
        const double* x = c + (ia * nb + jb) * CW;
#pragma unroll
        for (int w = 0; w < CW; ++w) v[w] += eb < 0 ? -x[w] : x[w];
    }
}

// (E^s_pq c)[Ia, Ib] of ONE spin, E^s_pq = a+_ps a_qs, from its table entry e: a signed copy, or 0.  Not sc_replaced with the
// other entry 0: its 0.0 + (-0.0) is +0.0, and this value keeps the sign of a zero.
template <int CW>
__device__ __forceinline__ void sc_replaced_spin(double (&v)[CW], const double* __restrict__ c, int32_t e, bool beta, int64_t ia,
                                                 int64_t ib, int64_t na, int64_t nb) {
    const int64_t jt = e ? sc_target(e, beta ? nb : na) : -1;
#pragma unroll
    for (int w = 0; w < CW; ++w) v[w] = 0.0;
    if (jt >= 0) {
        const double* x = c + (beta ? ia * nb + jt : jt * nb + ib) * CW;
#pragma unroll
        for (int w = 0; w < CW; ++w) v[w] = e < 0 ? -x[w] : x[w];
    }
}

// ---- the panel of one pass -----------------------------------------------------------------------------------------------
// A pass owns the alpha rows r0 <= Ka < r1 of D and G; c and sigma stay whole.  A layout says where the element (Ka, Kb) of
// such a row lies in the panel of one (qs) and vector, which elements are stored at all, and which of them carry the weight
// 1/2 in the fold; expand and fold below are written once over it.
//   ScRect: every column, D_p[(qs), k, Ka - r0, Kb], panel stride (r1 - r0) nb.  One pass [0, na) is qs_string_ci_sigma, passes
//           of equal length are qs_string_ci_sigma_rows.
//   ScTri : the columns Kb <= Ka of a packed row at off(Ka) = Ka (Ka + 1) / 2, off(r1) - off(r0) elements per (qs) and
//           vector (qs_string_ci_sigma_sym, below).

__host__ __device__ __forceinline__ int64_t sc_off(int64_t r) { return r * (r + 1) / 2; }

struct ScRect {
    static constexpr bool kPacked = false;
    int64_t r0, r1, nb;
    __host__ __device__ int64_t pdim() const { return (r1 - r0) * nb; }
    __device__ int64_t at(int64_t row, int64_t col) const { return (row - r0) * nb + col; }
    __device__ bool tile(int64_t, int64_t) const { return true; }        // the tile that starts at col0 holds a stored column
    __device__ bool holds(int64_t, int64_t) const { return true; }
    __device__ bool diagonal(int64_t, int64_t) const { return false; }
};

struct ScTri {
    static constexpr bool kPacked = true;
    int64_t r0, r1, nb;
    __host__ __device__ int64_t pdim() const { return sc_off(r1) - sc_off(r0); }
    __device__ int64_t at(int64_t row, int64_t col) const { return sc_off(row) - sc_off(r0) + col; }
    __device__ bool tile(int64_t row, int64_t col0) const { return col0 <= row; }
    __device__ bool holds(int64_t row, int64_t col) const { return col <= row; }
    __device__ bool diagonal(int64_t row, int64_t col) const { return col == row; }
};

// D_p = expand(c) on the rows of the pass: one workgroup per alpha string of the pass and tile of beta strings.  c is the
// whole vector: the targets lie anywhere.
template <int CW, class Layout>
__global__ __launch_bounds__(kScBlock) void string_ci_expand_kernel(const ScArgs a, const int32_t* __restrict__ ta,
                                                                   double* __restrict__ D, const Layout lay) {
    // ta and D are kernel arguments of their own: only there does __restrict__ tell the compiler that the stores of D
    // cannot change the table, which lets the uniform read below be a scalar load
    extern __shared__ __attribute__((aligned(16))) int32_t sc_tb[];
    const int B = blockDim.x, t = threadIdx.x, m2 = a.m2;
    const int64_t ia = lay.r0 + blockIdx.x / a.ntile;                     // uniform
    const int64_t ib0 = (int64_t)(blockIdx.x % a.ntile) * B;
    if (!lay.tile(ia, ib0)) return;                                       // uniform: the tile lies above the diagonal
    const int64_t ib = ib0 + t, nb = a.nb, dim = a.na * a.nb, pdim = lay.pdim();
    const bool live = ib < nb && lay.holds(ia, ib);                       // the others only stage
    const int64_t at = lay.at(ia, ib);
    const int32_t* __restrict__ ta_row = ta + ia * m2;
    const double* __restrict__ c = a.c;
    for (int pq0 = 0; pq0 < m2; pq0 += kScChunk) {
        __syncthreads();
        sc_stage(sc_tb, a.tb, ib0, nb, pq0, m2);
        __syncthreads();
        if (!live) continue;
        const int nj = m2 - pq0 < kScChunk ? m2 - pq0 : kScChunk;
        for (int j = 0; j < nj; ++j) {
            const int pq = pq0 + j;
            const int32_t ea = ta_row[pq];                                // uniform address: a scalar load
            const int32_t eb = sc_tb[j * (B + 1) + t];
            for (int k = 0; k < a.K; ++k) {
                double v[CW];
                sc_replaced<CW>(v, c + (int64_t)k * dim * CW, ea, eb, ia, ib, a.na, nb);
                double* d = D + (((int64_t)pq * a.K + k) * pdim + at) * CW;
#pragma unroll
                for (int w = 0; w < CW; ++w) d[w] = v[w];
            }
        }
    }
}

// acc += s (g + kk c) at one element: HW doubles per element of kk, CW per element of g, c and acc
template <int HW, int CW>
__device__ __forceinline__ void sc_feed(double (&acc)[CW], const double (&kk)[HW], const double* __restrict__ g,
                                        const double* __restrict__ c, bool minus) {
    const double s = minus ? -1.0 : 1.0;
    if constexpr (CW == 1) {
        acc[0] = fma(s, fma(kk[0], c[0], g[0]), acc[0]);
    } else {
        double xr = fma(kk[0], c[0], g[0]), xi = fma(kk[0], c[1], g[1]);
        if constexpr (HW == 2) {
            xr = fma(-kk[HW - 1], c[1], xr);
            xi = fma(kk[HW - 1], c[0], xi);
        }
        acc[0] = fma(s, xr, acc[0]);
        acc[CW - 1] = fma(s, xi, acc[CW - 1]);
    }
}

// acc += w s (g + kk c), w = 1/2 on the diagonal of X: the term s (g + kk c) through sc_feed from 0, which is exact, and the
// weight a power of two, so the one rounding is that of the sum
template <int HW, int CW>
__device__ __forceinline__ void sc_feed_tri(double (&acc)[CW], const double (&kk)[HW], const double* __restrict__ g,
                                            const double* __restrict__ c, bool minus, bool diagonal) {
    double x[CW];
#pragma unroll
    for (int w = 0; w < CW; ++w) x[w] = 0.0;
    sc_feed<HW, CW>(x, kk, g, c, minus);
    const double wt = diagonal ? 0.5 : 1.0;
#pragma unroll
    for (int w = 0; w < CW; ++w) acc[w] = fma(wt, x[w], acc[w]);
}

// the term of the source element (row, col) = k c + G_p there: the plain chain for the rectangle, the weighted one for the triangle
template <int HW, int CW, class Layout>
__device__ __forceinline__ void sc_feed_at(double (&acc)[CW], const double (&kk)[HW], const double* __restrict__ g,
                                           const double* __restrict__ ck, const Layout& lay, int64_t row, int64_t col, int64_t nb,
                                           bool minus) {
    const double* __restrict__ x = g + lay.at(row, col) * CW;
    const double* __restrict__ y = ck + (row * nb + col) * CW;
    if constexpr (Layout::kPacked) sc_feed_tri<HW, CW>(acc, kk, x, y, minus, lay.diagonal(row, col));
    else sc_feed<HW, CW>(acc, kk, x, y, minus);
}

// ---- sigma in passes over alpha rows of the intermediate (qs_string_ci_sigma_rows) -------------------------------------
// The fold runs over every (k, Ia, tile) in every pass and keeps the terms whose SOURCE row lies in the pass -- the alpha
// term of pr when r0 <= Ta[Ia,pr] < r1, the beta terms when r0 <= Ia < r1 --, so nothing is scattered: a pass adds into
// sigma, the first one (r0 = 0) starts from 0 and never reads it.  The order of one element's sum is pass ascending, pr
// ascending, alpha before beta; a pass boundary stores and reloads the accumulator exactly, so the passes of any schedule
// give the bits of the one pass [0, na).
//
// ---- sigma on the lower triangle for c = tau c^T (qs_string_ci_sigma_sym) ------------------------------------------------
// One table T and n strings for both spins, (P c)[Ia, Ib] = c[Ib, Ia], tau = +-1.  For c = tau P c every row D[(qs), k, :, :]
// and with it G = W . D and X = G + k c have the parity tau in (Ka, Kb): the columns Kb <= Ka carry everything (ScTri).
//   expand : D_p[(qs), k, off(Ka) - off(r0) + Kb] = sgn c_k[T[Ka,qs], Kb] + sgn c_k[Ka, T[Kb,qs]]            Kb <= Ka
//   fold   : S_k[Ia, Ib] (+)= sum_pr ( w(Ja, Ib) sgn X[(pr), k, off(Ja) + Ib]     Ja = T[Ia,pr] in the pass, Ja >= Ib
//                                    + w(Ia, Jb) sgn X[(pr), k, off(Ia) + Jb] )   Jb = T[Ib,pr], Ia in the pass, Jb <= Ia
//            w(r, c) = 1 for r > c, 1/2 for r == c
//   close  : sigma_k = S_k + tau S_k^T
// The fold runs over the whole square and reads only stored elements: the terms it drops are tau times the kept terms of
// the transposed element, and a diagonal element of X is met from both sides, hence the exact 1/2.  Its two reads are those
// of the rectangle -- contiguous over the lanes for alpha, a gather inside ONE packed row for beta --; nothing is strided by
// n.  The close makes sigma[a, b] == tau sigma[b, a] hold bit for bit, with +0.0 on the diagonal for tau = -1.

template <int FORM, class Layout>
__global__ __launch_bounds__(kScBlock) void string_ci_fold_kernel(const ScArgs a, const int32_t* __restrict__ ta,
                                                                 double* __restrict__ sigma, const Layout lay) {
    constexpr int HW = form_widths(FORM).uw, CW = form_widths(FORM).aw;
    extern __shared__ __attribute__((aligned(16))) int32_t sc_tb[];
    const int B = blockDim.x, t = threadIdx.x, m2 = a.m2;
    const unsigned row = blockIdx.x / a.ntile;                            // (k, ia), uniform
    const int64_t k = row / (unsigned)a.na, ia = row % (unsigned)a.na;
    const int64_t ib0 = (int64_t)(blockIdx.x % a.ntile) * B;
    const int64_t ib = ib0 + t, nb = a.nb, dim = a.na * a.nb, r0 = lay.r0, r1 = lay.r1, pdim = lay.pdim();
    const bool live = ib < nb;
    const int32_t* __restrict__ ta_row = ta + ia * m2;
    const double* __restrict__ ck = a.c + k * dim * CW;
    const double* __restrict__ kk = a.kk;
    const double* __restrict__ Gk = a.G + k * pdim * CW;                  // X_p[(pr), k, :] = Gk + pr K pdim
    double* __restrict__ out = sigma + (k * dim + ia * nb + ib) * CW;
    double acc[CW];
#pragma unroll
    for (int w = 0; w < CW; ++w) acc[w] = (r0 > 0 && live) ? out[w] : 0.0;        // the first pass never reads sigma
    if (ia >= r0 && ia < r1) {                                            // uniform: the row Ia itself is in the pass
        for (int pr0 = 0; pr0 < m2; pr0 += kScChunk) {
            __syncthreads();
            sc_stage(sc_tb, a.tb, ib0, nb, pr0, m2);
            __syncthreads();
            if (!live) continue;
            const int nj = m2 - pr0 < kScChunk ? m2 - pr0 : kScChunk;
            for (int j = 0; j < nj; ++j) {
                const int pr = pr0 + j;
                const int32_t ea = ta_row[pr];                            // uniform address: a scalar load
                const int32_t eb = sc_tb[j * (B + 1) + t];
                double kpr[HW];
#pragma unroll
                for (int w = 0; w < HW; ++w) kpr[w] = kk[pr * HW + w];
                const double* __restrict__ g = Gk + (int64_t)pr * a.K * pdim * CW;
                if (ea) {
                    const int64_t ja = sc_target(ea, a.na);               // -1 (past the list) is below every r0
                    // uniform: the row Ja is in the pass and reaches the tile; per lane: the stored columns
                    if (ja >= r0 && ja < r1 && lay.tile(ja, ib0) && lay.holds(ja, ib))
                        sc_feed_at<HW, CW>(acc, kpr, g, ck, lay, ja, ib, nb, ea < 0);
                }
                if (eb) {
                    const int64_t jb = sc_target(eb, nb);
                    if (jb >= 0 && lay.holds(ia, jb)) sc_feed_at<HW, CW>(acc, kpr, g, ck, lay, ia, jb, nb, eb < 0);
                }
            }
        }
    } else if (live) {
        // outside the pass: no beta term, no staging, no barrier; the alpha entries and their tests on the pass and on the
        // tile are scalar
        for (int pr = 0; pr < m2; ++pr) {
            const int32_t ea = ta_row[pr];                                // uniform address: a scalar load
            if (!ea) continue;
            const int64_t ja = sc_target(ea, a.na);
            if (ja < r0 || ja >= r1 || !lay.tile(ja, ib0)) continue;
            if (!lay.holds(ja, ib)) continue;
            double kpr[HW];
#pragma unroll
            for (int w = 0; w < HW; ++w) kpr[w] = kk[pr * HW + w];
            sc_feed_at<HW, CW>(acc, kpr, Gk + (int64_t)pr * a.K * pdim * CW, ck, lay, ja, ib, nb, ea < 0);
        }
    }
    if (live) {
#pragma unroll
        for (int w = 0; w < CW; ++w) out[w] = acc[w];
    }
}

constexpr int kScSymTile = 32;        // the close works on square tiles of 32 x 32 elements, 8 rows per sweep of the workgroup

// sigma_k = S_k + tau S_k^T in place: one workgroup per vector and pair of mirrored tiles (ti, tj), tj <= ti.  Both tiles go
// through LDS (rows padded by one element), so that every read and write of sigma runs along a row; a diagonal tile is its
// own mirror image.  a + tau b and b + tau a are one rounding of the same sum: the two sides agree bit for bit.
template <int CW>
__global__ __launch_bounds__(kScRhoBlock) void string_ci_symmetrize_kernel(double* __restrict__ sigma, int64_t n, unsigned nt,
                                                                           int minus) {
    constexpr int TS = kScSymTile, RS = kScRhoBlock / kScSymTile;
    __shared__ double lo[TS][TS + 1][CW], up[TS][TS + 1][CW];
    const unsigned pair = blockIdx.x % (nt * nt);
    const unsigned ti = pair / nt, tj = pair % nt;                        // uniform
    if (tj > ti) return;
    const bool mirror = ti != tj;
    double* __restrict__ s = sigma + (int64_t)(blockIdx.x / (nt * nt)) * n * n * CW;
    const int tx = threadIdx.x % TS, ty = threadIdx.x / TS;
    const int64_t i0 = (int64_t)ti * TS, j0 = (int64_t)tj * TS;
    for (int r = ty; r < TS; r += RS) {
        if (i0 + r < n && j0 + tx < n) {
#pragma unroll
            for (int w = 0; w < CW; ++w) lo[r][tx][w] = s[((i0 + r) * n + j0 + tx) * CW + w];
        }
        if (mirror && j0 + r < n && i0 + tx < n) {
#pragma unroll
            for (int w = 0; w < CW; ++w) up[r][tx][w] = s[((j0 + r) * n + i0 + tx) * CW + w];
        }
    }
    __syncthreads();
    for (int r = ty; r < TS; r += RS) {
        // the element (i0 + r, j0 + tx) and its mirror image (j0 + tx, i0 + r): loaded under the same two conditions
        if (i0 + r < n && j0 + tx < n) {
            const bool zero = !mirror && r == tx && minus;
#pragma unroll
            for (int w = 0; w < CW; ++w) {
                const double x = lo[r][tx][w], y = mirror ? up[tx][r][w] : lo[tx][r][w];
                s[((i0 + r) * n + j0 + tx) * CW + w] = zero ? 0.0 : (minus ? x - y : x + y);
            }
        }
        if (mirror && j0 + r < n && i0 + tx < n) {
#pragma unroll
            for (int w = 0; w < CW; ++w) {
                const double x = up[r][tx][w], y = lo[tx][r][w];
                s[((j0 + r) * n + i0 + tx) * CW + w] = minus ? x - y : x + y;
            }
        }
    }
}

// T[K, p * m + q] of one string list: one thread per entry (grid-stride).
__global__ __launch_bounds__(kScRhoBlock) void string_ci_table_kernel(const int64_t* __restrict__ strings, int64_t n, int m,
                                                                      int32_t* __restrict__ table) {
    const int64_t total = n * m * m, step = (int64_t)gridDim.x * kScRhoBlock;
    for (int64_t idx = (int64_t)blockIdx.x * kScRhoBlock + threadIdx.x; idx < total; idx += step) {
        const int64_t row = idx / (m * m);
        const int pq = (int)(idx % (m * m)), p = pq / m, q = pq % m;
        const uint64_t Kmask = (uint64_t)strings[row] & (dc_bit(m) - 1);
        int32_t e = 0;
        if ((Kmask & dc_bit(p)) && (p == q || !(Kmask & dc_bit(q)))) {
            const int64_t pos = p == q ? row : dc_find(strings, n, Kmask ^ dc_bit(p) ^ dc_bit(q));
            if (pos >= 0) {
                const bool minus = (__popcll((unsigned long long)(Kmask & dc_between(p, q))) & 1) != 0;
                e = minus ? -(int32_t)(pos + 1) : (int32_t)(pos + 1);
            }
        }
        table[idx] = e;
    }
}

// The ladder table L[J, p] (n_t, m) between two lists of ONE spin, one thread per entry (grid-stride): +-(index in source of
// target[J] ^ bit p, plus 1), sign (-1)^(bits of target[J] below p), the sign of a_p and of a+_p alike (source and target
// differ in bit p alone); 0 where that mask is not in source.  Against a source one particle richer only p outside J can hit
// (annihilation, out of source into target), against one a particle poorer only p in J (creation).
__global__ __launch_bounds__(kScRhoBlock) void string_ci_ladder_table_kernel(const int64_t* __restrict__ target, int64_t n_t,
                                                                             const int64_t* __restrict__ source, int64_t n_s, int m,
                                                                             int32_t* __restrict__ table) {
    const int64_t total = n_t * m, step = (int64_t)gridDim.x * kScRhoBlock;
    for (int64_t idx = (int64_t)blockIdx.x * kScRhoBlock + threadIdx.x; idx < total; idx += step) {
        const int64_t row = idx / m;
        const int p = (int)(idx % m);
        const uint64_t J = (uint64_t)target[row] & (dc_bit(m) - 1);
        const int64_t pos = dc_find(source, n_s, J ^ dc_bit(p));
        int32_t e = 0;
        if (pos >= 0) {
            const bool minus = (__popcll((unsigned long long)(J & (dc_bit(p) - 1))) & 1) != 0;
            e = minus ? -(int32_t)(pos + 1) : (int32_t)(pos + 1);
        }
        table[idx] = e;
    }
}

// D[Ia, Ib] = sum_p n_p ht[p,p] + 1/2 sum_pq n_p n_q ut[p,q,p,q] - 1/2 sum_pq (n_pa n_qa + n_pb n_qb) ut[p,q,q,p]  (real
// parts): one thread per determinant (grid-stride), p and q ascending over the occupied orbitals.
template <int HW>
__global__ __launch_bounds__(kScRhoBlock) void string_ci_diagonal_kernel(const double* __restrict__ ht, const double* __restrict__ ut,
                                                                         const int64_t* __restrict__ sa, const int64_t* __restrict__ sb,
                                                                         int64_t na, int64_t nb, int m, double* __restrict__ D) {
    const int64_t total = na * nb, step = (int64_t)gridDim.x * kScRhoBlock;
    const uint64_t all = dc_bit(m) - 1;
    for (int64_t idx = (int64_t)blockIdx.x * kScRhoBlock + threadIdx.x; idx < total; idx += step) {
        const uint64_t A = (uint64_t)sa[idx / nb] & all, Bm = (uint64_t)sb[idx % nb] & all;
        double d = 0.0;
        for (uint64_t po = A | Bm; po; po &= po - 1) {
            const int p = dc_lowest(po);
            const double pa = (double)((A >> p) & 1), pb = (double)((Bm >> p) & 1);
            d = fma(pa + pb, ht[(size_t)(p * m + p) * HW], d);
            for (uint64_t qo = A | Bm; qo; qo &= qo - 1) {
                const int q = dc_lowest(qo);
                const double qa = (double)((A >> q) & 1), qb = (double)((Bm >> q) & 1);
                d = fma(0.5 * (pa + pb) * (qa + qb), ut[(size_t)(((p * m + q) * m + p) * m + q) * HW], d);
                d = fma(-0.5 * (pa * qa + pb * qb), ut[(size_t)(((p * m + q) * m + q) * m + p) * HW], d);
            }
        }
        D[idx] = d;
    }
}

// rho[q * m + p] = sum_K conj(bra[K]) D[(pq), K]: one workgroup per pq = p * m + q strides over the dim determinants and
// closes with the xor butterfly of each wave and a fixed sum over the four waves.
template <int CW>
__global__ __launch_bounds__(kScRhoBlock) void string_ci_dot_kernel(const double* __restrict__ bra, const double* __restrict__ D,
                                                                    double* __restrict__ rho, int m, int64_t dim) {
    __shared__ double part[kScRhoBlock / 64][CW];
    const int p = blockIdx.x / m, q = blockIdx.x % m, tid = threadIdx.x;
    const double* __restrict__ row = D + (int64_t)blockIdx.x * dim * CW;
    double acc[CW];
#pragma unroll
    for (int w = 0; w < CW; ++w) acc[w] = 0.0;
    for (int64_t i = tid; i < dim; i += kScRhoBlock) {
        if constexpr (CW == 1) {
            acc[0] = fma(bra[i], row[i], acc[0]);
        } else {
            const double ar = bra[2 * i], ai = bra[2 * i + 1], br = row[2 * i], bi = row[2 * i + 1];
            acc[0] = fma(ai, bi, fma(ar, br, acc[0]));                    // conj(a) b
            acc[CW - 1] = fma(-ai, br, fma(ar, bi, acc[CW - 1]));
        }
    }
    const int lane = tid & 63, wave = tid >> 6;
#pragma unroll
    for (int w = 0; w < CW; ++w) {
#pragma unroll
        for (int mask = 32; mask >= 1; mask >>= 1) acc[w] += __shfl_xor(acc[w], mask);
        if (lane == 0) part[wave][w] = acc[w];
    }
    __syncthreads();
    if (tid < CW) {
        double s = part[0][tid];
#pragma unroll
        for (int v = 1; v < kScRhoBlock / 64; ++v) s += part[v][tid];
        rho[(size_t)(q * m + p) * CW + tid] = s;
    }
}

// ---- host side ---------------------------------------------------------------------------------------------------------

static inline bool sc_list_ok(int64_t n) { return n >= 1 && n < 0x7fffffffLL; }

// Extents of one call on K vectors: the columns of its product (K na nb elements of c, twice that as real columns for a
// real W against complex c) fit the product's 32-bit extents, which also keeps every grid below 2^31 workgroups.
static inline bool sc_extents_ok(int form, int64_t m, int64_t na, int64_t nb, int64_t K) {
    if (m < 1 || m > 63 || !sc_list_ok(na) || !sc_list_ok(nb) || K < 1) return false;
    int64_t cols;
    if (__builtin_mul_overflow(na * nb, K, &cols) || __builtin_mul_overflow(cols, (int64_t)(form == 2 ? 2 : 1), &cols)) return false;
    return cols <= 0x7fffffffLL;
}

// The byte budget of a call: the calling thread's string_ci_bytes, else the argument, else the shipped one.
static inline int64_t sc_budget(int64_t budget_bytes) {
    return g_tune.string_ci_bytes > 0 ? g_tune.string_ci_bytes : (budget_bytes > 0 ? budget_bytes : kScBytes);
}

// bytes of D (and of G): m^2 K na nb elements of c, to the next multiple of 16
static inline int64_t sc_panel_bytes(int form, int64_t m, int64_t na, int64_t nb, int64_t K) {
    return (m * m * K * na * nb * 8 * form_widths(form).aw + 15) & ~int64_t(15);      // < 2^12 * 2^31 * 16; G stays 16-byte aligned
}

static inline int sc_threads(int64_t nb) { return nb <= 64 ? 64 : (nb <= 128 ? 128 : kScBlock); }
static inline size_t sc_lds(int threads) { return sizeof(int32_t) * kScChunk * (threads + 1); }

static ScArgs sc_args(const int32_t* ta, const int32_t* tb, const void* c, int64_t m, int64_t na, int64_t nb, int64_t K) {
    ScArgs a{};
    a.ta = ta; a.tb = tb; a.c = (const double*)c;
    a.na = na; a.nb = nb; a.m2 = (int)(m * m); a.K = (int)K;
    a.ntile = (unsigned)cdiv(nb, sc_threads(nb));
    return a;
}

struct ScSpan {
    const void* at;
    int64_t bytes;
};

// The alias rule of every entry: no output shares a byte with an input or with an output before it.
static int sc_alias(const ScSpan* out, const ScSpan* out_end, std::initializer_list<ScSpan> in) {
    for (const ScSpan* o = out; o != out_end; ++o) {
        for (const ScSpan& x : in)
            if (overlaps(o->at, o->bytes, x.at, x.bytes)) return QS_ERR_ALIAS;
        for (const ScSpan* b = out; b != o; ++b)
            if (overlaps(o->at, o->bytes, b->at, b->bytes)) return QS_ERR_ALIAS;
    }
    return QS_OK;
}

static int sc_alias(std::initializer_list<ScSpan> out, std::initializer_list<ScSpan> in) {
    return sc_alias(out.begin(), out.end(), in);
}

// The refusals of the three sigma entries, in their order: form, extents (extra_ok: those of the entry's own arguments),
// null, alignment, workspace, aliases.  need() gives the bytes of the workspace; it runs on valid extents only.
template <class Need>
static int sc_sigma_check(int form, int h_dtype, int c_dtype, const void* k, const void* W, const int32_t* ta, const int32_t* tb,
                          int64_t m, int64_t na, int64_t nb, const void* c, int64_t K, const void* sigma, const void* work,
                          int64_t work_bytes, bool extra_ok, Need need) {
    if (form < 0) return form;
    if (!extra_ok || !sc_extents_ok(form, m, na, nb, K)) return QS_ERR_BAD_EXTENT;
    if (!k || !W || !ta || !tb || !c || !sigma || !work) return QS_ERR_NULL_POINTER;
    const int64_t hs = (int64_t)elem_size(h_dtype), cs = (int64_t)elem_size(c_dtype);
    if (!aligned(k, (size_t)hs) || !aligned(W, (size_t)hs) || !aligned(ta, 4) || !aligned(tb, 4) || !aligned(c, (size_t)cs) ||
        !aligned(sigma, (size_t)cs) || !aligned(work, 16))
        return QS_ERR_MISALIGNED;
    const int64_t w_bytes = need();
    if (work_bytes < w_bytes) return QS_ERR_WORKSPACE;
    const int64_t m2 = m * m, s_bytes = K * na * nb * cs;
    return sc_alias({{sigma, s_bytes}, {work, w_bytes}},
                    {{c, s_bytes}, {W, m2 * m2 * hs}, {k, m2 * hs}, {ta, na * m2 * 4}, {tb, nb * m2 * 4}});
}

// D_p = expand(c) on the rows of the layout's pass, for the K vectors of a.c
template <class Layout>
static int sc_expand(int cw, const ScArgs& a, void* D, const Layout& lay, hipStream_t s) {
    const int threads = sc_threads(a.nb);
    const unsigned grid = (unsigned)((lay.r1 - lay.r0) * a.ntile);
    with_width(cw, [&](auto CW) {
        hipLaunchKernelGGL((string_ci_expand_kernel<CW, Layout>), dim3(grid), dim3(threads), sc_lds(threads), s, a, a.ta, (double*)D, lay);
    });
    note_dispatch(Layout::kPacked ? "qs::string_ci_expand_kernel<%d, qs::ScTri>" : "qs::string_ci_expand_kernel<%d, qs::ScRect>", cw);
    return launch_status("string CI expand launch");
}

// One sigma: for every pass [r0, next(r0)) of the layout's rows, D_p = expand(c), G_p = W . D_p, sigma (+)= fold(G_p + k c),
// D_p and G_p the two panels of `panel` bytes in work.
template <class Layout, class Next>
static int sc_sigma_passes(int form, int h_dtype, const void* k, const void* W, ScArgs a, void* sigma, void* work, int64_t panel,
                           Next next, hipStream_t s) {
    const FormWidths fw = form_widths(form);
    char* D = (char*)work;
    char* G = D + panel;
    a.kk = (const double*)k; a.G = (const double*)G; a.out = (double*)sigma;
    const int threads = sc_threads(a.nb);
    const unsigned grid = (unsigned)(a.K * a.na * a.ntile);
    for (int64_t r0 = 0; r0 < a.na;) {
        const Layout lay{r0, next(r0), a.nb};
        int rc = sc_expand(fw.aw, a, D, lay, s);
        if (rc) return rc;
        // real W against complex c: the re / im pairs of D_p are columns of a real product
        rc = gemm(packed(h_dtype, W, D, G, a.m2, a.K * lay.pdim() * (fw.aw / fw.uw), a.m2), s);
        if (rc) return rc;
        with_form(form, [&](auto FORM) {
            hipLaunchKernelGGL((string_ci_fold_kernel<FORM, Layout>), dim3(grid), dim3(threads), sc_lds(threads), s, a, a.ta, a.out, lay);
            note_dispatch(Layout::kPacked ? "qs::string_ci_fold_kernel<%d, qs::ScTri>" : "qs::string_ci_fold_kernel<%d, qs::ScRect>",
                          (int)FORM);
        });
        rc = launch_status("string CI fold launch");
        if (rc) return rc;
        r0 = lay.r1;
    }
    return QS_OK;
}

// The schedule and the workspace of one qs_string_ci_sigma_rows call, fixed by its arguments and the calling thread's
// string_ci_bytes alone: the one place that carves it.
struct ScRowsPlan {
    int64_t rows, passes;     // alpha rows per pass (the last pass may have fewer), passes
    int64_t cols;             // columns of a full pass's product
    int64_t panel;            // bytes of D_p (and of G_p) of a full pass
};

static ScRowsPlan sc_rows_plan(int form, int64_t m, int64_t na, int64_t nb, int64_t K, int64_t budget_bytes) {
    const int64_t budget = sc_budget(budget_bytes);
    // 2 ceil16(x) <= budget  <=>  x <= the multiple of 16 at or below budget / 2
    int64_t rows = ((budget / 2) & ~int64_t(15)) / (m * m * K * nb * 8 * form_widths(form).aw);
    // rows <= na also keeps a pass's product within 2^31 - 1 columns: sc_extents_ok has bounded those of all na rows
    rows = rows < 1 ? 1 : (rows < na ? rows : na);
    ScRowsPlan p{};
    p.passes = cdiv(na, rows);
    p.rows = cdiv(na, p.passes);                                          // the same passes, of equal length
    p.cols = K * p.rows * nb * (form == 2 ? 2 : 1);
    p.panel = sc_panel_bytes(form, m, p.rows, nb, K);
    return p;
}

// The passes of one qs_string_ci_sigma_sym call over the packed rows, fixed by its arguments and the calling thread's
// string_ci_bytes alone: greedy from row 0, every pass as many rows as its D_p and G_p hold.
struct ScTriPlan {
    int64_t most;             // packed elements per (qs) and vector that a panel of half the budget holds
    int64_t passes, longest;  // passes, the largest off(b_i+1) - off(b_i)
    int64_t cols;             // columns of the largest product
    int64_t panel;            // bytes of D_p (and of G_p) of the largest pass
};

// the end of the pass that starts at row b: the largest r <= n with off(r) - off(b) <= most, at least b + 1
static int64_t sc_tri_next(int64_t b, int64_t n, int64_t most) {
    int64_t lo = b + 1, hi = n;
    while (lo < hi) {
        const int64_t mid = lo + (hi - lo + 1) / 2;
        if (sc_off(mid) - sc_off(b) <= most) lo = mid;
        else hi = mid - 1;
    }
    return lo;
}

// bounds, where given, has room for the passes + 1 boundaries of a plan already known; the others stay within n + 1
static ScTriPlan sc_tri_plan(int form, int64_t m, int64_t n, int64_t K, int64_t budget_bytes, int64_t* bounds, int64_t bounds_len) {
    const int64_t budget = sc_budget(budget_bytes);
    const int64_t per = m * m * K * 8 * form_widths(form).aw;             // bytes per packed element of a panel
    ScTriPlan p{};
    // 2 ceil16(x) <= budget  <=>  x <= the multiple of 16 at or below budget / 2
    p.most = ((budget / 2) & ~int64_t(15)) / per;
    for (int64_t b = 0; b < n; ++p.passes) {
        if (bounds && p.passes < bounds_len) bounds[p.passes] = b;
        const int64_t e = sc_tri_next(b, n, p.most), len = sc_off(e) - sc_off(b);
        p.longest = len > p.longest ? len : p.longest;
        b = e;
    }
    if (bounds && p.passes < bounds_len) bounds[p.passes] = n;
    // longest <= off(n) <= n^2: sc_extents_ok has bounded the columns
    p.cols = K * p.longest * (form == 2 ? 2 : 1);
    p.panel = (per * p.longest + 15) & ~int64_t(15);
    return p;
}

static unsigned sc_stride_grid(int64_t total) {
    const int64_t want = cdiv(total, kScRhoBlock);
    return (unsigned)(want < 65536 ? want : 65536);
}

// ---- two-body density and S^2 ------------------------------------------------------------------------------------------
//   X[(pr),(qs)]  = <bra| E_pr E_qs |ket> = sum_K conj((E_rp bra)[K]) (E_qs ket)[K]          (E_pr^+ = E_rp, E real)
//   Gamma[p,q,r,s] = sum_spins <bra| a+_p a+_q a_s a_r |ket> = X[(pr),(qs)] - delta_qr <bra| E_ps |ket>
// X is a Gram product of two expanded panels over the determinants, cut into passes over alpha rows so that both panels
// fit a byte budget.  Per pass: the bra panel A[(pq), K] (K fastest) = conj(E_pq bra), stored at (pq) as it stands, with
// conj(bra) itself as row m^2; the ket panel B[K, (qs)] ((qs) fastest) = E_qs ket; ONE batched product over T slices of
// kc determinants that adds into T partial results (m^2 + 1, m^2).  The close sums the partials in ascending t, reads X
// at the transposed row (rp), and takes the delta term and rho from the last row <bra| E_qs |ket>.  No atomics.
//   S^2 = S_z (S_z + 1) + N_beta - sum_pq E^alpha_qp E^beta_pq,      S_z = (N_alpha - N_beta) / 2
// is one gather through both tables per (p, q).  On a truncated list a missing target contributes nothing: like H, S^2 is
// then the operator of the truncated formulation, not the projection of the full one.

// Spin-resolved (qs_string_ci_density2_spin):
// E^s_pq = a+_ps a_qs acts on the strings of ONE spin: (E^a_pq c)[Ia, Ib] = sgn c[Ta[Ia,pq], Ib], (E^b_pq c)[Ia, Ib] =
// sgn c[Ia, Tb[Ib,pq]].
//   X^st[(pr),(qs)]   = <bra| E^s_pr E^t_qs |ket> = sum_K conj((E^s_rp bra)[K]) (E^t_qs ket)[K]
//   Gamma^st[p,q,r,s] = <bra| a+_ps a+_qt a_st a_rs |ket> = X^st[(pr),(qs)] - delta_st delta_qr <bra| E^s_ps |ket>
//   rho^s[q,p]        = <bra| E^s_pq |ket>
// The two panels of the spin-summed density with the alpha and the beta replacement kept apart; h = m^2, for fp64 rounded
// up to even so that every block below starts on a 16-byte boundary with an even leading dimension (the pad column holds
// zeros and is never read by the close).  Per pass, K counting its determinants:
//   ket panel B[K, 2 h]         : columns (qs) = E^a_qs ket, columns h + (qs) = E^b_qs ket
//   bra panel A[2 m^2 + 1, K]   : rows (pq) = conj(E^a_pq bra), row m^2 = conj(bra), rows m^2 + 1 + (pq) = conj(E^b_pq bra)
//   part1[t] (m^2 + 1, 2 h) (+)= A[0 ... m^2, slice t] . B[slice t, :]           X^aa | X^ab, last row <E^a_qs> | <E^b_qs>
//   part2[t] (m^2, h)       (+)= A[m^2 + 1 ..., slice t] . B[slice t, h ...]     X^bb
// The beta-alpha block is never formed: Gamma^ba[p,q,r,s] = Gamma^ab[q,p,s,r].  Expand, layout, passes and
// close are those of the spin sum, over S = 2 blocks instead of 1 (Sc2Shape).

constexpr int64_t kSc2Cus = 256;      // compute units the slices of one pass are meant to cover
constexpr int kScSpinG = 4;           // vectors that share the table reads of one S^2 workgroup

struct Sc2Args {
    const int32_t* tb;        // (nb, m^2)
    const double* c;          // (na, nb): bra or ket
    int64_t na, nb;
    int64_t ia0;              // first alpha row of the pass
    int64_t pitch;            // elements between rows of the bra panel, T kc
    unsigned ntile;
    int m2, h, S;             // Sc2Shape's: S spin blocks of h columns per determinant of the ket panel
};

// The expand of one pass, alpha rows ia0 ... ia0 + gridDim.x / ntile - 1, in the layout of one operand of the Gram product(s).
// S = 1: one block per determinant, the spin sum E_pq c.  S = 2: the alpha replacement E^a_pq c, then the beta one.
// KET: P[K, s h + (pq)] -- a thread keeps the 16 values of a table chunk of one block and writes them into the line of its
// determinant with 16-byte stores (8-byte ones where an odd h leaves the line on an 8-byte boundary: S = 1 in fp64 only, for
// S = 2 rounds h up to even and the pad columns m^2 <= pq < h receive zeros).  Otherwise P[s (m^2 + 1) + (pq), K], conjugated,
// every row written as it is formed, four columns in flight, and conj(c) as row m^2.  K = (Ia - ia0) nb + Ib counts the
// determinants of the pass.
template <int CW, bool KET, int S>
__global__ __launch_bounds__(kScBlock) void string_ci_expand_panel_kernel(const Sc2Args a, const int32_t* __restrict__ ta,
                                                                         double* __restrict__ P) {
    extern __shared__ __attribute__((aligned(16))) int32_t sc_tb[];
    const int B = blockDim.x, t = threadIdx.x, m2 = a.m2, h = a.h;
    const int64_t il = blockIdx.x / a.ntile;                              // uniform
    const int64_t ia = a.ia0 + il;
    const int64_t ib0 = (int64_t)(blockIdx.x % a.ntile) * B;
    const int64_t ib = ib0 + t, nb = a.nb;
    const bool live = ib < nb;
    const int64_t kl = il * nb + ib;
    const int32_t* __restrict__ ta_row = ta + ia * m2;
    const double* __restrict__ c = a.c;
    const bool wide = CW == 2 || S == 2 || !(h & 1);                      // every line and block starts on a 16-byte boundary
    // column pq of block s, j its place in the staged chunk; the alpha entry has a uniform address: a scalar load.  Past m^2
    // (uniform) the entries are 0 and so is the value: the pad columns
    auto value = [&](double (&v)[CW], int s, int pq, int j) {
        const int32_t ea = pq < m2 && (S == 1 || s == 0) ? ta_row[pq] : 0;
        const int32_t eb = pq < m2 && (S == 1 || s == 1) ? sc_tb[j * (B + 1) + t] : 0;
        if constexpr (S == 1) sc_replaced<CW>(v, c, ea, eb, ia, ib, a.na, nb);
        else sc_replaced_spin<CW>(v, c, s == 0 ? ea : eb, s != 0, ia, ib, a.na, nb);
    };
    for (int pq0 = 0; pq0 < m2; pq0 += kScChunk) {
        __syncthreads();
        sc_stage(sc_tb, a.tb, ib0, nb, pq0, m2);
        __syncthreads();
        if (!live) continue;
#pragma unroll
        for (int s = 0; s < S; ++s) {
            if constexpr (KET) {
                double v[kScChunk][CW];
#pragma unroll
                for (int j = 0; j < kScChunk; ++j) value(v[j], s, pq0 + j, j);
                double* line = P + ((kl * S + s) * h + pq0) * CW;
                if (wide) {
                    // an even h ends on an even column: the pairs of an fp64 line are whole
#pragma unroll
                    for (int j = 0; j < kScChunk; j += 2 / CW) {
                        if (pq0 + j < h) {
                            double2 x;
                            if constexpr (CW == 2) { x.x = v[j][0]; x.y = v[j][CW - 1]; }
                            else { x.x = v[j][0]; x.y = v[j + 2 / CW - 1][0]; }
                            *reinterpret_cast<double2*>(line + j * CW) = x;
                        }
                    }
                } else {
#pragma unroll
                    for (int j = 0; j < kScChunk; ++j)
                        if (pq0 + j < h) line[j] = v[j][0];
                }
            } else {
                const int nj = m2 - pq0 < kScChunk ? m2 - pq0 : kScChunk;
#pragma unroll 4
                for (int j = 0; j < nj; ++j) {
                    double v[CW];
                    value(v, s, pq0 + j, j);
                    double* d = P + ((int64_t)(s * (m2 + 1) + pq0 + j) * a.pitch + kl) * CW;
                    d[0] = v[0];
                    if constexpr (CW == 2) d[CW - 1] = -v[CW - 1];
                }
            }
        }
    }
    if constexpr (!KET) {
        if (live) {
            const double* x = c + (ia * nb + ib) * CW;
            double* d = P + ((int64_t)m2 * a.pitch + kl) * CW;
            d[0] = x[0];
            if constexpr (CW == 2) d[CW - 1] = -x[CW - 1];
        }
    }
}

// x = sum over t of part[t * stride + at], ascending
template <int CW>
__device__ __forceinline__ void sc_sum_partials(double (&x)[CW], const double* __restrict__ part, int64_t T, int64_t stride,
                                                int64_t at) {
#pragma unroll
    for (int w = 0; w < CW; ++w) x[w] = 0.0;
    for (int64_t t = 0; t < T; ++t) {
#pragma unroll
        for (int w = 0; w < CW; ++w) x[w] += part[(t * stride + at) * CW + w];
    }
}

// One Gamma of a close: where its X lies in the partial results, and what it writes.
struct Sc2Block {
    const double* part;       // the block's partial results, slice t at part + t stride
    int64_t stride;
    int64_t ld, col0;         // X[(pr),(qs)] lies at (rp) ld + col0 + (qs)
    int64_t erow;             // <bra| E_pq |ket> of the block's spin lies at erow + (pq) in the partials of block 0; -1: no delta
                              // term and no rho (the alpha-beta block)
    double* gamma;
    double* rho;
};

struct Sc2Close {
    Sc2Block b[3];
};

// The nblk Gamma[p,q,r,s] and their rho[q m + p] from the partial results: one thread per element of a Gamma (grid-stride over
// the nblk m^4 of them), the partials summed in ascending t, X read at the transposed row (rp), the delta term one subtraction.
template <int CW>
__global__ __launch_bounds__(kScRhoBlock) void string_ci_gamma_close_kernel(const Sc2Close tab, int nblk, int64_t T, int m) {
    const int64_t m2 = (int64_t)m * m, total = m2 * m2, step = (int64_t)gridDim.x * kScRhoBlock;
    const double* __restrict__ epart = tab.b[0].part;
    const int64_t es = tab.b[0].stride;
    for (int64_t idx = (int64_t)blockIdx.x * kScRhoBlock + threadIdx.x; idx < nblk * total; idx += step) {
        const Sc2Block& b = tab.b[idx / total];
        const int64_t el = idx % total;
        const int s = (int)(el % m), r = (int)((el / m) % m), q = (int)((el / m2) % m), p = (int)(el / (m2 * m));
        double x[CW];
        sc_sum_partials<CW>(x, b.part, T, b.stride, ((int64_t)r * m + p) * b.ld + b.col0 + q * m + s);
        if (b.erow >= 0 && q == r) {
            double e[CW];
            sc_sum_partials<CW>(e, epart, T, es, b.erow + p * m + s);                     // <bra| E_ps |ket>
#pragma unroll
            for (int w = 0; w < CW; ++w) x[w] = x[w] - e[w];
        }
#pragma unroll
        for (int w = 0; w < CW; ++w) b.gamma[el * CW + w] = x[w];
        if (b.erow >= 0 && r == 0 && s == 0) {
            double e[CW];
            sc_sum_partials<CW>(e, epart, T, es, b.erow + p * m + q);                     // <bra| E_pq |ket>
#pragma unroll
            for (int w = 0; w < CW; ++w) b.rho[((int64_t)q * m + p) * CW + w] = e[w];
        }
    }
}

// out_k = S^2 c_k for the vectors k0 ... k0 + kScSpinG - 1 of a workgroup: pq ascending over the staged beta columns, the
// alpha entry at the transposed column q m + p, every term an explicit fma, the diagonal term last.
template <int CW>
__global__ __launch_bounds__(kScBlock) void string_ci_spin_kernel(const ScArgs a, const int32_t* __restrict__ ta,
                                                                 double* __restrict__ out, double s0, int m) {
    extern __shared__ __attribute__((aligned(16))) int32_t sc_tb[];
    const int B = blockDim.x, t = threadIdx.x, m2 = a.m2;
    const unsigned row = blockIdx.x / a.ntile;                            // (vector group, ia), uniform
    const int64_t k0 = (int64_t)(row / (unsigned)a.na) * kScSpinG, ia = row % (unsigned)a.na;
    const int64_t ib0 = (int64_t)(blockIdx.x % a.ntile) * B;
    const int64_t ib = ib0 + t, nb = a.nb, dim = a.na * a.nb;
    const bool live = ib < nb;
    const int32_t* __restrict__ ta_row = ta + ia * m2;
    const double* __restrict__ c = a.c;
    const int nk = a.K - k0 < kScSpinG ? (int)(a.K - k0) : kScSpinG;
    double acc[kScSpinG][CW];
#pragma unroll
    for (int g = 0; g < kScSpinG; ++g)
#pragma unroll
        for (int w = 0; w < CW; ++w) acc[g][w] = 0.0;
    for (int pq0 = 0; pq0 < m2; pq0 += kScChunk) {
        __syncthreads();
        sc_stage(sc_tb, a.tb, ib0, nb, pq0, m2);
        __syncthreads();
        if (!live) continue;
        const int nj = m2 - pq0 < kScChunk ? m2 - pq0 : kScChunk;
        for (int j = 0; j < nj; ++j) {
            const int pq = pq0 + j, p = pq / m, q = pq % m;
            const int32_t ea = ta_row[q * m + p];                         // uniform address: a scalar load
            const int32_t eb = sc_tb[j * (B + 1) + t];
            if (!ea || !eb) continue;
            const int64_t ja = sc_target(ea, a.na), jb = sc_target(eb, nb);
            if (ja < 0 || jb < 0) continue;
            const double sg = ((ea < 0) != (eb < 0)) ? 1.0 : -1.0;        // -sgn_a sgn_b
#pragma unroll
            for (int g = 0; g < kScSpinG; ++g) {
                if (g < nk) {
                    const double* x = c + ((k0 + g) * dim + ja * nb + jb) * CW;
#pragma unroll
                    for (int w = 0; w < CW; ++w) acc[g][w] = fma(sg, x[w], acc[g][w]);
                }
            }
        }
    }
    if (live) {
#pragma unroll
        for (int g = 0; g < kScSpinG; ++g) {
            if (g < nk) {
                const int64_t at = ((k0 + g) * dim + ia * nb + ib) * CW;
#pragma unroll
                for (int w = 0; w < CW; ++w) out[at + w] = fma(s0, c[at + w], acc[g][w]);
            }
        }
    }
}

// ---- a one-body operator on a state (qs_string_ci_one_body) ----------------------------------------------------------------
//   out[x, k, Ia, Ib] = sum_pq ( Au[x,p,q] sgn c_k[Ta[Ia,pq], Ib] + Ad[x,p,q] sgn c_k[Ia, Tb[Ib,pq]] )
// A gather with the geometry of the fold and of S^2, and no intermediate: one workgroup per group of up to kScObG operators,
// vector, alpha string and tile of beta strings.  One read of the two table entries and one gather of c per replacement serve
// the whole group.  The order of one element's sum is pq ascending, alpha before beta, every product an explicit fma on the
// signed copy of c (exact); the table's zeros are skipped.

constexpr int kScObG = 4;             // operators that share the table reads and the gathers of one workgroup

// acc += a v: HW doubles per element of a, CW per element of v and acc
template <int HW, int CW>
__device__ __forceinline__ void sc_ob_feed(double (&acc)[CW], const double* __restrict__ a, const double (&v)[CW]) {
    acc[0] = fma(a[0], v[0], acc[0]);
    if constexpr (CW == 2) {
        acc[CW - 1] = fma(a[0], v[CW - 1], acc[CW - 1]);
        if constexpr (HW == 2) {
            acc[0] = fma(-a[HW - 1], v[CW - 1], acc[0]);
            acc[CW - 1] = fma(a[HW - 1], v[0], acc[CW - 1]);
        }
    }
}

template <int FORM>
__global__ __launch_bounds__(kScBlock) void string_ci_one_body_kernel(const ScArgs a, const int32_t* __restrict__ ta,
                                                                     const double* __restrict__ Au, const double* __restrict__ Ad,
                                                                     double* __restrict__ out, int64_t d) {
    constexpr int HW = form_widths(FORM).uw, CW = form_widths(FORM).aw;
    extern __shared__ __attribute__((aligned(16))) int32_t sc_tb[];
    const int B = blockDim.x, t = threadIdx.x, m2 = a.m2;
    const unsigned row = blockIdx.x / a.ntile;                            // (operator group, k, ia), uniform
    const int64_t ia = row % (unsigned)a.na;
    const unsigned gk = row / (unsigned)a.na;
    const int64_t k = gk % (unsigned)a.K, x0 = (int64_t)(gk / (unsigned)a.K) * kScObG;
    const int64_t ib0 = (int64_t)(blockIdx.x % a.ntile) * B;
    const int64_t ib = ib0 + t, nb = a.nb, dim = a.na * a.nb;
    const bool live = ib < nb;
    const int nx = d - x0 < kScObG ? (int)(d - x0) : kScObG;
    const int32_t* __restrict__ ta_row = ta + ia * m2;
    const double* __restrict__ ck = a.c + k * dim * CW;
    const double* __restrict__ au = Au + x0 * m2 * HW;                    // A[x0 + g][pq] at (g m2 + pq) HW: uniform addresses
    const double* __restrict__ ad = Ad + x0 * m2 * HW;
    double acc[kScObG][CW];
#pragma unroll
    for (int g = 0; g < kScObG; ++g)
#pragma unroll
        for (int w = 0; w < CW; ++w) acc[g][w] = 0.0;
    for (int pq0 = 0; pq0 < m2; pq0 += kScChunk) {
        __syncthreads();
        sc_stage(sc_tb, a.tb, ib0, nb, pq0, m2);
        __syncthreads();
        if (!live) continue;
        const int nj = m2 - pq0 < kScChunk ? m2 - pq0 : kScChunk;
        for (int j = 0; j < nj; ++j) {
            const int pq = pq0 + j;
            const int32_t ea = ta_row[pq];                                // uniform address: a scalar load
            const int32_t eb = sc_tb[j * (B + 1) + t];
            if (ea) {                                                     // uniform
                const int64_t ja = sc_target(ea, a.na);
                if (ja >= 0) {
                    const double* x = ck + (ja * nb + ib) * CW;           // contiguous over the lanes
                    double v[CW];
#pragma unroll
                    for (int w = 0; w < CW; ++w) v[w] = ea < 0 ? -x[w] : x[w];
#pragma unroll
                    for (int g = 0; g < kScObG; ++g)
                        if (g < nx) sc_ob_feed<HW, CW>(acc[g], au + ((int64_t)g * m2 + pq) * HW, v);
                }
            }
            if (eb) {
                const int64_t jb = sc_target(eb, nb);
                if (jb >= 0) {
                    const double* x = ck + (ia * nb + jb) * CW;           // a gather inside the row c[Ia, :]
                    double v[CW];
#pragma unroll
                    for (int w = 0; w < CW; ++w) v[w] = eb < 0 ? -x[w] : x[w];
#pragma unroll
                    for (int g = 0; g < kScObG; ++g)
                        if (g < nx) sc_ob_feed<HW, CW>(acc[g], ad + ((int64_t)g * m2 + pq) * HW, v);
                }
            }
        }
    }
    if (live) {
#pragma unroll
        for (int g = 0; g < kScObG; ++g) {
            if (g < nx) {
                double* o = out + (((x0 + g) * a.K + k) * dim + ia * nb + ib) * CW;
#pragma unroll
                for (int w = 0; w < CW; ++w) o[w] = acc[g][w];
            }
        }
    }
}

// ---- particle removal and addition (qs_string_ci_ladder) -------------------------------------------------------------------
//   spin 0: out[x, k, Ja, Jb] = sum_p phi[x,p] sgn(L[Ja,p]) c_k[|L[Ja,p]| - 1, Jb]
//   spin 1: out[x, k, Ja, Jb] = (-1)^n_alpha sum_p phi[x,p] sgn(L[Jb,p]) c_k[Ja, |L[Jb,p]| - 1]
// c lives on the source lists (na_s, nb_s), out on the target lists: (n_t, nb_s) for spin 0, (na_s, n_t) for spin 1; L is the
// ladder table (n_t, m) of the changed spin, and it alone says whether the call annihilates or creates.  The geometry is
// that of the one-body kernel: one workgroup per group of up to kScLadG operators, vector, target alpha string and tile of
// target beta strings.  For spin 0 the table entry and phi[x][p] have uniform addresses and c is read contiguously over the
// lanes; for spin 1 the table columns go through LDS in chunks of kScChunk and c is gathered inside the row c[Ja, :].  The
// order of one element's sum is p ascending, every term ONE fma of a coefficient with the exactly signed copy of c.  Skipped:
// the table's zeros, entries past the source list, and -- a uniform test -- every coefficient that is zero, so that a p whose
// coefficients vanish for the whole group costs no read of c (phi = 1, d = m: m row reads, not m^2 / 4) and an operator has
// the same terms alone and in a group.

constexpr int kScLadG = 4;            // operators that share the table reads and the gathers of one workgroup

struct ScLadArgs {
    const double* c;          // (K, na_s, nb_s)
    int64_t na_s, nb_s;       // the source lists
    int64_t na_t, nb_t;       // the target lists
    int64_t d;
    unsigned ntile;           // tiles of blockDim.x target beta strings
    int m, K, spin;
    int flip;                 // 1 where (-1)^n_alpha = -1 goes with a beta ladder
};

// bit g set where the coefficient phi[x0 + g][p] is not zero: uniform
template <int HW>
__device__ __forceinline__ unsigned sc_lad_live(const double* __restrict__ ph, int m, int p, int nx) {
    unsigned mask = 0;
#pragma unroll
    for (int g = 0; g < kScLadG; ++g) {
        if (g < nx) {
            const double* x = ph + ((int64_t)g * m + p) * HW;
            bool nz = x[0] != 0.0;
            if constexpr (HW == 2) nz = nz || x[HW - 1] != 0.0;
            mask |= nz ? 1u << g : 0u;
        }
    }
    return mask;
}

// acc[g] += phi[x0 + g][p] (+-x) for the operators of mask
template <int HW, int CW>
__device__ __forceinline__ void sc_lad_feed(double (&acc)[kScLadG][CW], const double* __restrict__ ph, int m, int p, unsigned mask,
                                            const double* __restrict__ x, bool minus) {
    double v[CW];
#pragma unroll
    for (int w = 0; w < CW; ++w) v[w] = minus ? -x[w] : x[w];
#pragma unroll
    for (int g = 0; g < kScLadG; ++g)
        if ((mask >> g) & 1u) sc_ob_feed<HW, CW>(acc[g], ph + ((int64_t)g * m + p) * HW, v);
}

template <int FORM>
__global__ __launch_bounds__(kScBlock) void string_ci_ladder_kernel(const ScLadArgs a, const int32_t* __restrict__ table,
                                                                   const double* __restrict__ phi, double* __restrict__ out) {
    constexpr int HW = form_widths(FORM).uw, CW = form_widths(FORM).aw;
    extern __shared__ __attribute__((aligned(16))) int32_t sc_tb[];
    const int B = blockDim.x, t = threadIdx.x, m = a.m;
    const unsigned row = blockIdx.x / a.ntile;                            // (operator group, k, ja), uniform
    const int64_t ja = row % (unsigned)a.na_t;
    const unsigned gk = row / (unsigned)a.na_t;
    const int64_t k = gk % (unsigned)a.K, x0 = (int64_t)(gk / (unsigned)a.K) * kScLadG;
    const int64_t jb0 = (int64_t)(blockIdx.x % a.ntile) * B;
    const int64_t jb = jb0 + t, nb_s = a.nb_s, nb_t = a.nb_t;
    const bool live = jb < nb_t;
    const int nx = a.d - x0 < kScLadG ? (int)(a.d - x0) : kScLadG;
    const double* __restrict__ ck = a.c + k * a.na_s * nb_s * CW;
    const double* __restrict__ ph = phi + x0 * m * HW;                    // phi[x0 + g][p] at (g m + p) HW: uniform addresses
    double acc[kScLadG][CW];
#pragma unroll
    for (int g = 0; g < kScLadG; ++g)
#pragma unroll
        for (int w = 0; w < CW; ++w) acc[g][w] = 0.0;
    if (a.spin == 0) {                                                    // uniform; nb_t == nb_s
        if (live) {
            const int32_t* __restrict__ t_row = table + ja * m;
            for (int p = 0; p < m; ++p) {
                const int32_t e = t_row[p];                               // uniform address: a scalar load
                if (!e) continue;
                const int64_t ia = sc_target(e, a.na_s);
                if (ia < 0) continue;
                const unsigned mask = sc_lad_live<HW>(ph, m, p, nx);
                if (!mask) continue;
                sc_lad_feed<HW, CW>(acc, ph, m, p, mask, ck + (ia * nb_s + jb) * CW, e < 0);      // contiguous over the lanes
            }
        }
    } else {                                                              // na_t == na_s: the row c[Ja, :]
        const bool flip = a.flip != 0;
        for (int p0 = 0; p0 < m; p0 += kScChunk) {
            __syncthreads();
            sc_stage(sc_tb, table, jb0, nb_t, p0, m);
            __syncthreads();
            if (!live) continue;
            const int nj = m - p0 < kScChunk ? m - p0 : kScChunk;
            for (int j = 0; j < nj; ++j) {
                const int p = p0 + j;
                const unsigned mask = sc_lad_live<HW>(ph, m, p, nx);
                if (!mask) continue;
                const int32_t e = sc_tb[j * (B + 1) + t];
                if (!e) continue;
                const int64_t ib = sc_target(e, nb_s);
                if (ib < 0) continue;
                sc_lad_feed<HW, CW>(acc, ph, m, p, mask, ck + (ja * nb_s + ib) * CW, (e < 0) != flip);      // a gather inside the row
            }
        }
    }
    if (live) {
#pragma unroll
        for (int g = 0; g < kScLadG; ++g) {
            if (g < nx) {
                double* o = out + ((((x0 + g) * a.K + k) * a.na_t + ja) * nb_t + jb) * CW;
#pragma unroll
                for (int w = 0; w < CW; ++w) o[w] = acc[g][w];
            }
        }
    }
}

// The panels of one pass of either density, filled here from (spin, cw, m) and nowhere else.
struct Sc2Shape {
    int64_t S;                // spin blocks: 1 (the spin sum) or 2 (alpha | beta)
    int64_t m2, h;            // h: columns of one block of the ket panel, m^2, for S = 2 in fp64 rounded up to even
    int64_t arows, bcols;     // rows of the bra panel S m^2 + 1, columns of the ket panel S h
};

static Sc2Shape sc2_shape(bool spin, int cw, int64_t m) {
    Sc2Shape g{};
    g.S = spin ? 2 : 1;
    g.m2 = m * m;
    g.h = spin && cw == 1 ? (g.m2 + 1) & ~int64_t(1) : g.m2;
    g.arows = g.S * g.m2 + 1;
    g.bcols = g.S * g.h;
    return g;
}

// The schedule and the workspace of one qs_string_ci_density2 or qs_string_ci_density2_spin call.
struct Sc2Plan {
    int64_t rows, passes;     // alpha rows per pass (the last pass may have fewer), passes
    int64_t T, kc, pitch;     // slices of kc determinants per pass, pitch = T kc >= rows nb
    int64_t off_2;            // byte offset of the second block of partial results (S = 2: X^bb) behind the first at 0
    int64_t off_a, off_b;     // byte offsets of the bra and ket panels behind the partial results
    int64_t bytes;
};

// The one place that carves the workspace: T slices of (m^2 + 1, bcols) partial results, for S = 2 T more of (m^2, h), the bra
// panel, the ket panel.
static Sc2Plan sc2_layout(const Sc2Shape& g, int cw, int64_t nb, int64_t rows) {
    const int64_t m2 = g.m2, es = 8 * cw, R = rows * nb;
    Sc2Plan p{};
    p.rows = rows;
    // slices: tiles of the first product x T covers the compute units, the partial results stay below an eighth of the panels
    // (S = 2: 3 h (m^2 + 1) at the most per slice against more than 4 m^2 R)
    int64_t T = cdiv(kSc2Cus, cdiv(m2 + 1, 128) * cdiv(g.bcols, 128));
    const int64_t cap = g.S == 1 ? R / (4 * (m2 + 1)) : (4 * m2 * R) / (24 * g.h * (m2 + 1));
    T = T < cap ? T : cap;
    T = T < 1 ? 1 : T;
    p.kc = (cdiv(R, T) + 1) & ~int64_t(1);                               // even: every slice starts on a 16-byte boundary
    p.T = cdiv(R, p.kc);
    p.pitch = p.T * p.kc;
    p.off_2 = p.T * (m2 + 1) * g.bcols * es;                              // (m^2 + 1) m^2 and 2 h are even
    p.off_a = p.off_2 + (g.S == 2 ? p.T * m2 * g.h * es : 0);             // h or the element size is even
    p.off_b = p.off_a + g.arows * p.pitch * es;                           // pitch is even
    p.bytes = p.off_b + p.pitch * g.bcols * es;
    return p;
}

// The schedule of a pass-wise density: as many alpha rows per pass as keep the two panels, arows + bcols elements per
// determinant, within the budget, at least one; then the same passes of equal length where that costs no more.  The panels
// lie behind off_a.
static Sc2Plan sc2_plan(const Sc2Shape& g, int cw, int64_t na, int64_t nb, int64_t budget_bytes) {
    const int64_t budget = sc_budget(budget_bytes);
    int64_t rows = budget / ((g.arows + g.bcols) * nb * 8 * cw);
    rows = rows < 1 ? 1 : (rows < na ? rows : na);
    Sc2Plan p = sc2_layout(g, cw, nb, rows);
    while (p.rows > 1 && p.bytes - p.off_a > budget) p = sc2_layout(g, cw, nb, p.rows - 1);      // the padding of the slices
    const int64_t passes = cdiv(na, p.rows);
    const Sc2Plan even = sc2_layout(g, cw, nb, cdiv(na, passes));         // the same passes, of equal length
    if (even.bytes - even.off_a <= p.bytes - p.off_a) p = even;
    p.passes = cdiv(na, p.rows);
    return p;
}

static int sc2_check(int c_dtype, int64_t m, int64_t na, int64_t nb, int64_t budget_bytes) {
    if (!dtype_ok(c_dtype)) return QS_ERR_BAD_DTYPE;
    if (!sc_extents_ok(c_dtype == QS_C128 ? 1 : 0, m, na, nb, 1) || budget_bytes < 0) return QS_ERR_BAD_EXTENT;
    return QS_OK;
}

// the workspace query of either density
static int64_t sc2_workspace(bool spin, int c_dtype, int64_t m, int64_t na, int64_t nb, int64_t budget_bytes) {
    const int rc = sc2_check(c_dtype, m, na, nb, budget_bytes);
    if (rc) return rc;
    const int cw = c_dtype == QS_C128 ? 2 : 1;
    return sc2_plan(sc2_shape(spin, cw, m), cw, na, nb, budget_bytes).bytes;
}

// the plan query of either density
static int sc2_plan_query(bool spin, int c_dtype, int64_t m, int64_t na, int64_t nb, int64_t budget_bytes, int64_t* plan) {
    const int rc = sc2_check(c_dtype, m, na, nb, budget_bytes);
    if (rc) return rc;
    if (!plan) return QS_ERR_NULL_POINTER;
    const int cw = c_dtype == QS_C128 ? 2 : 1;
    const Sc2Plan p = sc2_plan(sc2_shape(spin, cw, m), cw, na, nb, budget_bytes);
    plan[0] = p.rows; plan[1] = p.passes; plan[2] = p.T; plan[3] = p.kc; plan[4] = p.bytes;
    return QS_OK;
}

// one operand panel of a pass of `rows` alpha rows: the bra or the ket, of a.S blocks
static int sc2_expand(int cw, bool ket, const Sc2Args& a, const int32_t* ta, int64_t rows, void* P, hipStream_t s) {
    const int threads = sc_threads(a.nb);
    const unsigned grid = (unsigned)(rows * a.ntile);
    auto launch = [&](auto kernel) {
        hipLaunchKernelGGL(kernel, dim3(grid), dim3(threads), sc_lds(threads), s, a, ta, (double*)P);
    };
    with_width(cw, [&](auto CW) {
        if (a.S == 2) ket ? launch(string_ci_expand_panel_kernel<CW, true, 2>) : launch(string_ci_expand_panel_kernel<CW, false, 2>);
        else ket ? launch(string_ci_expand_panel_kernel<CW, true, 1>) : launch(string_ci_expand_panel_kernel<CW, false, 1>);
    });
    note_dispatch("qs::string_ci_expand_panel_kernel<%d, %s, %d>", cw, ket ? "true" : "false", a.S);
    return launch_status("string CI density expand launch");
}

// The passes of either two-body density over alpha rows.  Per pass: zeros in the ragged tails of both panels, the bra panel
// A (arows rows of pitch determinants), the ket panel B (bcols columns per determinant), and the batched product(s) that add
// into the partial results at the head of work (split-k as a batch: slice t is columns t kc ... of A and rows t kc ... of B).
static int sc2_passes(int c_dtype, const Sc2Shape& g, const Sc2Plan& p, const int32_t* ta, const int32_t* tb, int64_t na,
                      int64_t nb, const void* bra, const void* ket, void* work, hipStream_t s) {
    const int cw = c_dtype == QS_C128 ? 2 : 1;
    const int64_t cs = 8 * cw, m2 = g.m2, h = g.h, arows = g.arows, bcols = g.bcols;
    char* part = (char*)work;
    char* A = part + p.off_a;
    char* B = part + p.off_b;
    Sc2Args a{};
    a.tb = tb; a.na = na; a.nb = nb; a.pitch = p.pitch; a.m2 = (int)m2; a.h = (int)h; a.S = (int)g.S;
    a.ntile = (unsigned)cdiv(nb, sc_threads(nb));
    for (int64_t pass = 0; pass < p.passes; ++pass) {
        a.ia0 = pass * p.rows;
        const int64_t rows = na - a.ia0 < p.rows ? na - a.ia0 : p.rows, R = rows * nb;
        int rc;
        if (R < p.pitch) {
            // the tail of the last slice, and of a ragged last pass: zeros in both operands
            rc = hip_status(hipMemset2DAsync(A + R * cs, (size_t)(p.pitch * cs), 0, (size_t)((p.pitch - R) * cs), (size_t)arows, s),
                            "string CI bra panel tail");
            if (rc) return rc;
            rc = hip_status(hipMemsetAsync(B + R * bcols * cs, 0, (size_t)((p.pitch - R) * bcols * cs), s), "string CI ket panel tail");
            if (rc) return rc;
        }
        a.c = (const double*)bra;
        rc = sc2_expand(cw, false, a, ta, rows, A, s);
        if (rc) return rc;
        a.c = (const double*)ket;
        rc = sc2_expand(cw, true, a, ta, rows, B, s);
        if (rc) return rc;
        // the first m^2 + 1 rows of A against all ket columns; spin-resolved, these are the alpha rows and conj(bra):
        // X^aa | X^ab, and <E^a_qs> | <E^b_qs> in the last row
        rc = gemm(Product{c_dtype, (const double*)A, (const double*)B, (double*)part, m2 + 1, bcols, p.kc, p.pitch, bcols, bcols, p.T,
                          p.kc, p.kc * bcols, (m2 + 1) * bcols, pass > 0 ? 1 : 0},
                  s);
        if (rc) return rc;
        if (g.S == 1) continue;
        // beta rows against the beta columns: X^bb
        rc = gemm(Product{c_dtype, (const double*)(A + (m2 + 1) * p.pitch * cs), (const double*)(B + h * cs),
                          (double*)(part + p.off_2), m2, h, p.kc, p.pitch, bcols, h, p.T, p.kc, p.kc * bcols, m2 * h, pass > 0 ? 1 : 0},
                  s);
        if (rc) return rc;
    }
    return QS_OK;
}

// Either two-body density.  out: the 2 S - 1 Gamma (the spin sum, or alpha-alpha, alpha-beta, beta-beta), then the S rho.  The
// refusals in their order: dtype, extents and budget, null, alignment, workspace, aliases.
static int sc2_density(bool spin, int c_dtype, const int32_t* ta, const int32_t* tb, int64_t m, int64_t na, int64_t nb, const void* bra,
                       const void* ket, std::initializer_list<void*> out, void* work, int64_t work_bytes, int64_t budget_bytes,
                       hipStream_t s) {
    dispatch_reset();
    int rc = sc2_check(c_dtype, m, na, nb, budget_bytes);
    if (rc) return rc;
    const int64_t cs = (int64_t)elem_size(c_dtype);
    bool null = !ta || !tb || !bra || !ket || !work;
    bool skew = !aligned(ta, 4) || !aligned(tb, 4) || !aligned(bra, (size_t)cs) || !aligned(ket, (size_t)cs) || !aligned(work, 16);
    for (void* x : out) null = null || !x, skew = skew || !aligned(x, (size_t)cs);
    if (null) return QS_ERR_NULL_POINTER;
    if (skew) return QS_ERR_MISALIGNED;
    const int cw = c_dtype == QS_C128 ? 2 : 1;
    const Sc2Shape g = sc2_shape(spin, cw, m);
    const Sc2Plan p = sc2_plan(g, cw, na, nb, budget_bytes);
    if (work_bytes < p.bytes) return QS_ERR_WORKSPACE;
    const int64_t m2 = g.m2, v_bytes = na * nb * cs;
    const int nblk = (int)(2 * g.S - 1);
    ScSpan span[6] = {{work, p.bytes}};
    void* const* o = out.begin();
    for (int i = 0; i < (int)out.size(); ++i) span[1 + i] = {o[i], (i < nblk ? m2 * m2 : m2) * cs};
    rc = sc_alias(span, span + 1 + out.size(), {{bra, v_bytes}, {ket, v_bytes}, {ta, na * m2 * 4}, {tb, nb * m2 * 4}});
    if (rc) return rc;

    rc = sc2_passes(c_dtype, g, p, ta, tb, na, nb, bra, ket, work, s);
    if (rc) return rc;
    // block 0 reads the first product, X | <E_qs> in its last row; S = 2 adds X^ab beside it (no delta term, no rho) and X^bb from
    // the second product with <E^b_qs> from the last row of the first
    const double* part = (const double*)work;
    Sc2Close tab{};
    tab.b[0] = {part, (m2 + 1) * g.bcols, g.bcols, 0, m2 * g.bcols, (double*)o[0], (double*)o[nblk]};
    if (g.S == 2) {
        tab.b[1] = {part, (m2 + 1) * g.bcols, g.bcols, g.h, -1, (double*)o[1], nullptr};
        tab.b[2] = {(const double*)((const char*)work + p.off_2), m2 * g.h, g.h, 0, m2 * g.bcols + g.h, (double*)o[2], (double*)o[4]};
    }
    with_width(cw, [&](auto CW) {
        hipLaunchKernelGGL((string_ci_gamma_close_kernel<CW>), dim3(sc_stride_grid(nblk * m2 * m2)), dim3(kScRhoBlock), 0, s, tab, nblk,
                           p.T, (int)m);
    });
    note_dispatch("qs::string_ci_gamma_close_kernel<%d>", cw);
    return launch_status(spin ? "string CI spin-resolved density close launch" : "string CI two-body density close launch");
}

}  // namespace qs

using namespace qs;

extern "C" {

int qs_string_ci_table(const int64_t* strings, int64_t n, int64_t m, int64_t N, int32_t* table, void* stream) {
    dispatch_reset();
    if (m < 1 || m > 63 || N < 0 || N > m || !sc_list_ok(n)) return QS_ERR_BAD_EXTENT;
    if (!strings || !table) return QS_ERR_NULL_POINTER;
    if (!aligned(strings, 8) || !aligned(table, 4)) return QS_ERR_MISALIGNED;
    if (overlaps(table, n * m * m * 4, strings, n * 8)) return QS_ERR_ALIAS;
    hipLaunchKernelGGL(string_ci_table_kernel, dim3(sc_stride_grid(n * m * m)), dim3(kScRhoBlock), 0, (hipStream_t)stream,
                       strings, n, (int)m, table);
    note_dispatch("qs::string_ci_table_kernel");
    return launch_status("string CI table launch");
}

int qs_string_ci_diagonal(int h_dtype, const void* ht, const void* ut, const int64_t* sa, int64_t na, int64_t Na,
                          const int64_t* sb, int64_t nb, int64_t Nb, int64_t m, double* D, void* stream) {
    dispatch_reset();
    if (!dtype_ok(h_dtype)) return QS_ERR_BAD_DTYPE;
    if (m < 1 || m > 63 || Na < 0 || Na > m || Nb < 0 || Nb > m || !sc_list_ok(na) || !sc_list_ok(nb)) return QS_ERR_BAD_EXTENT;
    if (!ht || !ut || !sa || !sb || !D) return QS_ERR_NULL_POINTER;
    const int64_t es = (int64_t)elem_size(h_dtype);
    if (!aligned(ht, (size_t)es) || !aligned(ut, (size_t)es) || !aligned(sa, 8) || !aligned(sb, 8) || !aligned(D, 8))
        return QS_ERR_MISALIGNED;
    if (int rc = sc_alias({{D, na * nb * 8}}, {{ht, m * m * es}, {ut, m * m * m * m * es}, {sa, na * 8}, {sb, nb * 8}})) return rc;
    const unsigned grid = sc_stride_grid(na * nb);
    hipStream_t s = (hipStream_t)stream;
    with_width(h_dtype == QS_F64 ? 1 : 2, [&](auto HW) {
        hipLaunchKernelGGL((string_ci_diagonal_kernel<HW>), dim3(grid), dim3(kScRhoBlock), 0, s, (const double*)ht, (const double*)ut, sa, sb, na, nb, (int)m, D);
    });
    note_dispatch("qs::string_ci_diagonal_kernel<%d>", h_dtype == QS_F64 ? 1 : 2);
    return launch_status("string CI diagonal launch");
}

int64_t qs_string_ci_workspace(int h_dtype, int c_dtype, int64_t m, int64_t na, int64_t nb, int64_t K) {
    const int form = tensor_form(h_dtype, c_dtype);
    if (form < 0) return form;
    if (!sc_extents_ok(form, m, na, nb, K)) return QS_ERR_BAD_EXTENT;
    return 2 * sc_panel_bytes(form, m, na, nb, K);
}

int64_t qs_string_ci_group(int h_dtype, int c_dtype, int64_t m, int64_t na, int64_t nb, int64_t K, int64_t budget_bytes) {
    const int form = tensor_form(h_dtype, c_dtype);
    if (form < 0) return form;
    if (!sc_extents_ok(form, m, na, nb, 1) || K < 1 || budget_bytes < 0) return QS_ERR_BAD_EXTENT;
    int64_t g = sc_budget(budget_bytes) / (2 * sc_panel_bytes(form, m, na, nb, 1));
    const int64_t cols = 0x7fffffffLL / (na * nb * (form == 2 ? 2 : 1));      // the product's 32-bit extent
    g = g < cols ? g : cols;
    return g < 1 ? 1 : (g < K ? g : K);
}

int qs_string_ci_sigma(int h_dtype, int c_dtype, const void* k, const void* W, const int32_t* ta, const int32_t* tb,
                       int64_t m, int64_t na, int64_t nb, const void* c, int64_t K, void* sigma, void* work,
                       int64_t work_bytes, void* stream) {
    dispatch_reset();
    const int form = tensor_form(h_dtype, c_dtype);
    int64_t panel = 0;
    if (int rc = sc_sigma_check(form, h_dtype, c_dtype, k, W, ta, tb, m, na, nb, c, K, sigma, work, work_bytes, true,
                                [&] { return 2 * (panel = sc_panel_bytes(form, m, na, nb, K)); }))
        return rc;
    // one pass over all rows
    return sc_sigma_passes<ScRect>(form, h_dtype, k, W, sc_args(ta, tb, c, m, na, nb, K), sigma, work, panel,
                                   [&](int64_t) { return na; }, (hipStream_t)stream);
}

int qs_string_ci_sigma_plan(int h_dtype, int c_dtype, int64_t m, int64_t na, int64_t nb, int64_t K, int64_t budget_bytes,
                            int64_t* plan) {
    const int form = tensor_form(h_dtype, c_dtype);
    if (form < 0) return form;
    if (!sc_extents_ok(form, m, na, nb, K) || budget_bytes < 0) return QS_ERR_BAD_EXTENT;
    if (!plan) return QS_ERR_NULL_POINTER;
    const ScRowsPlan p = sc_rows_plan(form, m, na, nb, K, budget_bytes);
    plan[0] = p.rows; plan[1] = p.passes; plan[2] = p.cols; plan[3] = 2 * p.panel;
    return QS_OK;
}

int qs_string_ci_sigma_rows(int h_dtype, int c_dtype, const void* k, const void* W, const int32_t* ta, const int32_t* tb,
                            int64_t m, int64_t na, int64_t nb, const void* c, int64_t K, void* sigma, void* work,
                            int64_t work_bytes, int64_t budget_bytes, void* stream) {
    dispatch_reset();
    const int form = tensor_form(h_dtype, c_dtype);
    ScRowsPlan p{};
    if (int rc = sc_sigma_check(form, h_dtype, c_dtype, k, W, ta, tb, m, na, nb, c, K, sigma, work, work_bytes, budget_bytes >= 0,
                                [&] { return 2 * (p = sc_rows_plan(form, m, na, nb, K, budget_bytes)).panel; }))
        return rc;
    return sc_sigma_passes<ScRect>(form, h_dtype, k, W, sc_args(ta, tb, c, m, na, nb, K), sigma, work, p.panel,
                                   [&](int64_t r0) { return r0 + p.rows < na ? r0 + p.rows : na; }, (hipStream_t)stream);
}

int qs_string_ci_sigma_sym_plan(int h_dtype, int c_dtype, int64_t m, int64_t n, int64_t K, int64_t budget_bytes,
                                int64_t* plan, int64_t* bounds, int64_t bounds_len) {
    const int form = tensor_form(h_dtype, c_dtype);
    if (form < 0) return form;
    if (!sc_extents_ok(form, m, n, n, K) || budget_bytes < 0) return QS_ERR_BAD_EXTENT;
    if (!plan) return QS_ERR_NULL_POINTER;
    const ScTriPlan p = sc_tri_plan(form, m, n, K, budget_bytes, nullptr, 0);
    if (bounds) {
        if (bounds_len < p.passes + 1) return QS_ERR_BAD_EXTENT;
        sc_tri_plan(form, m, n, K, budget_bytes, bounds, bounds_len);
    }
    plan[0] = p.passes; plan[1] = p.longest; plan[2] = p.cols; plan[3] = 2 * p.panel;
    return QS_OK;
}

int qs_string_ci_sigma_sym(int h_dtype, int c_dtype, const void* k, const void* W, const int32_t* t, int64_t m, int64_t n,
                           int64_t parity, const void* c, int64_t K, void* sigma, void* work, int64_t work_bytes,
                           int64_t budget_bytes, void* stream) {
    dispatch_reset();
    const int form = tensor_form(h_dtype, c_dtype);
    ScTriPlan p{};
    if (int rc = sc_sigma_check(form, h_dtype, c_dtype, k, W, t, t, m, n, n, c, K, sigma, work, work_bytes,
                                (parity == 1 || parity == -1) && budget_bytes >= 0,
                                [&] { return 2 * (p = sc_tri_plan(form, m, n, K, budget_bytes, nullptr, 0)).panel; }))
        return rc;
    hipStream_t s = (hipStream_t)stream;
    if (int rc = sc_sigma_passes<ScTri>(form, h_dtype, k, W, sc_args(t, t, c, m, n, n, K), sigma, work, p.panel,
                                        [&](int64_t r0) { return sc_tri_next(r0, n, p.most); }, s))
        return rc;
    const int cw = form_widths(form).aw;
    const unsigned nt = (unsigned)cdiv(n, kScSymTile);
    with_width(cw, [&](auto CW) {
        hipLaunchKernelGGL((string_ci_symmetrize_kernel<CW>), dim3((unsigned)K * nt * nt), dim3(kScRhoBlock), 0, s, (double*)sigma, n, nt, parity < 0 ? 1 : 0);
    });
    note_dispatch("qs::string_ci_symmetrize_kernel<%d>", cw);
    return launch_status("string CI symmetrise launch");
}

int qs_string_ci_density1(int c_dtype, const int32_t* ta, const int32_t* tb, int64_t m, int64_t na, int64_t nb,
                          const void* bra, const void* ket, void* rho, void* work, int64_t work_bytes, void* stream) {
    dispatch_reset();
    if (!dtype_ok(c_dtype)) return QS_ERR_BAD_DTYPE;
    const int form = c_dtype == QS_C128 ? 1 : 0;
    if (!sc_extents_ok(form, m, na, nb, 1)) return QS_ERR_BAD_EXTENT;
    if (!ta || !tb || !bra || !ket || !rho || !work) return QS_ERR_NULL_POINTER;
    const int64_t cs = (int64_t)elem_size(c_dtype);
    if (!aligned(ta, 4) || !aligned(tb, 4) || !aligned(bra, (size_t)cs) || !aligned(ket, (size_t)cs) || !aligned(rho, (size_t)cs) ||
        !aligned(work, 16))
        return QS_ERR_MISALIGNED;
    const int64_t panel = sc_panel_bytes(form, m, na, nb, 1);
    if (work_bytes < panel) return QS_ERR_WORKSPACE;
    const int64_t m2 = m * m, v_bytes = na * nb * cs;
    if (int rc = sc_alias({{rho, m2 * cs}, {work, panel}}, {{bra, v_bytes}, {ket, v_bytes}, {ta, na * m2 * 4}, {tb, nb * m2 * 4}})) return rc;
    hipStream_t s = (hipStream_t)stream;
    const int cw = form_widths(form).aw;
    // D of the ket, whole: the rectangle's one pass
    if (int rc = sc_expand(cw, sc_args(ta, tb, ket, m, na, nb, 1), work, ScRect{0, na, nb}, s)) return rc;
    with_width(cw, [&](auto CW) {
        hipLaunchKernelGGL((string_ci_dot_kernel<CW>), dim3((unsigned)m2), dim3(kScRhoBlock), 0, s, (const double*)bra, (const double*)work, (double*)rho, (int)m, na * nb);
    });
    note_dispatch("qs::string_ci_dot_kernel<%d>", cw);
    return launch_status("string CI density launch");
}

int64_t qs_string_ci_density2_workspace(int c_dtype, int64_t m, int64_t na, int64_t nb, int64_t budget_bytes) {
    return sc2_workspace(false, c_dtype, m, na, nb, budget_bytes);
}

int qs_string_ci_density2_plan(int c_dtype, int64_t m, int64_t na, int64_t nb, int64_t budget_bytes, int64_t* plan) {
    return sc2_plan_query(false, c_dtype, m, na, nb, budget_bytes, plan);
}

int qs_string_ci_density2(int c_dtype, const int32_t* ta, const int32_t* tb, int64_t m, int64_t na, int64_t nb,
                          const void* bra, const void* ket, void* gamma, void* rho, void* work, int64_t work_bytes,
                          int64_t budget_bytes, void* stream) {
    return sc2_density(false, c_dtype, ta, tb, m, na, nb, bra, ket, {gamma, rho}, work, work_bytes, budget_bytes, (hipStream_t)stream);
}

int64_t qs_string_ci_density2_spin_workspace(int c_dtype, int64_t m, int64_t na, int64_t nb, int64_t budget_bytes) {
    return sc2_workspace(true, c_dtype, m, na, nb, budget_bytes);
}

int qs_string_ci_density2_spin_plan(int c_dtype, int64_t m, int64_t na, int64_t nb, int64_t budget_bytes, int64_t* plan) {
    return sc2_plan_query(true, c_dtype, m, na, nb, budget_bytes, plan);
}

int qs_string_ci_density2_spin(int c_dtype, const int32_t* ta, const int32_t* tb, int64_t m, int64_t na, int64_t nb,
                               const void* bra, const void* ket, void* gamma_aa, void* gamma_ab, void* gamma_bb, void* rho_a,
                               void* rho_b, void* work, int64_t work_bytes, int64_t budget_bytes, void* stream) {
    return sc2_density(true, c_dtype, ta, tb, m, na, nb, bra, ket, {gamma_aa, gamma_ab, gamma_bb, rho_a, rho_b}, work, work_bytes,
                       budget_bytes, (hipStream_t)stream);
}

int qs_string_ci_spin_squared(int c_dtype, const int32_t* ta, const int32_t* tb, int64_t m, int64_t na, int64_t nb,
                              int64_t Na, int64_t Nb, const void* c, int64_t K, void* out, void* stream) {
    dispatch_reset();
    if (!dtype_ok(c_dtype)) return QS_ERR_BAD_DTYPE;
    if (!sc_extents_ok(c_dtype == QS_C128 ? 1 : 0, m, na, nb, K) || Na < 0 || Na > m || Nb < 0 || Nb > m) return QS_ERR_BAD_EXTENT;
    if (!ta || !tb || !c || !out) return QS_ERR_NULL_POINTER;
    const int64_t cs = (int64_t)elem_size(c_dtype);
    if (!aligned(ta, 4) || !aligned(tb, 4) || !aligned(c, (size_t)cs) || !aligned(out, (size_t)cs)) return QS_ERR_MISALIGNED;
    const int64_t m2 = m * m, o_bytes = K * na * nb * cs;
    if (int rc = sc_alias({{out, o_bytes}}, {{c, o_bytes}, {ta, na * m2 * 4}, {tb, nb * m2 * 4}})) return rc;
    const double sz = 0.5 * (double)(Na - Nb), s0 = sz * (sz + 1.0) + (double)Nb;       // multiples of 1/4: exact
    const ScArgs a = sc_args(ta, tb, c, m, na, nb, K);
    const int threads = sc_threads(nb);
    const unsigned grid = (unsigned)(cdiv(K, kScSpinG) * na * a.ntile);
    hipStream_t s = (hipStream_t)stream;
    const int cw = c_dtype == QS_F64 ? 1 : 2;
    with_width(cw, [&](auto CW) {
        hipLaunchKernelGGL((string_ci_spin_kernel<CW>), dim3(grid), dim3(threads), sc_lds(threads), s, a, ta, (double*)out, s0, (int)m);
    });
    note_dispatch("qs::string_ci_spin_kernel<%d>", cw);
    return launch_status("string CI spin launch");
}

int qs_string_ci_one_body(int h_dtype, int c_dtype, const void* A_up, const void* A_down, int64_t d, const int32_t* ta,
                          const int32_t* tb, int64_t m, int64_t na, int64_t nb, const void* c, int64_t K, void* out, void* stream) {
    dispatch_reset();
    const int form = tensor_form(h_dtype, c_dtype);
    if (form < 0) return form;
    if (!sc_extents_ok(form, m, na, nb, K) || d < 1) return QS_ERR_BAD_EXTENT;
    const int64_t hs = (int64_t)elem_size(h_dtype), cs = (int64_t)elem_size(c_dtype);
    const int64_t m2 = m * m, v_elems = K * na * nb, ntile = cdiv(nb, sc_threads(nb));
    int64_t o_bytes, a_bytes, grid;
    if (__builtin_mul_overflow(d, v_elems, &o_bytes) || __builtin_mul_overflow(o_bytes, cs, &o_bytes) ||
        __builtin_mul_overflow(d, m2 * hs, &a_bytes))
        return QS_ERR_BAD_EXTENT;
    if (__builtin_mul_overflow(cdiv(d, kScObG), K * na * ntile, &grid) || grid > 0x7fffffffLL) return QS_ERR_BAD_EXTENT;
    if (!A_up || !ta || !tb || !c || !out) return QS_ERR_NULL_POINTER;
    if (!aligned(A_up, (size_t)hs) || !aligned(A_down, (size_t)hs) || !aligned(ta, 4) || !aligned(tb, 4) || !aligned(c, (size_t)cs) ||
        !aligned(out, (size_t)cs))
        return QS_ERR_MISALIGNED;
    // a null A_down has no bytes: it overlaps nothing
    if (int rc = sc_alias({{out, o_bytes}}, {{c, v_elems * cs}, {A_up, a_bytes}, {A_down, A_down ? a_bytes : 0}, {ta, na * m2 * 4},
                                             {tb, nb * m2 * 4}}))
        return rc;
    const ScArgs a = sc_args(ta, tb, c, m, na, nb, K);
    const int threads = sc_threads(nb);
    hipStream_t s = (hipStream_t)stream;
    with_form(form, [&](auto FORM) {
        hipLaunchKernelGGL((string_ci_one_body_kernel<FORM>), dim3((unsigned)grid), dim3(threads), sc_lds(threads), s, a, ta,
                           (const double*)A_up, (const double*)(A_down ? A_down : A_up), (double*)out, d);
    });
    note_dispatch("qs::string_ci_one_body_kernel<%d>", form);
    return launch_status("string CI one-body launch");
}

int qs_string_ci_ladder_table(const int64_t* target, int64_t n_t, const int64_t* source, int64_t n_s, int64_t m, int32_t* table,
                              void* stream) {
    dispatch_reset();
    if (m < 1 || m > 63 || !sc_list_ok(n_t) || !sc_list_ok(n_s)) return QS_ERR_BAD_EXTENT;
    if (!target || !source || !table) return QS_ERR_NULL_POINTER;
    if (!aligned(target, 8) || !aligned(source, 8) || !aligned(table, 4)) return QS_ERR_MISALIGNED;
    if (int rc = sc_alias({{table, n_t * m * 4}}, {{target, n_t * 8}, {source, n_s * 8}})) return rc;
    hipLaunchKernelGGL(string_ci_ladder_table_kernel, dim3(sc_stride_grid(n_t * m)), dim3(kScRhoBlock), 0, (hipStream_t)stream,
                       target, n_t, source, n_s, (int)m, table);
    note_dispatch("qs::string_ci_ladder_table_kernel");
    return launch_status("string CI ladder table launch");
}

int qs_string_ci_ladder(int h_dtype, int c_dtype, const void* phi, int64_t d, int64_t spin, const int32_t* table, int64_t m,
                        int64_t n_alpha, int64_t na_s, int64_t nb_s, int64_t n_t, const void* c, int64_t K, void* out,
                        void* stream) {
    dispatch_reset();
    const int form = tensor_form(h_dtype, c_dtype);
    if (form < 0) return form;
    if (spin != 0 && spin != 1) return QS_ERR_BAD_EXTENT;
    const int64_t na_t = spin == 0 ? n_t : na_s, nb_t = spin == 0 ? nb_s : n_t;
    if (!sc_extents_ok(form, m, na_s, nb_s, K) || !sc_extents_ok(form, m, na_t, nb_t, K)) return QS_ERR_BAD_EXTENT;
    if (d < 1 || n_alpha < 0 || n_alpha > m) return QS_ERR_BAD_EXTENT;
    const int64_t hs = (int64_t)elem_size(h_dtype), cs = (int64_t)elem_size(c_dtype);
    const int threads = sc_threads(nb_t);
    const int64_t ntile = cdiv(nb_t, threads);
    int64_t o_bytes, p_bytes, grid;
    if (__builtin_mul_overflow(d, K * na_t * nb_t, &o_bytes) || __builtin_mul_overflow(o_bytes, cs, &o_bytes) ||
        __builtin_mul_overflow(d, m * hs, &p_bytes))
        return QS_ERR_BAD_EXTENT;
    if (__builtin_mul_overflow(cdiv(d, kScLadG), K * na_t * ntile, &grid) || grid > 0x7fffffffLL) return QS_ERR_BAD_EXTENT;
    if (!phi || !table || !c || !out) return QS_ERR_NULL_POINTER;
    if (!aligned(phi, (size_t)hs) || !aligned(table, 4) || !aligned(c, (size_t)cs) || !aligned(out, (size_t)cs))
        return QS_ERR_MISALIGNED;
    if (int rc = sc_alias({{out, o_bytes}}, {{c, K * na_s * nb_s * cs}, {phi, p_bytes}, {table, n_t * m * 4}})) return rc;
    ScLadArgs a{};
    a.c = (const double*)c;
    a.na_s = na_s; a.nb_s = nb_s; a.na_t = na_t; a.nb_t = nb_t; a.d = d;
    a.ntile = (unsigned)ntile;
    a.m = (int)m; a.K = (int)K; a.spin = (int)spin;
    a.flip = (spin == 1 && (n_alpha & 1)) ? 1 : 0;
    hipStream_t s = (hipStream_t)stream;
    with_form(form, [&](auto FORM) {
        hipLaunchKernelGGL((string_ci_ladder_kernel<FORM>), dim3((unsigned)grid), dim3(threads), spin == 1 ? sc_lds(threads) : 0, s, a,
                           table, (const double*)phi, (double*)out);
    });
    note_dispatch("qs::string_ci_ladder_kernel<%d>", form);
    return launch_status("string CI ladder launch");
}

}  // extern "C"
