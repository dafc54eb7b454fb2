// Mean-field (Fock) build from a one-body density: both sums of
//   W[p,q] = cj * sum_{r,s} u[p,r,q,s] D[s,r]  +  ck * sum_{r,s} u[p,r,s,q] D[s,r]
// from ONE read of u.  For fixed (p, r) the L x L slab S = u[p,r,:,:] gives  J[p,a] += sum_b S[a,b] D[b,r]  (row dot
// products) and  K[p,b] += sum_a S[a,b] D[a,r]  (weighted column sums): every element S[a,b] is used twice while it
// sits in a register.
//
// Work unit = (row p, chunk of Rc consecutive r): one workgroup of 256 threads.  The threads form a (RT x CT) grid over
// a tile of the slab, CT column threads of one 16-byte item each (two real columns, or one complex element) and RT =
// 256 / CT row threads of TA rows each (row = tile row + i * RT + tr: with CT < 64 a wave's lanes still cover
// consecutive rows, i.e. contiguous memory).  A thread keeps its POSITIONS of the tile and streams over the chunk's r:
// TA running J sums (its rows, its two columns) and its columns' K sums live in registers across r, so nothing crosses
// lanes inside the stream.  After the chunk's last r the tile is closed once: J over the column threads (xor butterfly
// inside a wave, then across the waves of a row through LDS), K over the row threads through LDS, both in a fixed
// order, into the unit's J[L] / K[L] in LDS.  The unit stores cj J + ck K to the caller's workspace, [p][chunk][q]; a
// second small launch adds the chunks in ascending order.  No floating-point atomics; the split into units depends on
// (L, R, dtype) only, so row p of a slab call is bit-identical to row p of the full call.
//
// The chunk's columns of D are staged in LDS once per unit (D[s, r] for fixed r is a strided read, L elements per
// L x L slab of u).  Global items are raw buffer loads over one slab: the range check returns zero for padding lanes
// and never fetches past the slab; 16-byte items at 8-byte-aligned addresses (odd L).

#include "qs_contract_common.h"

namespace qs {

constexpr int kMfRows = 8;            // TA: rows of a tile per thread = global items in flight per thread and r
constexpr int kMfChunkTarget = 4096;  // work units aimed at for P = L: cdiv(4096, L) chunks of r (at most R)
constexpr int kMfStageWords = 2048;   // doubles of LDS for the chunk's columns of D (one column always fits: L <= 1024)

struct MfArgs {
    const double* u;
    const double* D;
    double* part;           // workspace [P][nchunk][L] result elements
    double cj, ck;
    int64_t slab_words;     // doubles of one (p, r) slab
    int L, R, r_lo, Rc, nchunk;
    int ct_log, ncb, nrb;   // CT = 1 << ct_log column threads; tiles: ncb column blocks x nrb row blocks
};

// Chunk length and count: a function of (L, R, dtype of D) only.
static inline void mf_chunks(int64_t L, int64_t R, int dw, int* Rc, int* nchunk) {
    const int64_t Ls = (L + 1) & ~int64_t(1);
    const int64_t want = cdiv(kMfChunkTarget, L) < R ? cdiv(kMfChunkTarget, L) : R;
    int64_t rc = cdiv(R, want);
    const int64_t fit = kMfStageWords / (Ls * dw) > 1 ? kMfStageWords / (Ls * dw) : 1;
    if (rc > fit) rc = fit;
    *Rc = (int)rc;
    *nchunk = (int)cdiv(R, rc);
}

// FORM 0: u, D, W real; 1: all complex128; 2: real u, complex D and W (two real accumulations from one load).
template <int FORM, bool DOJ, bool DOK>
__global__ __launch_bounds__(256) void mean_field_kernel(const MfArgs g) {
    constexpr auto W = form_widths(FORM);
    constexpr int UW = W.uw, AW = W.aw, CPI = W.cpi;      // (CPI columns per item = K sums per thread)
    constexpr int TA = kMfRows;
    extern __shared__ __attribute__((aligned(16))) double mf_lds[];

    const int L = g.L, Ls = (L + 1) & ~1, tid = threadIdx.x;
    const int CT = 1 << g.ct_log, RT = 256 >> g.ct_log, RB = RT * TA, WPR = CT > 64 ? CT >> 6 : 1;
    const int tc = tid & (CT - 1), tr = tid >> g.ct_log;
    const unsigned chunk = blockIdx.x % (unsigned)g.nchunk, p = blockIdx.x / (unsigned)g.nchunk;
    const int r0 = (int)chunk * g.Rc, rn = g.R - r0 < g.Rc ? g.R - r0 : g.Rc;

    double* Dc = mf_lds;                                // [rn][Ls] columns of D, zero beyond L
    double* Jl = Dc + (size_t)g.Rc * Ls * AW;           // [nrb * RB]
    double* Kl = Jl + (size_t)g.nrb * RB * AW;          // [ncb * CT * CPI]
    double* redJ = Kl + (size_t)g.ncb * CT * CPI * AW;  // [RB][WPR]
    double* redK = redJ + (size_t)RB * WPR * AW;        // [256][CPI]

    for (int idx = tid; idx < rn * Ls; idx += 256) {
        const int rr = idx % rn, s = idx / rn;
#pragma unroll
        for (int w = 0; w < AW; ++w)
            Dc[(size_t)(rr * Ls + s) * AW + w] = s < L ? g.D[((int64_t)s * L + g.r_lo + r0 + rr) * AW + w] : 0.0;
    }
    for (int idx = tid; idx < (g.nrb * RB + g.ncb * CT * CPI) * AW; idx += 256) Jl[idx] = 0.0;
    __syncthreads();

    const unsigned room = (unsigned)(g.slab_words * 8);
    const uint64_t u0 = uniform64(reinterpret_cast<uint64_t>(g.u) + ((uint64_t)p * g.R + r0) * (uint64_t)g.slab_words * 8);

    for (int cb = 0; cb < g.ncb; ++cb) {
        const int b0 = (cb * CT + tc) * CPI;
        const bool colok = b0 < L, full = b0 + 1 < L;
        for (int rb = 0; rb < g.nrb; ++rb) {
            unsigned off[TA];
            bool rowok[TA];
            int row[TA];
#pragma unroll
            for (int i = 0; i < TA; ++i) {
                row[i] = rb * RB + i * RT + tr;
                rowok[i] = row[i] < L;
                off[i] = (rowok[i] && colok) ? (unsigned)(row[i] * L + b0) * (UW * 8) : room;
                if (!rowok[i]) row[i] = 0;
            }
            double J[TA][AW], K[CPI][AW];
#pragma unroll
            for (int i = 0; i < TA; ++i)
#pragma unroll
                for (int w = 0; w < AW; ++w) J[i][w] = 0.0;
#pragma unroll
            for (int k = 0; k < CPI; ++k)
#pragma unroll
                for (int w = 0; w < AW; ++w) K[k][w] = 0.0;

            f64x2 cur[TA], nxt[TA];
#pragma unroll
            for (int i = 0; i < TA; ++i) nxt[i] = cur[i] = FastItem<true>::load(u0, room, off[i]);
            for (int rr = 0; rr < rn; ++rr) {
                if (rr + 1 < rn) {
                    const uint64_t base = u0 + (uint64_t)(rr + 1) * (uint64_t)g.slab_words * 8;
#pragma unroll
                    for (int i = 0; i < TA; ++i) nxt[i] = FastItem<true>::load(base, room, off[i]);
                }
                const double* dcol = Dc + (size_t)rr * Ls * AW;
                // D[b, r] of this thread's columns (zero for padding columns: nothing times them may become NaN)
                double d[CPI][AW];
#pragma unroll
                for (int k = 0; k < CPI; ++k)
#pragma unroll
                    for (int w = 0; w < AW; ++w) d[k][w] = colok ? dcol[(size_t)(b0 + k) * AW + w] : 0.0;
#pragma unroll
                for (int i = 0; i < TA; ++i) {
                    f64x2 v = cur[i];
                    if (FORM != 1 && !full) v.y = 0.0;        // odd L: the item's second half is the next row's
                    if (DOJ) {
                        if (FORM == 0) {
                            J[i][0] += v.x * d[0][0] + v.y * d[CPI - 1][0];
                        } else if (FORM == 2) {
                            J[i][0] += v.x * d[0][0] + v.y * d[CPI - 1][0];
                            J[i][1] += v.x * d[0][AW - 1] + v.y * d[CPI - 1][AW - 1];
                        } else {
                            J[i][0] += v.x * d[0][0] - v.y * d[0][AW - 1];
                            J[i][AW - 1] += v.x * d[0][AW - 1] + v.y * d[0][0];
                        }
                    }
                    if (DOK) {
                        double da[AW];
#pragma unroll
                        for (int w = 0; w < AW; ++w) da[w] = rowok[i] ? dcol[(size_t)row[i] * AW + w] : 0.0;
                        if (FORM == 0) {
                            K[0][0] += v.x * da[0];
                            K[CPI - 1][0] += v.y * da[0];
                        } else if (FORM == 2) {
                            K[0][0] += v.x * da[0];
                            K[0][AW - 1] += v.x * da[AW - 1];
                            K[CPI - 1][0] += v.y * da[0];
                            K[CPI - 1][AW - 1] += v.y * da[AW - 1];
                        } else {
                            K[0][0] += v.x * da[0] - v.y * da[AW - 1];
                            K[0][AW - 1] += v.x * da[AW - 1] + v.y * da[0];
                        }
                    }
                }
#pragma unroll
                for (int i = 0; i < TA; ++i) cur[i] = nxt[i];
            }

            // close the tile: J over the column threads of a row, K over the row threads of a column, fixed order
            if (DOJ) {
                const int span = CT < 64 ? CT : 64;
#pragma unroll
                for (int i = 0; i < TA; ++i)
#pragma unroll
                    for (int w = 0; w < AW; ++w) {
                        double x = J[i][w];
                        for (int m = span >> 1; m >= 1; m >>= 1) x += __shfl_xor(x, m);
                        if ((tc & 63) == 0) redJ[(size_t)((i * RT + tr) * WPR + (tc >> 6)) * AW + w] = x;
                    }
            }
            if (DOK) {
#pragma unroll
                for (int k = 0; k < CPI; ++k)
#pragma unroll
                    for (int w = 0; w < AW; ++w) redK[(size_t)(tid * CPI + k) * AW + w] = K[k][w];
            }
            __syncthreads();
            if (DOJ && tid < RB) {
#pragma unroll
                for (int w = 0; w < AW; ++w) {
                    double x = 0.0;
                    for (int h = 0; h < WPR; ++h) x += redJ[(size_t)(tid * WPR + h) * AW + w];
                    Jl[(size_t)(rb * RB + tid) * AW + w] += x;
                }
            }
            if (DOK && tid < CT) {
#pragma unroll
                for (int k = 0; k < CPI; ++k)
#pragma unroll
                    for (int w = 0; w < AW; ++w) {
                        double x = 0.0;
                        for (int t = 0; t < RT; ++t) x += redK[(size_t)((t * CT + tid) * CPI + k) * AW + w];
                        Kl[(size_t)((cb * CT + tid) * CPI + k) * AW + w] += x;
                    }
            }
            __syncthreads();
        }
    }

    double* dst = g.part + ((size_t)p * g.nchunk + chunk) * (size_t)L * AW;
    for (int idx = tid; idx < L * AW; idx += 256) {
        double x = 0.0;
        if (DOJ) x = g.cj * Jl[idx];
        if (DOK) x = DOJ ? x + g.ck * Kl[idx] : g.ck * Kl[idx];
        dst[idx] = x;
    }
}

// W[p][j] = sum over the chunks, ascending: one thread per real word of the result.
__global__ __launch_bounds__(256) void mean_field_close_kernel(const double* __restrict__ part, double* __restrict__ W,
                                                               int64_t total, int row_words, int nchunk) {
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= total) return;
    const int64_t p = idx / row_words, j = idx - p * row_words;
    const double* src = part + p * nchunk * (int64_t)row_words + j;
    double x = src[0];
    for (int c = 1; c < nchunk; ++c) x += src[(int64_t)c * row_words];
    W[idx] = x;
}

int mean_field_close(const double* part, double* W, int64_t total, int row_words, int nchunk, hipStream_t s) {
    hipLaunchKernelGGL(mean_field_close_kernel, dim3((unsigned)cdiv(total, 256)), dim3(256), 0, s, part, W, total,
                       row_words, nchunk);
    note_dispatch("qs::mean_field_close_kernel");
    return launch_status("mean field close launch");
}

template <int FORM>
static void mf_launch(const MfArgs& g, unsigned grid, size_t lds, hipStream_t s) {
    const bool j = g.cj != 0.0, k = g.ck != 0.0;
    if (j && k) {
        hipLaunchKernelGGL((mean_field_kernel<FORM, true, true>), dim3(grid), dim3(256), lds, s, g);
        note_dispatch("qs::mean_field_kernel<%d, true, true>", FORM);
    } else if (k) {
        hipLaunchKernelGGL((mean_field_kernel<FORM, false, true>), dim3(grid), dim3(256), lds, s, g);
        note_dispatch("qs::mean_field_kernel<%d, false, true>", FORM);
    } else {
        // (cj == ck == 0: the J form, scaled by zero)
        hipLaunchKernelGGL((mean_field_kernel<FORM, true, false>), dim3(grid), dim3(256), lds, s, g);
        note_dispatch("qs::mean_field_kernel<%d, true, false>", FORM);
    }
}

// The launch geometry of one call: everything the kernel reads from MfArgs apart from the pointers, the weights and
// r_lo, its dynamic LDS in bytes and its grid -- a function of (form, L, P, R); all but the grid of (form, L, R) only.
// The entry, the workspace query and the plan hook all take it from here.
static inline void mf_plan(int form, int64_t L, int64_t P, int64_t R, MfArgs* g, size_t* lds, unsigned* grid) {
    const FormWidths w = form_widths(form);
    const MfTiles t = mf_tiles(L, w.cpi, kMfRows);
    g->slab_words = L * L * w.uw;
    g->L = (int)L; g->R = (int)R;
    mf_chunks(L, R, w.aw, &g->Rc, &g->nchunk);
    g->ct_log = t.ct_log; g->ncb = t.ncb; g->nrb = t.nrb;
    const int64_t wpr = t.ct > 64 ? t.ct >> 6 : 1;
    *lds = (size_t)(g->Rc * t.Ls + t.nrb * t.rb + t.ncb * t.ct * w.cpi + t.rb * wpr + 256 * w.cpi) * w.aw * 8;
    *grid = (unsigned)(P * g->nchunk);
}

}  // namespace qs

using namespace qs;

extern "C" {

int64_t qs_mean_field_workspace(int u_dtype, int d_dtype, int64_t L, int64_t P, int64_t R) {
    const int form = tensor_form(u_dtype, d_dtype);
    if (form < 0) return form;
    if (!mf_extents_ok(L, P, R)) return QS_ERR_BAD_EXTENT;
    MfArgs g{};
    size_t lds;
    unsigned grid;
    mf_plan(form, L, P, R, &g, &lds, &grid);
    return P * L * g.nchunk * (int64_t)elem_size(d_dtype);
}

int qs_mean_field_plan(int u_dtype, int d_dtype, int64_t L, int64_t P, int64_t R, int64_t* out, int n_out) {
    const int form = tensor_form(u_dtype, d_dtype);
    if (form < 0) return form;
    if (!mf_extents_ok(L, P, R) || n_out < 7) return QS_ERR_BAD_EXTENT;
    if (!out) return QS_ERR_NULL_POINTER;
    MfArgs g{};
    size_t lds;
    unsigned grid;
    mf_plan(form, L, P, R, &g, &lds, &grid);
    const int64_t plan[7] = {g.Rc, g.nchunk, g.ct_log, g.ncb, g.nrb, (int64_t)lds, (int64_t)grid};
    for (int i = 0; i < 7; ++i) out[i] = plan[i];
    return 0;
}

int qs_mean_field(int u_dtype, int d_dtype, const void* u_slab, const void* D, void* W, int64_t L, int64_t P,
                  int64_t R, int64_t r_lo, double cj, double ck, void* workspace, int64_t workspace_bytes,
                  void* stream) {
    dispatch_reset();
    const int form = tensor_form(u_dtype, d_dtype);
    if (form < 0) return form;
    if (!mf_extents_ok(L, P, R) || r_lo < 0 || r_lo + R > L) return QS_ERR_BAD_EXTENT;
    if (!u_slab || !D || !W || !workspace) return QS_ERR_NULL_POINTER;
    const int64_t es = (int64_t)elem_size(d_dtype), ues = (int64_t)elem_size(u_dtype);
    if (!aligned(u_slab, (size_t)ues) || !aligned(D, (size_t)es) || !aligned(W, (size_t)es) || !aligned(workspace, 16))
        return QS_ERR_MISALIGNED;
    const int64_t need = qs_mean_field_workspace(u_dtype, d_dtype, L, P, R);
    if (overlaps(W, P * L * es, u_slab, P * R * L * L * ues) || overlaps(W, P * L * es, D, L * L * es) ||
        overlaps(W, P * L * es, workspace, need))
        return QS_ERR_ALIAS;
    if (workspace_bytes < need) return QS_ERR_WORKSPACE;

    MfArgs g{};
    size_t lds;
    unsigned grid;
    mf_plan(form, L, P, R, &g, &lds, &grid);
    if (lds > 64 * 1024) return QS_ERR_BAD_EXTENT;      // (not reached for L <= 1024)
    g.u = (const double*)u_slab; g.D = (const double*)D; g.part = (double*)workspace;
    g.cj = cj; g.ck = ck;
    g.r_lo = (int)r_lo;
    hipStream_t s = (hipStream_t)stream;
    with_form(form, [&](auto F) { mf_launch<F>(g, grid, lds, s); });
    const int rc = launch_status("mean field launch");
    if (rc) return rc;
    const int64_t row_words = L * form_widths(form).aw;
    return mean_field_close((const double*)workspace, (double*)W, P * row_words, (int)row_words, g.nchunk, s);
}

}  // extern "C"
