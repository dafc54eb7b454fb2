// Mean field of SEVERAL one-body densities from one read of u:
//   W_k[p,q] = cj_k * sum_{r,s} u[p,r,q,s] D_k[s,r]  +  ck_k * sum_{r,s} u[p,r,s,q] D_k[s,r],   k = 0 ... ND-1.
// qs_mean_field.hip reads u at the HBM roof and leaves the fp64 VALU ~30x idle; a Davidson step (CIS) needs the same
// contraction for a handful of trial densities.  Here every 16-byte item of u is loaded once per GROUP of G densities
// and feeds all 2 G running sums (J and K of each density) while it sits in a register.
//
// The design is qs_mean_field.hip's: work unit = (row p, chunk of Rc consecutive r), one workgroup of 256 threads as a
// (RT x CT) grid over a tile of the L x L slab u[p,r,:,:], CT column threads of one 16-byte item and RT = 256 / CT row
// threads of TA rows each.  A thread keeps its positions of the tile and streams over the chunk's r with TA x G J sums
// and CPI x G K sums in registers; raw buffer loads, out of range = zero, 16-byte items at 8-byte alignment (odd L).
// The chunk's columns of every D_k of the group are staged in LDS as [r][s][g]: the G values a product needs are
// adjacent.  After the chunk's last r the tile is closed once, in a fixed order: J by an xor butterfly over the column
// threads of a wave, K by one over the row threads a wave holds (CT < 64), then wave after wave adds its sums to the
// unit's J[L][G] / K[L][G] in LDS.  The unit stores cj_k J_k + ck_k K_k to the workspace, [k][p][chunk][q]; one closing
// launch adds the chunks of every (k, p) in ascending order.  No floating-point atomics.
//
// Reproducible across batches: every product is an explicit fma in a fixed order, and the chunk split and the tile
// geometry depend on (L, R, dtypes) only -- not on ND, on a density's position, or on the instantiation its group runs
// on (a partial last group takes the smallest instantiation that holds it).  So W_k has the same bits alone and
// anywhere in a batch of any size.  Both sums of every density are always accumulated (the arithmetic hides under the
// load stream); a zero weight drops its sum where the unit stores, so a NaN in a sum that is not asked for stays out.

#include "qs_contract_common.h"

namespace qs {

constexpr int kMfbRows = 4;                     // TA: rows of a tile per thread (qs_mean_field.hip: 8; the G-fold sums need the room)
constexpr int kMfbChunkTarget = 4096;           // work units aimed at for P = L, as qs_mean_field.hip
constexpr int kMfbLdsWords = 8192;             // doubles of LDS a workgroup may carve: 64 KB, two workgroups per CU (160 KB)
constexpr int kMfbMaxG = 8;
// Shipped group size per form {fp64, complex128, mixed}: the largest G of the form that keeps two workgroups per CU in
// VGPRs and in LDS (DESIGN.md 3.4b has the code-object figures and what was timed).
constexpr int kMfbGroup[3] = {8, 4, 4};

struct MfbArgs {
    const double* u;
    const double* D;          // first density of the group, [ng][L][L]
    double* part;             // workspace of the group's first density, [ng][P][nchunk][L] result elements
    double cj[kMfbMaxG], ck[kMfbMaxG];
    int64_t slab_words;       // doubles of one (p, r) slab
    int64_t d_words;          // doubles of one density
    int64_t part_words;       // doubles of one density's part of the workspace
    int L, R, r_lo, Rc, nchunk;
    int ct_log, ncb, nrb;     // CT = 1 << ct_log column threads; tiles: ncb column blocks x nrb row blocks
    int ng;                   // densities of this launch, 1 ... G of the instantiation
};

struct MfbPlan {
    int G, Rc, nchunk, ct_log, ncb, nrb;
};

static inline MfTiles mfb_tiles(int form, int64_t L) { return mf_tiles(L, form_widths(form).cpi, kMfbRows); }

// LDS doubles of a unit that stages `rc` columns for `G` densities.
static inline int64_t mfb_lds_words(const MfTiles& t, int form, int64_t rc, int G) {
    const FormWidths w = form_widths(form);
    return (rc * t.Ls + t.nrb * t.rb + t.ncb * t.ct * w.cpi) * G * w.aw;
}

// Everything the kernel's geometry rests on: a function of (form, L, R) and the form's group size only.  The group
// size is lowered (halved) for the L at which one column of every density and the unit's sums no longer fit the LDS.
static inline MfbPlan mfb_plan(const MfTiles& t, int form, int64_t L, int64_t R, int group) {
    MfbPlan pl{};
    pl.ct_log = t.ct_log; pl.ncb = t.ncb; pl.nrb = t.nrb;
    int G = group;
    while (G > 1 && mfb_lds_words(t, form, 1, G) > kMfbLdsWords) G >>= 1;
    pl.G = G;
    const int64_t want = cdiv(kMfbChunkTarget, L) < R ? cdiv(kMfbChunkTarget, L) : R;
    int64_t rc = cdiv(R, want);
    while (rc > 1 && mfb_lds_words(t, form, rc, G) > kMfbLdsWords) --rc;
    pl.Rc = (int)rc;
    pl.nchunk = (int)cdiv(R, rc);
    return pl;
}

// FORM 0: u, D, W real; 1: all complex128; 2: real u, complex D and W.  G: densities per load of u.
template <int FORM, int G>
__global__ __launch_bounds__(256) void mean_field_batch_kernel(const MfbArgs g) {
    constexpr auto W = form_widths(FORM);
    constexpr int UW = W.uw, AW = W.aw, CPI = W.cpi;      // (CPI columns per item = K sums per thread and density)
    constexpr int TA = kMfbRows;
    extern __shared__ __attribute__((aligned(16))) double mfb_lds[];

    const int L = g.L, Ls = (L + 1) & ~1, tid = threadIdx.x;
    const int CT = 1 << g.ct_log, RT = 256 >> g.ct_log, RB = RT * TA;
    const int tc = tid & (CT - 1), tr = tid >> g.ct_log;
    const unsigned chunk = blockIdx.x % (unsigned)g.nchunk, p = blockIdx.x / (unsigned)g.nchunk;
    const int r0 = (int)chunk * g.Rc, rn = g.R - r0 < g.Rc ? g.R - r0 : g.Rc;

    double* Dc = mfb_lds;                                  // [rn][Ls][G] columns of the D_k, zero beyond L and beyond ng
    double* Jl = Dc + (size_t)g.Rc * Ls * G * AW;          // [nrb * RB][G]
    double* Kl = Jl + (size_t)g.nrb * RB * G * AW;         // [ncb * CT * CPI][G]

    for (int idx = tid; idx < rn * G * Ls; idx += 256) {
        const int rr = idx % rn, t = idx / rn, gg = t % G, s = t / G;
        const bool ok = s < L && gg < g.ng;
        const double* src = g.D + (ok ? (int64_t)gg * g.d_words + ((int64_t)s * L + g.r_lo + r0 + rr) * AW : 0);
#pragma unroll
        for (int w = 0; w < AW; ++w) Dc[((size_t)(rr * Ls + s) * G + gg) * AW + w] = ok ? src[w] : 0.0;
    }
    for (int idx = tid; idx < (g.nrb * RB + g.ncb * CT * CPI) * G * AW; idx += 256) Jl[idx] = 0.0;
    __syncthreads();

    const unsigned room = (unsigned)(g.slab_words * 8);
    const uint64_t u0 = uniform64(reinterpret_cast<uint64_t>(g.u) + ((uint64_t)p * g.R + r0) * (uint64_t)g.slab_words * 8);
    // the four waves take turns adding to the unit's sums.  J: lane 0 of every CT-lane row segment holds its sum.
    // K: CT >= 64: row thread tr adds in turn tr (RT <= 4); CT < 64: a wave's butterfly has closed its 64 / CT row threads
    constexpr int turns = 4;

    for (int cb = 0; cb < g.ncb; ++cb) {
        const int b0 = (cb * CT + tc) * CPI;
        const bool colok = b0 < L, full = b0 + 1 < L;
        const int bl = colok ? b0 : 0;
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
            double J[TA][G][AW], K[CPI][G][AW];
#pragma unroll
            for (int i = 0; i < TA; ++i)
#pragma unroll
                for (int q = 0; q < G; ++q)
#pragma unroll
                    for (int w = 0; w < AW; ++w) J[i][q][w] = 0.0;
#pragma unroll
            for (int k = 0; k < CPI; ++k)
#pragma unroll
                for (int q = 0; q < G; ++q)
#pragma unroll
                    for (int w = 0; w < AW; ++w) K[k][q][w] = 0.0;

            f64x2 cur[TA], nxt[TA];
#pragma unroll
            for (int i = 0; i < TA; ++i) nxt[i] = cur[i] = FastItem<true>::load(u0, room, off[i]);
            for (int rr = 0; rr < rn; ++rr) {
                if (rr + 1 < rn) {
                    const uint64_t base = u0 + (uint64_t)(rr + 1) * (uint64_t)g.slab_words * 8;
#pragma unroll
                    for (int i = 0; i < TA; ++i) nxt[i] = FastItem<true>::load(base, room, off[i]);
                }
                const double* dcol = Dc + (size_t)rr * Ls * G * AW;
                // D_k[b, r] of this thread's columns (zero for padding columns: nothing times them may become NaN)
                double d[CPI][G][AW];
#pragma unroll
                for (int k = 0; k < CPI; ++k)
#pragma unroll
                    for (int q = 0; q < G; ++q)
#pragma unroll
                        for (int w = 0; w < AW; ++w) {
                            const double x = dcol[((size_t)(bl + k) * G + q) * AW + w];
                            d[k][q][w] = colok ? x : 0.0;
                        }
#pragma unroll
                for (int i = 0; i < TA; ++i) {
                    f64x2 v = cur[i];
                    if (FORM != 1 && !full) v.y = 0.0;        // odd L: the item's second half is the next row's
                    const double* drow = dcol + (size_t)row[i] * G * AW;
#pragma unroll
                    for (int q = 0; q < G; ++q) {
                        double da[AW];
#pragma unroll
                        for (int w = 0; w < AW; ++w) da[w] = rowok[i] ? drow[q * AW + w] : 0.0;
                        if (FORM == 0) {
                            J[i][q][0] = fma(v.y, d[CPI - 1][q][0], fma(v.x, d[0][q][0], J[i][q][0]));
                            K[0][q][0] = fma(v.x, da[0], K[0][q][0]);
                            K[CPI - 1][q][0] = fma(v.y, da[0], K[CPI - 1][q][0]);
                        } else if (FORM == 2) {
#pragma unroll
                            for (int w = 0; w < AW; ++w) {
                                J[i][q][w] = fma(v.y, d[CPI - 1][q][w], fma(v.x, d[0][q][w], J[i][q][w]));
                                K[0][q][w] = fma(v.x, da[w], K[0][q][w]);
                                K[CPI - 1][q][w] = fma(v.y, da[w], K[CPI - 1][q][w]);
                            }
                        } else {
                            J[i][q][0] = fma(-v.y, d[0][q][AW - 1], fma(v.x, d[0][q][0], J[i][q][0]));
                            J[i][q][AW - 1] = fma(v.y, d[0][q][0], fma(v.x, d[0][q][AW - 1], J[i][q][AW - 1]));
                            K[0][q][0] = fma(-v.y, da[AW - 1], fma(v.x, da[0], K[0][q][0]));
                            K[0][q][AW - 1] = fma(v.y, da[0], fma(v.x, da[AW - 1], K[0][q][AW - 1]));
                        }
                    }
                }
#pragma unroll
                for (int i = 0; i < TA; ++i) cur[i] = nxt[i];
            }

            // close the tile in a fixed order: J over the column threads of a wave, K over the row threads of a wave
            {
                const int span = CT < 64 ? CT : 64;
#pragma unroll
                for (int i = 0; i < TA; ++i)
#pragma unroll
                    for (int q = 0; q < G; ++q)
#pragma unroll
                        for (int w = 0; w < AW; ++w) {
                            double x = J[i][q][w];
                            for (int m = span >> 1; m >= 1; m >>= 1) x += __shfl_xor(x, m);
                            J[i][q][w] = x;
                        }
                if (CT < 64) {
#pragma unroll
                    for (int k = 0; k < CPI; ++k)
#pragma unroll
                        for (int q = 0; q < G; ++q)
#pragma unroll
                            for (int w = 0; w < AW; ++w) {
                                double x = K[k][q][w];
                                for (int m = 32; m >= CT; m >>= 1) x += __shfl_xor(x, m);
                                K[k][q][w] = x;
                            }
                }
            }
            // ... then the waves one after the other add to the unit's sums
            for (int t = 0; t < turns; ++t) {
                if ((tid >> 6) == t && (tc & 63) == 0) {
                    // the row threads this lane closed: CT >= 64 one row thread per wave, else 64 / CT of them
#pragma unroll
                    for (int i = 0; i < TA; ++i)
#pragma unroll
                        for (int q = 0; q < G; ++q)
#pragma unroll
                            for (int w = 0; w < AW; ++w)
                                Jl[((size_t)(rb * RB + i * RT + tr) * G + q) * AW + w] += J[i][q][w];
                }
                if (CT >= 64 ? tr == t : ((tid >> 6) == t && (tid & 63) < CT)) {
#pragma unroll
                    for (int k = 0; k < CPI; ++k)
#pragma unroll
                        for (int q = 0; q < G; ++q)
#pragma unroll
                            for (int w = 0; w < AW; ++w)
                                Kl[((size_t)((cb * CT + tc) * CPI + k) * G + q) * AW + w] += K[k][q][w];
                }
                __syncthreads();
            }
        }
    }

    for (int gg = 0; gg < g.ng; ++gg) {
        const double cj = g.cj[gg], ck = g.ck[gg];
        double* dst = g.part + (size_t)gg * g.part_words + ((size_t)p * g.nchunk + chunk) * (size_t)L * AW;
        for (int idx = tid; idx < L * AW; idx += 256) {
            const int q = idx / AW, w = idx - q * AW;
            double x = 0.0;
            if (cj != 0.0) x = cj * Jl[((size_t)q * G + gg) * AW + w];
            if (ck != 0.0) {
                const double kk = Kl[((size_t)q * G + gg) * AW + w];
                x = cj != 0.0 ? fma(ck, kk, x) : ck * kk;
            }
            dst[idx] = x;
        }
    }
}

// One group of g.ng densities on the smallest instantiation that holds it; the LDS size follows that instantiation.
static void mfb_launch(int form, const MfbArgs& g, const MfTiles& t, int rc, unsigned grid, hipStream_t s) {
    with_form(form, [&](auto F) {
        with_group(g.ng, [&](auto G) {
            const size_t lds = (size_t)mfb_lds_words(t, F, rc, G) * 8;
            hipLaunchKernelGGL((mean_field_batch_kernel<F, G>), dim3(grid), dim3(256), lds, s, g);
            note_dispatch("qs::mean_field_batch_kernel<%d, %d>", (int)F, (int)G);
        });
    });
}

// The form's group size: the shipped one, or the tuning run's (mean_field_batch_g = 1, 2, 4, 8).
static inline int mfb_group(int form) { return group_size(g_tune.mean_field_batch_g, kMfbGroup[form]); }

}  // namespace qs

using namespace qs;

extern "C" {

int64_t qs_mean_field_batch_workspace(int u_dtype, int d_dtype, int64_t L, int64_t P, int64_t R, int64_t ND) {
    const int form = tensor_form(u_dtype, d_dtype);
    if (form < 0) return form;
    if (!mf_extents_ok(L, P, R, ND)) return QS_ERR_BAD_EXTENT;
    const MfbPlan pl = mfb_plan(mfb_tiles(form, L), form, L, R, mfb_group(form));
    return ND * P * L * pl.nchunk * (int64_t)elem_size(d_dtype);
}

int qs_mean_field_batch_plan(int u_dtype, int d_dtype, int64_t L, int64_t P, int64_t R, int64_t ND, int64_t* out,
                             int n_out) {
    const int form = tensor_form(u_dtype, d_dtype);
    if (form < 0) return form;
    if (!mf_extents_ok(L, P, R, ND) || n_out < 9) return QS_ERR_BAD_EXTENT;
    if (!out) return QS_ERR_NULL_POINTER;
    const MfTiles t = mfb_tiles(form, L);
    const MfbPlan pl = mfb_plan(t, form, L, R, mfb_group(form));
    const int64_t plan[9] = {pl.G, cdiv(ND, pl.G), pl.Rc, pl.nchunk, pl.ct_log, pl.ncb, pl.nrb,
                             mfb_lds_words(t, form, pl.Rc, pl.G) * 8, P * pl.nchunk};
    for (int i = 0; i < 9; ++i) out[i] = plan[i];
    return 0;
}

int qs_mean_field_batch(int u_dtype, int d_dtype, const void* u_slab, const void* D, void* W, int64_t L, int64_t P,
                        int64_t R, int64_t r_lo, int64_t ND, const double* cj, const double* ck, void* workspace,
                        int64_t workspace_bytes, void* stream) {
    dispatch_reset();
    const int form = tensor_form(u_dtype, d_dtype);
    if (form < 0) return form;
    if (!mf_extents_ok(L, P, R, ND) || r_lo < 0 || r_lo + R > L) return QS_ERR_BAD_EXTENT;
    if (!u_slab || !D || !W || !workspace || !cj || !ck) return QS_ERR_NULL_POINTER;
    const int64_t es = (int64_t)elem_size(d_dtype), ues = (int64_t)elem_size(u_dtype);
    if (!aligned(u_slab, (size_t)ues) || !aligned(D, (size_t)es) || !aligned(W, (size_t)es) || !aligned(workspace, 16))
        return QS_ERR_MISALIGNED;
    const int64_t need = qs_mean_field_batch_workspace(u_dtype, d_dtype, L, P, R, ND);
    const int64_t w_bytes = ND * P * L * es;
    if (overlaps(W, w_bytes, u_slab, P * R * L * L * ues) || overlaps(W, w_bytes, D, ND * L * L * es) ||
        overlaps(W, w_bytes, workspace, need))
        return QS_ERR_ALIAS;
    if (workspace_bytes < need) return QS_ERR_WORKSPACE;

    const MfTiles t = mfb_tiles(form, L);
    const MfbPlan pl = mfb_plan(t, form, L, R, mfb_group(form));
    if (mfb_lds_words(t, form, pl.Rc, pl.G) > kMfbLdsWords) return QS_ERR_BAD_EXTENT;      // (not reached for L <= 1024)
    const FormWidths w = form_widths(form);
    MfbArgs g{};
    g.u = (const double*)u_slab;
    g.slab_words = L * L * w.uw;
    g.d_words = L * L * w.aw;
    g.part_words = P * pl.nchunk * L * w.aw;
    g.L = (int)L; g.R = (int)R; g.r_lo = (int)r_lo;
    g.Rc = pl.Rc; g.nchunk = pl.nchunk; g.ct_log = pl.ct_log; g.ncb = pl.ncb; g.nrb = pl.nrb;
    const unsigned grid = (unsigned)(P * pl.nchunk);
    hipStream_t s = (hipStream_t)stream;
    const int rc = for_each_group(ND, pl.G, [&](int64_t k0, int ng) {
        g.ng = ng;
        g.D = (const double*)D + k0 * g.d_words;
        g.part = (double*)workspace + k0 * g.part_words;
        for (int q = 0; q < kMfbMaxG; ++q) {
            g.cj[q] = q < ng ? cj[k0 + q] : 0.0;
            g.ck[q] = q < ng ? ck[k0 + q] : 0.0;
        }
        mfb_launch(form, g, t, pl.Rc, grid, s);
        return launch_status("mean field batch launch");
    });
    if (rc) return rc;
    const int64_t row_words = L * w.aw;
    return mean_field_close((const double*)workspace, (double*)W, ND * P * row_words, (int)row_words, pl.nchunk, s);
}

}  // extern "C"
