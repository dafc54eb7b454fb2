// What the streamed contractions share (qs_mean_field.hip, qs_mean_field_batch.hip, qs_pair_contract.hip,
// qs_pair_contract_antisym.hip, qs_pair_contract_exchange.hip, qs_lead_contract.hip, qs_det_ci.hip): the dtype pair -> form rule and the widths a form implies, the group size and
// the dispatch of a run-time form / group size to a kernel instantiation, the loop over the groups of a batch, and the
// tile arithmetic and the closing launch of the two mean-field kernels.  What only the three pair contractions share
// (the closing butterfly, the chunk loop, the launch, the packed-triangle walk and its C entry) is in qs_pair_walk.h.
#pragma once

#include <type_traits>

#include "qs_fast_items.h"

namespace qs {

// The kernel form of a (tensor, coefficient) dtype pair: the tensor real or complex, the coefficients at least as
// complex.  0: both fp64; 1: both complex128; 2: real tensor, complex coefficients and result (two real accumulations
// from one load); negative = the pair is refused.
inline int tensor_form(int tensor_dtype, int coeff_dtype) {
    if (!dtype_ok(tensor_dtype) || !dtype_ok(coeff_dtype) || (tensor_dtype == QS_C128 && coeff_dtype == QS_F64))
        return QS_ERR_BAD_DTYPE;
    return tensor_dtype == QS_C128 ? 1 : (coeff_dtype == QS_C128 ? 2 : 0);
}

struct FormWidths {
    int uw;     // doubles per element of the tensor
    int aw;     // doubles per element of the coefficients and of the result
    int cpi;    // tensor elements (columns) per 16-byte item
};
constexpr FormWidths form_widths(int form) { return {form == 1 ? 2 : 1, form == 0 ? 1 : 2, form == 1 ? 1 : 2}; }

// Vectors per load of the tensor: the tuning run's value (1, 2, 4, 8), otherwise the shipped one of the form.
inline int group_size(int tuned, int shipped) {
    return (tuned == 1 || tuned == 2 || tuned == 4 || tuned == 8) ? tuned : shipped;
}

// f(std::integral_constant<int, FORM>) for the run-time form 0 ... 2.
template <class F>
inline auto with_form(int form, F&& f) {
    if (form == 0) return f(std::integral_constant<int, 0>{});
    if (form == 1) return f(std::integral_constant<int, 1>{});
    return f(std::integral_constant<int, 2>{});
}

// f(std::integral_constant<int, W>) for the run-time width W = 1 or 2 doubles per element.
template <class F>
inline auto with_width(int w, F&& f) {
    if (w == 1) return f(std::integral_constant<int, 1>{});
    return f(std::integral_constant<int, 2>{});
}

// f(std::integral_constant<int, G>) for the smallest instantiation G of 1, 2, 4, 8 that holds ng <= 8 vectors.
template <class F>
inline auto with_group(int ng, F&& f) {
    if (ng <= 1) return f(std::integral_constant<int, 1>{});
    if (ng <= 2) return f(std::integral_constant<int, 2>{});
    if (ng <= 4) return f(std::integral_constant<int, 4>{});
    return f(std::integral_constant<int, 8>{});
}

// f(k0, ng) for every group of up to G of K vectors, ascending; stops at the first status that is not QS_OK.
template <class F>
inline int for_each_group(int64_t K, int G, F&& f) {
    for (int64_t k0 = 0; k0 < K; k0 += G) {
        const int rc = f(k0, (int)(K - k0 < G ? K - k0 : G));
        if (rc) return rc;
    }
    return QS_OK;
}

// ---- the two mean-field kernels: a workgroup of 256 threads as CT column threads x 256 / CT row threads of `rows` rows

// Column threads: the power of two in 8 ... 128 with the least padded tile area (ties: the widest, whole rows per wave).
inline int mf_ct_log(int64_t L, int cpi, int rows) {
    const int64_t items = cdiv(L, cpi);
    int best = 3;
    int64_t best_area = -1;
    for (int lg = 3; lg <= 7; ++lg) {
        const int64_t ct = int64_t(1) << lg, rb = (256 >> lg) * rows;
        const int64_t area = cdiv(items, ct) * ct * cdiv(L, rb) * rb;
        if (best_area < 0 || area <= best_area) { best = lg; best_area = area; }
    }
    return best;
}

// The tiles of an L x L slab: a function of (L, columns per item, rows per thread) only.
struct MfTiles {
    int ct_log, ncb, nrb;   // CT = 1 << ct_log column threads; ncb column blocks x nrb row blocks
    int64_t Ls, ct, rb;     // L rounded up to even; column threads and rows of one tile
};
inline MfTiles mf_tiles(int64_t L, int cpi, int rows) {
    MfTiles t{};
    t.ct_log = mf_ct_log(L, cpi, rows);
    t.ct = int64_t(1) << t.ct_log;
    t.rb = (256 >> t.ct_log) * rows;
    t.ncb = (int)cdiv(cdiv(L, cpi), t.ct);
    t.nrb = (int)cdiv(L, t.rb);
    t.Ls = (L + 1) & ~int64_t(1);
    return t;
}

// A slab of P rows and R second indices of an L-orbital tensor, ND densities.
inline bool mf_extents_ok(int64_t L, int64_t P, int64_t R, int64_t ND = 1) {
    return L > 0 && L <= 1024 && P > 0 && P <= L && R > 0 && R <= L && ND > 0 && ND <= 65536;
}

// W[row][j] = sum over the chunks of part[row][chunk][j], ascending; total = rows * row_words doubles
// (qs_mean_field.hip: mean_field_close_kernel).
int mean_field_close(const double* part, double* W, int64_t total, int row_words, int nchunk, hipStream_t stream);

}  // namespace qs
