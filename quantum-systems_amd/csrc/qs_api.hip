// extern "C" surface of libqs_amd.so (include/qs_amd.h): argument checking,
// workspace carving and the contraction schedule.  No kernels live here.
//
// contraction -> GEMM map for  out = Ct Ct u C C  (basis_set.py:341-348), all
// operands row-major, L = old size, M = new size:
//   d:  T1[(abc), s]   = sum_d u[(abc), d]  C[d, s]        m=rows*L^2 n=M   k=L
//   c:  T2[ab][r, s]   = sum_c CT[r, c]     T1[ab][c, s]   batch rows*L, m=n=M, k=L
//   b:  T3[a][q, (rs)] = sum_b Ct[q, b]     T2[a][b, (rs)] batch rows,   m=M n=M^2 k=L
//   a:  out[p, (qrs)]  = sum_a Ct[p, a]     T3[a, (qrs)]   m=M n=M^3 k=L
// CT = C^T is materialised once (L*M elements) so that every product is the
// same row-major kernel with the tensor streamed along its contiguous axis.

#include <stdarg.h>
#include <stdio.h>
#include <string.h>

#include <mutex>

#include "qs_common.h"
#include "qs_triangle.h"

namespace qs {

static thread_local char g_hip_err[256] = "";

void note_hip_error(hipError_t e, const char* what) {
    snprintf(g_hip_err, sizeof(g_hip_err), "%s: %s", what, hipGetErrorString(e));
}

int current_device() {
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) {
        (void)hipGetLastError();
        return 0;
    }
    return (dev >= 0 && dev < kMaxDevices) ? dev : 0;
}

int device_cu_count() {
    static PerDeviceInt n_cu;
    const int dev = current_device();
    int n = n_cu.v[dev].load(std::memory_order_relaxed);
    if (n == 0) {
        hipDeviceProp_t prop;
        if (hipGetDeviceProperties(&prop, dev) == hipSuccess && prop.multiProcessorCount > 0) {
            n = prop.multiProcessorCount;
        } else {
            (void)hipGetLastError();
            n = 256;   // MI355X
        }
        n_cu.v[dev].store(n, std::memory_order_relaxed);
    }
    return n;
}

int opt_in_dynamic_lds(const void* kern, size_t lds_bytes, PerDeviceLds& seen, const char* what) {
    if (lds_bytes <= 64 * 1024) return QS_OK;
    std::atomic<uint32_t>& top = seen.bytes[current_device()];
    if (top.load(std::memory_order_acquire) >= lds_bytes) return QS_OK;
    // slow path (a first launch, or one that needs more than any before it): serialised, so that the attribute and the
    // record of it cannot end up in different orders when two threads raise the limit at once
    static std::mutex raise;
    std::lock_guard<std::mutex> hold(raise);
    if (top.load(std::memory_order_relaxed) >= lds_bytes) return QS_OK;
    hipError_t e = hipFuncSetAttribute(kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes);
    if (e != hipSuccess) return hip_status(e, what);
    top.store((uint32_t)lds_bytes, std::memory_order_release);
    return QS_OK;
}

int resident_workgroups(const void* kern, PerDeviceInt& cache, int fallback) {
    const int dev = current_device();
    int n = cache.v[dev].load(std::memory_order_relaxed);
    if (n == 0) {
        int nb = 0;
        if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, kern, 256, 0) != hipSuccess || nb < 1) {
            (void)hipGetLastError();
            nb = fallback;
        }
        n = nb > 4 ? 4 : nb;
        cache.v[dev].store(n, std::memory_order_relaxed);
    }
    return n;
}

thread_local Tuning g_tune;

static thread_local char g_dispatch[4096] = "";
static thread_local size_t g_dispatch_len = 0;

void dispatch_reset() {
    g_dispatch[0] = 0;
    g_dispatch_len = 0;
}

void note_dispatch(const char* fmt, ...) {
    char name[160];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(name, sizeof(name), fmt, ap);
    va_end(ap);
    // "name xN" run-length form: the four contractions of a large transform are one kernel
    const size_t nl = strlen(name);
    char* last = strrchr(g_dispatch, ';');
    last = last ? last + 1 : g_dispatch;
    if (g_dispatch_len && !strncmp(last, name, nl) && (last[nl] == 0 || !strncmp(last + nl, " x", 2))) {
        const int count = last[nl] ? atoi(last + nl + 2) + 1 : 2;
        const size_t room = sizeof(g_dispatch) - (size_t)(last - g_dispatch);
        if (nl + 16 < room) {
            snprintf(last + nl, room - nl, " x%d", count);
            g_dispatch_len = strlen(g_dispatch);
        }
        return;
    }
    if (g_dispatch_len + nl + 2 >= sizeof(g_dispatch)) return;
    if (g_dispatch_len) g_dispatch[g_dispatch_len++] = ';';
    memcpy(g_dispatch + g_dispatch_len, name, nl + 1);
    g_dispatch_len += nl;
}

int matmul_real_by_complex(const void* A, const void* B, void* out, int64_t m, int64_t n, int64_t k, hipStream_t stream) {
    return gemm(packed(QS_F64, A, B, out, m, 2 * n, k), stream);
}

int gemm_d(int in_dtype, int dtype, const void* u, const void* C, void* T1, int64_t rows3, int64_t L, int64_t M, hipStream_t s) {
    if (in_dtype == dtype) return gemm(packed(dtype, u, C, T1, rows3, M, L), s);
    return matmul_real_by_complex(u, C, T1, rows3, M, L, s);
}

static inline int64_t even_up(int64_t x) { return (x + 1) & ~int64_t(1); }

static inline char* at(void* base, int64_t elems, size_t es) { return (char*)base + (size_t)elems * es; }

// The two fused passes of a small-basis transform (qs_common.h: FusedPass), T2 (L, L, M, M) between them.
// Slab pass, (d, c): item t = slab u[t] (L x L, contiguous), Out_t = C^T . u[t] . C = T2[t] (M x M); with `t2_transposed`
// T2 is stored (r, s, a, b) instead (nitems = L^2 then).
static FusedPass slab_pass(const void* u, void* T2, const void* C, int64_t nitems, int64_t L, int64_t M, bool t2_transposed) {
    FusedPass p{};
    p.in = (const double*)u; p.out = (double*)T2;
    p.R = (const double*)C; p.r_sk = M; p.r_sj = 1;          // R = C (L x M)
    p.Lm = (const double*)C; p.l_sp = 1; p.l_sa = M;         // Lm = C^T
    p.in_item = L * L; p.in_row = L; p.in_col = 1;
    if (t2_transposed) { p.out_item = 1; p.out_row = M * nitems; p.out_col = nitems; }
    else { p.out_item = M * M; p.out_row = M; p.out_col = 1; }
    p.L = (int)L; p.M = (int)M; p.nitems = (unsigned)nitems;     // (extents_ok: every count fits)
    return p;
}

// Column pass, (b, a): item t = column (r, s) of T2, Out_t = Ct . T2[:, :, t] . Ct^T = out[:, :, t]; with `t2_transposed`
// the items are T2's slabs.
static FusedPass column_pass(const void* T2, void* out, const void* Ct, int64_t L, int64_t M, bool t2_transposed) {
    const int64_t MM = M * M;
    FusedPass p{};
    p.in = (const double*)T2; p.out = (double*)out;
    p.R = (const double*)Ct; p.r_sk = 1; p.r_sj = L;         // R = Ct^T (Ct: M x L)
    p.Lm = (const double*)Ct; p.l_sp = L; p.l_sa = 1;        // Lm = Ct
    if (t2_transposed) { p.in_item = L * L; p.in_row = L; p.in_col = 1; }
    else { p.in_item = 1; p.in_row = L * MM; p.in_col = MM; }
    p.out_item = 1; p.out_row = M * MM; p.out_col = MM;
    p.L = (int)L; p.M = (int)M; p.nitems = (unsigned)MM;
    return p;
}

// contractions d, c, b on `rows` leading-index rows.  `CT` is scratch for C^T: the c contraction of
// the tiled path multiplies with it; the fused small-basis pass reads C itself and needs no transpose.
static int contract_dcb(int in_dtype, int dtype, const void* u, const void* C, void* CT, const void* Ct,
                        void* T1, void* T2, void* T3, int64_t rows, int64_t L, int64_t M,
                        hipStream_t s) {
    // small bases: d and c in one pass over the tensor (each slab u[a, b] is contiguous):
    //   T2[ab] = C^T . u[ab] . C   on the 4-wide matrix instruction, else on the 16-wide one
    int rc = 1;
    if (in_dtype == dtype && (g_tune.sandwich == 1 || g_tune.sandwich == 2 || g_tune.sandwich == 4 || g_tune.sandwich == 5))
        rc = sandwich4_try(dtype, slab_pass(u, T2, C, rows * L, L, M, false), 0, s);
    if (rc == 1 && in_dtype == dtype) rc = slab_pair_try(dtype, u, C, T2, rows * L, L, M, s);
    if (rc == 1) {
        rc = transpose_small(dtype, C, CT, L, M, s);
        if (rc) return rc;
        rc = gemm_d(in_dtype, dtype, u, C, T1, rows * L * L, L, M, s);
        if (rc) return rc;
        rc = gemm(packed(dtype, CT, T1, T2, M, M, L, rows * L), s);
    }
    if (rc) return rc;
    return gemm(packed(dtype, Ct, T2, T3, M, M * M, L, rows), s);
}

}  // namespace qs

using namespace qs;

extern "C" {

int qs_abi_version(void) { return QS_ABI_VERSION; }

const char* qs_error_string(int code) {
    switch (code) {
        case QS_OK: return "ok";
        case QS_ERR_BAD_EXTENT: return "bad extent (non-positive, inconsistent or too large)";
        case QS_ERR_NULL_POINTER: return "null pointer";
        case QS_ERR_MISALIGNED: return "pointer not aligned to its element size";
        case QS_ERR_WORKSPACE: return "workspace too small";
        case QS_ERR_HIP: return "HIP runtime error";
        case QS_ERR_BAD_DTYPE: return "unsupported dtype code";
        case QS_ERR_ALIAS: return "output aliases an input";
        case QS_ERR_COMM: return "RCCL error";
        default: return "unknown error code";
    }
}

const char* qs_last_hip_error(void) { return g_hip_err; }

const char* qs_last_dispatch(void) { return g_dispatch; }

int qs_tuning_reset(void) {
    g_tune = Tuning();
    return QS_OK;
}

int qs_tuning_set(const char* key, int64_t value) {
    if (!key) return QS_ERR_NULL_POINTER;
    if (!strcmp(key, "gemm_f64_cfg")) { g_tune.gemm_f64_cfg = (int)value; return QS_OK; }
    if (!strcmp(key, "gemm_c128_cfg")) { g_tune.gemm_c128_cfg = (int)value; return QS_OK; }
    if (!strcmp(key, "gemm_pipe")) { g_tune.gemm_pipe = (int)value; return QS_OK; }
    if (!strcmp(key, "gemm_fast")) { g_tune.gemm_fast = (int)value; return QS_OK; }
    if (!strcmp(key, "gemm_fit")) { g_tune.gemm_fit = (int)value; return QS_OK; }
    if (!strcmp(key, "gemm_skinny")) { g_tune.gemm_skinny = (int)value; return QS_OK; }
    if (!strcmp(key, "gemm_stream")) { g_tune.gemm_stream = (int)value; return QS_OK; }
    if (!strcmp(key, "slab_pair")) { g_tune.slab_pair = (int)value; return QS_OK; }
    if (!strcmp(key, "gemm_fast_persist")) { g_tune.gemm_fast_persist = (int)value; return QS_OK; }
    if (!strcmp(key, "sandwich_tail")) { g_tune.sandwich_tail = (int)value; return QS_OK; }
    if (!strcmp(key, "gemm_fast_shape")) { g_tune.gemm_fast_shape = (int)value; return QS_OK; }
    if (!strcmp(key, "gemm_pick")) { g_tune.gemm_pick = (int)value; return QS_OK; }
    if (!strcmp(key, "small4")) { g_tune.small4 = (int)value; return QS_OK; }
    if (!strcmp(key, "quad4s")) { g_tune.quad4s = (int)value; return QS_OK; }
    if (!strcmp(key, "pair4c")) { g_tune.pair4c = (int)value; return QS_OK; }
    if (!strcmp(key, "sandwich")) { g_tune.sandwich = (int)value; return QS_OK; }
    if (!strcmp(key, "gemm_strip")) { g_tune.gemm_strip = (int)value; return QS_OK; }
    if (!strcmp(key, "gemm_strip_w")) { g_tune.gemm_strip_w = (int)value; return QS_OK; }
    if (!strcmp(key, "gemm_strip_wide")) {
        if (value < 0 || value > 2) return QS_ERR_BAD_EXTENT;
        g_tune.gemm_strip_wide = (int)value;
        return QS_OK;
    }
    if (!strcmp(key, "gemm_strip_wgs")) {
        if (value < 0 || value > 4096) return QS_ERR_BAD_EXTENT;
        g_tune.gemm_strip_wgs = (int)value;
        return QS_OK;
    }
    if (!strcmp(key, "gemm_stream_wgs")) {
        if (value < 0 || value > 4096) return QS_ERR_BAD_EXTENT;
        g_tune.gemm_stream_wgs = (int)value;
        return QS_OK;
    }
    if (!strcmp(key, "gemm_fast_unaligned")) { g_tune.gemm_fast_unaligned = (int)value; return QS_OK; }
    if (!strcmp(key, "comm_drop_wait")) { g_tune.comm_drop_wait = (int)value; return QS_OK; }
    if (!strcmp(key, "sandwich_mode")) { g_tune.sandwich_mode = (int)value; return QS_OK; }
    if (!strcmp(key, "sandwich_t2")) { g_tune.sandwich_t2 = (int)value; return QS_OK; }
    if (!strcmp(key, "sandwich_v2")) { g_tune.sandwich_v2 = (int)value; return QS_OK; }
    if (!strcmp(key, "exchange")) {
        if (value < 0 || value > 2) return QS_ERR_BAD_EXTENT;
        g_tune.exchange = (int)value;
        return QS_OK;
    }
    if (!strcmp(key, "exchange_block") || !strcmp(key, "exchange_block_d")) {
        if (value < 0 || value > 4096) return QS_ERR_BAD_EXTENT;
        (key[14] ? g_tune.exchange_block_d : g_tune.exchange_block) = (int)value;
        return QS_OK;
    }
    if (!strcmp(key, "exchange_pairs")) {
        if (value < 0 || value > 1) return QS_ERR_BAD_EXTENT;
        g_tune.exchange_pairs = (int)value;
        return QS_OK;
    }
    if (!strcmp(key, "exchange_order")) {
        if (value < 0 || value > 2) return QS_ERR_BAD_EXTENT;
        g_tune.exchange_order = (int)value;
        return QS_OK;
    }
    if (!strcmp(key, "exchange_leading")) {
        if (value < 0 || value > 2) return QS_ERR_BAD_EXTENT;
        g_tune.exchange_leading = (int)value;
        return QS_OK;
    }
    if (!strcmp(key, "exchange_upper")) {
        if (value < 0 || value > 2) return QS_ERR_BAD_EXTENT;
        g_tune.exchange_upper = (int)value;
        return QS_OK;
    }
    if (!strcmp(key, "exchange_lower")) {
        if (value < 0 || value > 2) return QS_ERR_BAD_EXTENT;
        g_tune.exchange_lower = (int)value;
        return QS_OK;
    }
    if (!strcmp(key, "gemm_upper_s")) {
        if (value != 0 && value != 16 && value != 32) return QS_ERR_BAD_EXTENT;
        g_tune.gemm_upper_s = (int)value;
        return QS_OK;
    }
    if (!strcmp(key, "mean_field_batch_g")) {
        if (value != 0 && value != 1 && value != 2 && value != 4 && value != 8) return QS_ERR_BAD_EXTENT;
        g_tune.mean_field_batch_g = (int)value;
        return QS_OK;
    }
    if (!strcmp(key, "pair_contract_g")) {
        if (value != 0 && value != 1 && value != 2 && value != 4 && value != 8) return QS_ERR_BAD_EXTENT;
        g_tune.pair_contract_g = (int)value;
        return QS_OK;
    }
    if (!strcmp(key, "det_ci_g")) {
        if (value != 0 && value != 1 && value != 2 && value != 4 && value != 8) return QS_ERR_BAD_EXTENT;
        g_tune.det_ci_g = (int)value;
        return QS_OK;
    }
    if (!strcmp(key, "string_ci_bytes")) {
        if (value < 0) return QS_ERR_BAD_EXTENT;
        g_tune.string_ci_bytes = value;
        return QS_OK;
    }
    if (!strcmp(key, "triples_bytes")) {
        if (value < 0) return QS_ERR_BAD_EXTENT;
        g_tune.triples_bytes = value;
        return QS_OK;
    }
    if (!strcmp(key, "lead_rows_max")) {
        if (value < 0 || value > 32) return QS_ERR_BAD_EXTENT;
        g_tune.lead_rows_max = (int)value;
        return QS_OK;
    }
    return QS_ERR_BAD_EXTENT;
}

int qs_matmul(int dtype, const void* A, const void* B, void* out, int64_t m, int64_t n, int64_t k,
              int64_t lda, int64_t ldb, int64_t ldc, int64_t batch, int64_t stride_a,
              int64_t stride_b, int64_t stride_c, int accumulate, void* stream) {
    dispatch_reset();
    if (!dtype_ok(dtype)) return QS_ERR_BAD_DTYPE;
    if (!A || !B || !out) return QS_ERR_NULL_POINTER;
    const size_t es = elem_size(dtype);
    if (!aligned(A, es) || !aligned(B, es) || !aligned(out, es)) return QS_ERR_MISALIGNED;
    if (stride_a < 0 || stride_b < 0 || stride_c < 0) return QS_ERR_BAD_EXTENT;
    return gemm(Product{dtype, (const double*)A, (const double*)B, (double*)out, m, n, k, lda, ldb, ldc, batch,
                        stride_a, stride_b, stride_c, accumulate},
                (hipStream_t)stream);
}

static int matmul_pairs(int dtype, const void* A, const void* B, void* out, int64_t m, int64_t n, int64_t k,
                        int64_t lda, int64_t ldb, int64_t ldc, int64_t grid_n, int64_t stride_a,
                        int64_t stride_b, int64_t stride_c, int accumulate, void* stream, bool mirror, bool lower = false) {
    dispatch_reset();
    if (!dtype_ok(dtype)) return QS_ERR_BAD_DTYPE;
    if (!A || !B || !out) return QS_ERR_NULL_POINTER;
    const size_t es = elem_size(dtype);
    if (!aligned(A, es) || !aligned(B, es) || !aligned(out, es)) return QS_ERR_MISALIGNED;
    if (stride_a < 0 || stride_b < 0 || stride_c < 0) return QS_ERR_BAD_EXTENT;
    if (grid_n <= 0 || grid_n > kTriangleMax) return QS_ERR_BAD_EXTENT;
    Product p{dtype, (const double*)A, (const double*)B, (double*)out, m, n, k, lda, ldb, ldc,
              grid_n * (grid_n + 1) / 2, stride_a, stride_b, stride_c, accumulate, grid_n, mirror};
    p.lower_from_mirror = lower;
    return gemm(p, (hipStream_t)stream);
}

int qs_matmul_pairs(int dtype, const void* A, const void* B, void* out, int64_t m, int64_t n, int64_t k,
                    int64_t lda, int64_t ldb, int64_t ldc, int64_t grid_n, int64_t stride_a,
                    int64_t stride_b, int64_t stride_c, int accumulate, void* stream) {
    return matmul_pairs(dtype, A, B, out, m, n, k, lda, ldb, ldc, grid_n, stride_a, stride_b, stride_c, accumulate, stream, false);
}

int qs_matmul_pairs_mirrored(int dtype, const void* A, const void* B, void* out, int64_t m, int64_t n, int64_t k,
                             int64_t lda, int64_t ldb, int64_t ldc, int64_t grid_n, int64_t stride_a,
                             int64_t stride_b, int64_t stride_c, int accumulate, void* stream) {
    return matmul_pairs(dtype, A, B, out, m, n, k, lda, ldb, ldc, grid_n, stride_a, stride_b, stride_c, accumulate, stream, true);
}

int qs_matmul_pairs_lower(int dtype, const void* A, const void* B, void* out, int64_t m, int64_t n, int64_t k,
                          int64_t lda, int64_t ldb, int64_t ldc, int64_t grid_n, int64_t stride_a,
                          int64_t stride_b, int64_t stride_c, int accumulate, void* stream) {
    return matmul_pairs(dtype, A, B, out, m, n, k, lda, ldb, ldc, grid_n, stride_a, stride_b, stride_c, accumulate, stream, false, true);
}

int qs_matmul_upper(int dtype, const void* A, const void* B, void* out, int64_t m, int64_t side, int64_t stack, int64_t k,
                    int64_t lda, int64_t ldb, int64_t ldc, int64_t batch, int64_t stride_a, int64_t stride_b,
                    int64_t stride_c, int accumulate, void* stream) {
    dispatch_reset();
    if (!dtype_ok(dtype)) return QS_ERR_BAD_DTYPE;
    if (!A || !B || !out) return QS_ERR_NULL_POINTER;
    const size_t es = elem_size(dtype);
    if (!aligned(A, es) || !aligned(B, es) || !aligned(out, es)) return QS_ERR_MISALIGNED;
    if (stride_a < 0 || stride_b < 0 || stride_c < 0) return QS_ERR_BAD_EXTENT;
    if (side <= 0 || side > 65535 || stack <= 0 || stack > INT32_MAX / (side * side)) return QS_ERR_BAD_EXTENT;
    Product p{dtype, (const double*)A, (const double*)B, (double*)out, m, stack * side * side, k, lda, ldb, ldc, batch,
              stride_a, stride_b, stride_c, accumulate};
    p.upper = side;
    return gemm(p, (hipStream_t)stream);
}

int qs_triangle_pair(int64_t n, int64_t t, int64_t* i, int64_t* j) {
    if (!i || !j) return QS_ERR_NULL_POINTER;
    if (n <= 0 || n > kTriangleMax || t < 0 || t >= n * (n + 1) / 2) return QS_ERR_BAD_EXTENT;
    const int64_t f = triangle_flat((uint32_t)t, (uint32_t)n);
    *i = f / n;
    *j = f % n;
    return QS_OK;
}

int64_t qs_transform_two_body_workspace(int dtype, int64_t L, int64_t M) {
    if (!dtype_ok(dtype)) return QS_ERR_BAD_DTYPE;
    if (!extents_ok(L, M)) return QS_ERR_BAD_EXTENT;
    const int64_t wa = (L * L * L * M > L * M * M * M) ? L * L * L * M : L * M * M * M;
    const int64_t wb = (M < L) ? L * L * M * M : 0;   // otherwise T2 lives in `out`
    return (even_up(L * M) + wa + wb) * (int64_t)elem_size(dtype);
}

}  // extern "C"

namespace qs {
// qs_transform_two_body / qs_transform_two_body_mixed: `in_dtype` is the type of u, `dtype` that of C, Ct and out

// where the streamed fp64 kernel measured faster than the other small-basis paths (profiles/r03_quad4s.txt)
// (9 ... 16 orbitals: 1.06-1.14x over qs_small4.hip; 17 ... 32: 1.12-1.21x over it / the 16-wide kernels, l = 20 10.2 -> 9.1 us, 32 22.4 -> 19.8; from 33
// the hand-scheduled qs_sandwich4*.hip stay ahead, 0.72-0.86x)
// 65 ... 95 orbitals (two workgroups per item quad): 1.05-1.42x over the tiled kernels, every size (l = 66 444 -> 331 us, 78 740 -> 585,
// 91 1406 -> 1113); 96 itself level (0.98x): the tiled kernels keep it.
static bool quad4s_wins(int64_t L, int64_t M) {
    if (L >= 9 && M >= 9 && L <= 32 && M <= 32) return true;
    // (round 4: a basis of exactly 80 = 5 x 16 orbitals is the strip kernels' -- 597 against 678 us, found by tools/dispatch_guard.py)
    if (L == 80 && M == 80) return false;
    return L >= 65 && M >= 65 && L <= 96 && M <= 96 && !(L == 96 && M == 96);
}

// The fused small-basis routes of the transform, tried in this order: small4, quad4s, pair4c, pair4m, sandwich.  T2
// (L, L, M, M) goes to WA; CT and WB are scratch of the unfused first pass of the sandwich route.  QS_OK / error after
// launching, 1 = no fused route applies (the four tiled products follow).
static int transform_two_body_fused(int in_dtype, int dtype, const void* u, const void* C, const void* Ct, void* out,
                                    void* CT, void* WA, void* WB, int64_t L, int64_t M, hipStream_t s) {
    const FusedPass slab = slab_pass(u, WA, C, L * L, L, M, false), column = column_pass(WA, out, Ct, L, M, false);
    // one family's two passes, pass_try(pass, tensor_is_b): 1 = it refused either pass, and the next candidate runs (after
    // a first pass that ran, it writes T2 again from the start)
    auto both = [&](auto pass_try) { const int rc = pass_try(slab, 0); return rc == QS_OK ? pass_try(column, 1) : rc; };
    int rc = 1;

    // up to 32 orbitals, both dtypes: two launches of the LDS-staged kernel (what is left below ~33 orbitals is launches, not
    // work: the 16-wide kernels need three to five); T2 (L, L, M, M) in WA
    // (same-box sweep with the launches of a transform captured in one graph, profiles/r03_small4.txt: 1.8-2.9x up to 15
    // orbitals for both dtypes, 1.1-1.4x for complex128 up to 24.  Since the streamed kernels exist (below: the loads of the
    // next items under the products of these) it is the automatic choice only up to 8 orbitals (fp64) / 4 (complex128) -- what the kernel waits for there is the one round trip of its loads and the
    // drain of its stores, with one workgroup per CU and nothing to overlap them with.  g_tune.small4 == 2: wherever it exists)
    const int64_t n4 = cdiv(L, 4);
    if (in_dtype == dtype && g_tune.small4 && L <= 32 && M <= 32 && n4 == cdiv(M, 4) &&
        (g_tune.small4 == 2 || n4 <= (dtype == QS_C128 ? 1 : 2)))
        rc = both([&](const FusedPass& p, int b) { return small4_try(dtype, p, b, s); });

    // fp64, 5 ... 96 orbitals: the two passes on the streamed kernel (qs_quad4s.h) where it measured faster than what
    // follows (profiles/r03_quad4s.txt).  g_tune.quad4s == 2: wherever it exists.
    if (rc == 1 && in_dtype == dtype && dtype == QS_F64 && g_tune.quad4s && L >= 5 && M >= 5 && L <= 96 && M <= 96 && n4 == cdiv(M, 4) &&
        (g_tune.quad4s == 2 || (quad4s_wins(L, M) && g_tune.sandwich < 4)))       // (sandwich >= 4: tuning runs of those kernels)
        rc = both([&](const FusedPass& p, int) { return quad4s_try(dtype, p, s); });

    // complex128 up to 56 orbitals: the same two passes with two items per matrix instruction (qs_pair4c.hip).  Automatic
    // where it measured faster than qs_small4.hip / the four 16-wide passes (same-box sweeps, profiles/r03_pair4c.txt): from 5
    // orbitals, all of them in the STREAMED form (section 5: item pairs through a ring of row quads, fetched ahead): 1.07-1.56x
    // (l = 20 17.2 -> 12.0 us, l = 55 409 -> 351 us = 45.9 TFLOP/s); 57 ... 64 orbitals exist but spill and lose.
    // g_tune.pair4c == 2: wherever it exists.
    if (rc == 1 && in_dtype == dtype && dtype == QS_C128 && g_tune.pair4c && L <= 64 && M <= 64 && n4 == cdiv(M, 4) &&
        (g_tune.pair4c == 2 || (n4 >= 2 && n4 <= 14)))
        rc = both([&](const FusedPass& p, int b) { return pair4c_try(dtype, p, b, s); });

    // small bases: two passes over the tensor instead of four -- (d, c) per slab u[a, b], then (b, a) per
    // column (r, s): out[:, :, rs] = Ct . T2[:, :, rs] . Ct^T (the same k-ordered sums, element for element)
    // a REAL tensor against complex coefficients (qs_transform_two_body_mixed), 5 ... 56 orbitals: the streamed pair kernel with
    // real items for the first pass (its first product is one MFMA per fragment instead of two), the complex one for the second
    // (tools/mixed_small.py: the tiled route took 22.7 us at l = 20 where a complex tensor takes 13.3).
    if (rc == 1 && in_dtype == QS_F64 && dtype == QS_C128 && g_tune.pair4c && L >= 5 && M >= 5 && L <= 56 && M <= 56 &&
        n4 == cdiv(M, 4))
        rc = both([&](const FusedPass& p, int b) { return b ? pair4c_try(dtype, p, b, s) : pair4m_try(p, s); });
    if (rc != 1) return rc;

    if (in_dtype == dtype && (g_tune.sandwich == 1 || g_tune.sandwich == 3 || g_tune.sandwich == 4 || g_tune.sandwich == 6)) {
        // T2 (L, L, M, M) goes to WA; the eligibility of the second pass is known before the first runs
        const int64_t MM = M * M;
        // the policy (where two fused passes measured faster) ...
        const bool wanted = dtype == QS_F64 && L <= 64 && M <= 64 && n4 == cdiv(M, 4) && MM >= 1024 &&
                            (4 * n4) * L * MM * 2 * 8 < (int64_t(1) << 31) &&
                            (g_tune.sandwich >= 4 ? n4 >= 6 : n4 >= 9) &&
                            // (15: both passes on slabs through the balanced kernel's instantiation for 16, or not at all)
                            (n4 != 15 || (g_tune.sandwich_v2 != 0 && g_tune.sandwich_t2 != 0 && g_tune.sandwich != 3 &&
                                          g_tune.sandwich != 6));
        // ... and the kernel's own eligibility rule, asked of the kernel (dry run of the very calls made below), so the
        // two can never disagree after the first pass has run: T2 transposed only if both passes take that layout
        const FusedPass slab_tr = slab_pass(u, WA, C, L * L, L, M, true), column_tr = column_pass(WA, out, Ct, L, M, true);
        const bool second_nat = wanted && sandwich4_try(dtype, column, 1, s) == QS_OK;
        const bool second_tr = wanted && g_tune.sandwich != 3 && g_tune.sandwich != 6 &&
                               sandwich4_try(dtype, slab_tr, 1, s) == QS_OK && sandwich4_try(dtype, column_tr, 1, s) == QS_OK;
        const bool second_ok = second_nat || second_tr;
        if (second_ok) {
            int rc2 = 1;
            // T2 transposed, (r, s, a, b): the second pass then fetches slabs like the first (64-byte runs, the four
            // waves of a workgroup on the same lines) instead of columns (32-byte runs), and the first one stores the
            // way the second does.  Same-box sweep (profiles/r02_small_basis_sweep.txt): 4-10 % faster for
            // ceil(l/4) in {10, 13, 14, 16}, faster than the second pass alone for 11, slower for 9 and l = 48 (45 ... 47:
            // faster since round 3, gpurun_out r03y tail_ab*); 15 has
            // slab passes only (the balanced kernel's instantiation for 16).
            const bool want_t2 = second_tr && (!second_nat || (g_tune.sandwich_t2 >= 0 ? g_tune.sandwich_t2 != 0
                                                                                         : (n4 == 10 || n4 == 11 || n4 >= 13 ||
                                                                                            (n4 == 12 && L % 4 != 0) ||
                                                                                            (n4 == 9 && L == 36 && M == 36 && g_tune.sandwich_tail))));
            // (want_t2: the dry run of this very call passed, so it launches; otherwise second_nat holds)
            if (g_tune.sandwich != 3 && g_tune.sandwich != 6) rc2 = sandwich4_try(dtype, want_t2 ? slab_tr : slab, 0, s);
            if (rc2 == 1) {
                // first pass on the 16-wide kernels (T1 in the spare buffer WB, T2 into WA, natural layout)
                rc2 = slab_pair_try(dtype, u, C, WA, L * L, L, M, s);
                if (rc2 == 1) {
                    rc2 = transpose_small(dtype, C, CT, L, M, s);
                    if (rc2) return rc2;
                    rc2 = gemm(packed(dtype, u, C, WB, L * L * L, M, L), s);
                    if (rc2) return rc2;
                    rc2 = gemm(packed(dtype, CT, WB, WA, M, M, L, L * L), s);
                }
            }
            if (rc2) return rc2;
            rc2 = sandwich4_try(dtype, want_t2 ? column_tr : column, 0, s);
            if (rc2 != 1) return rc2;
            // not reached: the dry runs above ARE the kernel's eligibility rule for these very calls
            snprintf(g_hip_err, sizeof(g_hip_err), "qs_transform_two_body: second fused pass refused after its dry run");
            return QS_ERR_HIP;
        }
    }
    return 1;
}

// ---- the route for a tensor with particle-exchange symmetry, u[a,b,c,d] == u[b,a,d,c] bit for bit.
// Both leading indices meet the same Ct and both trailing ones the same C, so T2[a,b,r,s] == T2[b,a,s,r] and
// out[p,q,r,s] == out[q,p,s,r]: the d and c contractions run on the pairs b >= a only, the closing product on q >= the
// block of p, and a mirror (qs_permute.hip) writes the other half.  The a contraction comes BEFORE the b contraction here
// (the closing product then has M - p0 rows, mostly on the 128-row form):
//   d:  T1[a, b][c, s]         = u[a, b][c, d] C[d, s]               one product over the pairs b >= a (or, where that pads
//                                                                    more, per block [a0, a1) of rows a on b >= a0)
//   c:  T2[a, b][r, s]         = CT[r, c] T1[a, b][c, s]             one product over the pairs b >= a;  then the mirror, a > b
//   a:  X[p, (b r s)]          = Ct[p, a] T2[a, (b r s)]             one product
//   b:  out[p][q >= p0, (r s)] = Ct[q >= p0, b] X[p][b, (r s)]       per block [p0, p1) of rows p, batched over p; then the mirror
// T1 (L, L, L, M), T2 (L, L, M, M), X (M, L, M, M); T1 and X may share storage, so may T2 and out.
// The other order contracts the leading indices first (u arrives complete, so nothing between the products needs its
// other half: X2[p,q,c,d] == X2[q,p,d,c] for any Ct, and each pair-wise step needs its own pair alone):
//   a:  X1[p, (b c d)]         = Ct[p, a] u[a, (b c d)]              one product
//   b:  X2[p][q >= p0, (c d)]  = Ct[q >= p0, b] X1[p][b, (c d)]      per block [p0, p1) of rows p, batched over p
//   d:  Y[p, q][c, s]          = X2[p, q][c, d] C[d, s]              over the pairs q >= p of the M x M grid
//   c:  out[p, q][r, s]        = CT[r, c] Y[p, q][c, s]              over the same pairs; then ONE mirror, q < p -- stored
//                                                                    by the c launch itself where its kernel can (gemm_mirrors)
// X1 (M, L, L, L), X2 (M, M, L, L), Y (M, M, L, M): the same flops (1 + 0.625 + 0.502 + 0.502 of a product at L == M), at
// L == M the very launches of the first order, and one mirror (of out, over all pairs) instead of two.

// smallest basis (both sizes) that takes the route by itself: the smallest measured size where it is >= 5 % faster than the plain
// route (profiles/exchange_pairs_ab.txt, plain / route: fp64 160 1.036, 192 1.179; complex128 160 1.258)
static constexpr int64_t kExchangeMin = 192, kExchangeMinC128 = 160;

static bool exchange_wanted(int dtype, int64_t L, int64_t M) {
    if (!dtype_ok(dtype) || !extents_ok(L, M) || !g_tune.exchange || !exchange_grids_fit(L, M)) return false;
    if (g_tune.exchange == 2) return true;
    return (L < M ? L : M) >= (dtype == QS_C128 ? kExchangeMinC128 : kExchangeMin);
}

// g_tune.exchange_order: which of the two orders above a call takes (0 the first, 2 the second).
// 1, the automatic rule: the leading indices first only where M >= L (for M < L the half the symmetry saves falls on the
// larger products in the other order) and from the smallest size measured to gain (profiles/exchange_order_ab.txt),
// never below the route's own thresholds.
static constexpr int64_t kExchangeOrderMin = 192, kExchangeOrderMinC128 = 160;

// (-DQS_EXCHANGE_FUSED_MIRROR=0 builds the route with the separate mirror everywhere: the A/B baseline)
#ifndef QS_EXCHANGE_FUSED_MIRROR
#define QS_EXCHANGE_FUSED_MIRROR 1
#endif

static bool exchange_leading_first(int dtype, int64_t L, int64_t M) {
    if (g_tune.exchange_order != 1) return g_tune.exchange_order == 2;
    return M >= L && L >= (dtype == QS_C128 ? kExchangeOrderMinC128 : kExchangeOrderMin);
}

// g_tune.exchange_leading: how the second order contracts its leading indices.  Seen through its trailing indices u has the
// same symmetry, u[:, :, c, d] == u[:, :, d, c]^T, so for a fixed (c, d) the a and b contractions are a two-sided product of
// the L x L matrix over (a, b), needed on the pairs d >= c only -- the trailing pass itself, with Ct^T for C and Ct for CT, once
// the pair matrix is turned (qs_permute.hip):
//   in:    Xs[c, d][a, b]   = u[a, b, c, d]                         on the pairs d >= c
//   b, a:  Xt[c, d][p, q]   = Ct[p, a] (Xs[c, d][a, b] Ct^T[b, q])  over those pairs: 0.502 + 0.502 of a product, not 1 + 0.625
//   back:  X2[p, q][c, d]   = Xt[c, d][p, q] (d >= c), Xt[d, c][q, p] (d < c)     on the pairs q >= p
// Xs (L, L, L, L) and Xt (L, L, M, M) go where X goes, the one between them (L, L, L, M) where T2 goes: that needs M >= L.
// 2 = this wherever M >= L and the movers' grids fit (else the launches of 0), 0 = never, 1 = from the smallest size at which
// it measured faster (profiles/exchange_leading_pairs_ab.txt section 2), never below the route's own thresholds.
// (fp64: 192 level, 224 loses 0.7 ms of 62; 240, 256, 288 and 320 gain 5.6, 5.9, 10.6 and 8.9 ms = 3-6.5 %; complex128 gains 7.5-16 % from 160 to 256)
static constexpr int64_t kExchangeLeadingMin = 240, kExchangeLeadingMinC128 = 160;

static bool exchange_leading_upper(int dtype, int64_t L, int64_t M);

static bool exchange_leading_pairs(int dtype, int64_t L, int64_t M) {
    if (exchange_leading_upper(dtype, L, M)) return false;
    if (g_tune.exchange_leading == 0 || M < L || !exchange_pair_grids_fit(dtype, L, M)) return false;
    if (g_tune.exchange_leading == 2) return true;
    const bool c128 = dtype == QS_C128;
    return L >= (c128 ? kExchangeMinC128 : kExchangeMin) && L >= (c128 ? kExchangeLeadingMinC128 : kExchangeLeadingMin);
}

// g_tune.exchange_upper: the leading indices with the triangle on the COLUMNS of the products' tile lists instead of on their
// batch index (Product::upper): every operand stays in its natural layout, so there is no way in and no way back --
//   b':   Z[a][q][c,d]  = Ct[q,b] u[a][b][c,d]     m = M (q), k = L (b, ldb = L^2), columns (c, d), batch a
//   a':   X2[p][q][c,d] = Ct[p,a] Z[a][q][c,d]     m = M (p), k = L (a, ldb = M L^2), columns (q, c, d)
//         ... both on the column blocks that meet d >= c only, for ALL (a | q) and ALL (p, q)
//   fill: X2[p,q][c,d]  = X2[q,p][d,c]             p <= q, d < c (the lower triangles of the pairs d and c read)
// Z (L, M, L, L) goes where X1 goes, X2 where it goes now; also for M < L and in place.
// 2 = wherever gemm_upper() takes both products and the fill's grid fits, 0 = never, 1 = where it measured faster, and only
// while exchange_leading is at its own automatic value (an explicit 0 or 2 there keeps exactly those launches).
// (fp64, L == M, profiles/exchange_upper_ab.txt: 192 gains 3.3 ms of 26.7 against the closing blocks, 256 8.0 ms of 89.0 and
// 320 33.2 ms of 296.4 against the pairs between two transposes: every eligible size measured, from the route's own threshold)
static constexpr int64_t kExchangeUpperMin = 192;

// the two products of a (L -> M) transform as gemm() would get them
static Product exchange_upper_b(const void* Ct, const void* src, void* mid, int64_t L, int64_t M) {
    Product p{QS_F64, (const double*)Ct, (const double*)src, (double*)mid, M, L * L, L, L, L * L, L * L, L, 0, L * L * L, M * L * L, 0};
    p.upper = L;
    return p;
}

static Product exchange_upper_a(const void* Ct, const void* mid, void* dst, int64_t L, int64_t M) {
    Product p{QS_F64, (const double*)Ct, (const double*)mid, (double*)dst, M, M * L * L, L, L, M * L * L, M * L * L, 1, 0, 0, 0, 0};
    p.upper = L;
    return p;
}

static bool exchange_leading_upper(int dtype, int64_t L, int64_t M) {
    if (g_tune.exchange_upper == 0 || dtype != QS_F64 || !exchange_mirror_lower_fits(M, L)) return false;
    // (16-byte aligned stand-ins for the buffers: the conditions on the extents are what is asked here)
    const double* al = reinterpret_cast<const double*>(uintptr_t(256));
    if (!gemm_upper(exchange_upper_b(al, al, const_cast<double*>(al), L, M)) ||
        !gemm_upper(exchange_upper_a(al, al, const_cast<double*>(al), L, M)))
        return false;
    if (g_tune.exchange_upper == 2) return true;
    // (M < L, reached under a forced order only, was not measured)
    return g_tune.exchange_leading == 1 && M >= L && L >= kExchangeMin && L >= kExchangeUpperMin;
}

// g_tune.exchange_lower: the column-triangle pass WITHOUT its fill.  The fill's one consumer is the d launch over the pairs
// q >= p, which for row block G = block(c) walks the k-stages J = block(d): the block X2[p,q](G, J >= G) is there after a', and
// for J < G the wanted block is X2[q,p](J, G)^T, and X2[q,p](J, G) is there.  The d launch then carries
// Product::lower_from_mirror (qs_gemm_fast.hip: the mirror pair's block lands in LDS as it is and is read the other way
// round).  The lower blocks of X2 are never written -- in place they hold stale u -- and nothing reads them.
// 2 = wherever the pass runs, d is one launch over the pairs and gemm_lower() takes it (L a multiple of 64, M of 128; else the
// launches with the fill), 0 = never, 1 = where it measured faster, and only while exchange_upper is at its own automatic
// value (an explicit 2 there keeps exactly its launches, the fill included).
// (fp64, profiles/exchange_lower_ab.txt: L == M == 256, the one eligible size that fits one device with L == M)
static constexpr int64_t kExchangeLowerMin = 256;

static bool exchange_lower_wanted(int64_t L) {
    if (g_tune.exchange_lower == 0) return false;
    if (g_tune.exchange_lower == 2) return true;
    return g_tune.exchange_upper == 1 && L >= kExchangeLowerMin;
}

// the d launch over the pairs j >= i of a G x G grid of (L, L) matrices, as gemm() would get it
static Product exchange_d_pairs(int dtype, const void* src, const void* C, void* mid, int64_t G, int64_t L, int64_t M) {
    return Product{dtype, (const double*)src, (const double*)C, (double*)mid, L, M, L, L, M, M, G * (G + 1) / 2, L * L, 0, L * M, 0, G};
}

// T1, T2, X: the three buffers of the comment above.  The a, b, d, c order keeps X1 where X goes, X2 where T2 goes and Y
// where T1 goes; in either order every product reads one of the two storages and writes the other.
static int transform_two_body_exchange_route(int dtype, const void* u, const void* C, const void* Ct, void* CT, void* T1,
                                             void* T2, void* X, void* out, int64_t L, int64_t M, hipStream_t s) {
    const size_t es = elem_size(dtype);
    const int64_t MM = M * M;
    // blocks (same-call sweep at l = 192 ... 256, profiles/exchange_route_sweep.txt): 64 rows keep the closing product of fp64 on
    // its exact forms (32: level at 256, -1 % at 192; 128: -1.4 %); complex128 gains 1 % from 32; d is flat from 8 to 32
    const int64_t blk = g_tune.exchange_block > 0 ? g_tune.exchange_block : (dtype == QS_C128 ? 32 : 64);
    const int64_t blk_d = g_tune.exchange_block_d > 0 ? g_tune.exchange_block_d : (blk < 16 ? blk : 16);
    auto cat = [&](const void* base, int64_t elems) { return (const double*)((const char*)base + (size_t)elems * es); };
    auto mat = [&](void* base, int64_t elems) { return (double*)at(base, elems, es); };
    // (asked again with the buffers themselves: their alignment is one of the product's conditions)
    const bool leading_upper = exchange_leading_first(dtype, L, M) && exchange_leading_upper(dtype, L, M) &&
                               gemm_upper(exchange_upper_b(Ct, u, X, L, M)) && gemm_upper(exchange_upper_a(Ct, X, T2, L, M));
    const bool leading_pairs = exchange_leading_first(dtype, L, M) && exchange_leading_pairs(dtype, L, M);
    int rc = leading_pairs ? QS_OK : transpose_small(dtype, C, CT, L, M, s);      // (on pairs the slot holds Ct^T first)
    if (rc) return rc;
    // The trailing indices, on the pairs j >= i of a G x G grid of (L, L) matrices (G = L on u, G = M on X2):
    //   mid[i, j][c, s] = src[i, j][c, d] C[d, s],   dst[i, j][r, s] = CT[r, c] mid[i, j][c, s]
    // with the two small matrices the caller names: (C, C^T) for the trailing indices, (Ct^T, Ct) for the leading ones of a
    // turned tensor.
    // d and c are one product per pair on operands that are contiguous in the flat pair index i G + j: a
    // triangular batch (Product::pairs) runs each as ONE launch on exactly the G (G + 1) / 2 pairs.  For c that is the
    // per-row launches' tile list in one grid.  For d it pads the L rows of EVERY pair to whole tiles where the blocks'
    // flat (G - i0) L rows pad once, so the dispatch's own estimates of the two forms decide (at L a multiple of 128
    // neither pads: the single launch, 0.502 of a product where the blocks compute 0.53).
    // g_tune.exchange_pairs == 0: the launches per block and per row.  Same bits: for c the same kernel on the same tiles;
    // for d the tiles differ where L is no whole number of them (L rows per pair against (G - i0) L flat rows), possibly
    // the instantiation too, and the bits agree because every tiled form sums along k in the same order.
    // (A block of rows i computes the pairs j >= i0: for j < i that is work nobody reads -- on X2, whose closing blocks
    // need not line up with these, possibly from storage nothing has written; a row of a product depends on its own row of
    // the operand alone.)
    // `mirrored` (null: not wanted): dst is the result and its other half is wanted too -- where the dispatch can, the c
    // launch stores it from its own registers (Product::mirror) and *mirrored says so; otherwise the caller launches the
    // mirror.
    // `lower`: src holds the blocks (G, J >= G) of every entry only (g_tune.exchange_lower, above); the caller has asked
    // d_is_single() and gemm_lower() for this very launch.
    auto d_block = [&](const void* src, void* mid, int64_t G, const void* C, int64_t i0) {
        const int64_t rows = (i0 + blk_d < G ? i0 + blk_d : G) - i0, LL = L * L, LM = L * M;
        return Product{dtype, cat(src, (i0 * G + i0) * LL), (const double*)C, mat(mid, (i0 * G + i0) * LM),
                       (G - i0) * L, M, L, L, M, M, rows, G * LL, 0, G * LM, 0};
    };
    auto d_is_single = [&](const void* src, void* mid, int64_t G, const void* C) {
        if (g_tune.exchange_pairs == 0) return false;
        double blocks_cost = 0.0;
        for (int64_t i0 = 0; i0 < G; i0 += blk_d) blocks_cost += gemm_cost(d_block(src, mid, G, C, i0));
        return gemm_cost(exchange_d_pairs(dtype, src, C, mid, G, L, M)) <= blocks_cost;
    };
    auto trailing = [&](const void* src, void* mid, void* dst, int64_t G, const void* C, const void* CT, bool* mirrored,
                        bool lower = false) -> int {
        const int64_t npairs = G * (G + 1) / 2, LM = L * M;
        Product d_pairs =exchange_d_pairs(dtype, src, C, mid, G, L, M);
        d_pairs.lower_from_mirror = lower;
        if (lower || d_is_single(src, mid, G, C)) {
            if (int rc = gemm(d_pairs, s)) return rc;
        } else {
            for (int64_t i0 = 0; i0 < G; i0 += blk_d)
                if (int rc = gemm(d_block(src, mid, G, C, i0), s)) return rc;
        }
        if (g_tune.exchange_pairs) {
            Product c{dtype, (const double*)CT, (const double*)mid, (double*)dst, M, M, L, L, M, M, npairs, 0, LM, MM, 0, G};
            if (mirrored) c.mirror = *mirrored = QS_EXCHANGE_FUSED_MIRROR && gemm_mirrors(c);
            return gemm(c, s);
        }
        for (int64_t i = 0; i < G; ++i)
            if (int rc = gemm(packed(dtype, CT, cat(mid, (i * G + i) * LM), mat(dst, (i * G + i) * MM), M, M, L, G - i), s)) return rc;
        return QS_OK;
    };
    // The leading indices, on matrices of W elements (W = M M on T2, W = L L on u):
    //   mid[p, (b w)] = Ct[p, a] src[a, (b w)],   dst[p][q >= p0, w] = Ct[q >= p0, b] mid[p][b, w]  per block [p0, p1) of rows p
    auto leading = [&](const void* src, void* mid, void* dst, int64_t W) -> int {
        if (int rc = gemm(packed(dtype, Ct, src, mid, M, L * W, L), s)) return rc;
        for (int64_t p0 = 0; p0 < M; p0 += blk) {
            const int64_t rows = (p0 + blk < M ? p0 + blk : M) - p0;
            if (int rc = gemm(Product{dtype, cat(Ct, p0 * L), cat(mid, p0 * L * W), mat(dst, (p0 * M + p0) * W),
                                      M - p0, W, L, L, W, W, rows, 0, L * W, M * W, 0}, s))
                return rc;
        }
        return QS_OK;
    };
    // ... on the column blocks d >= c of W = L L (g_tune.exchange_upper, above): mid (L, M, L, L), dst (M, M, L, L) complete on
    // the pairs q >= p after the fill (`fill`; without it, on the blocks (G, J >= G) of every pair)
    auto leading_upper_pass = [&](const void* src, void* mid, void* dst, bool fill) -> int {
        if (int rc = gemm(exchange_upper_b(Ct, src, mid, L, M), s)) return rc;
        if (int rc = gemm(exchange_upper_a(Ct, mid, dst, L, M), s)) return rc;
        return fill ? exchange_mirror_lower(dtype, dst, M, L, s) : QS_OK;
    };
    if (exchange_leading_first(dtype, L, M)) {
        // (the d launch that follows, asked with the buffers themselves)
        const bool lower_d = leading_upper && exchange_lower_wanted(L) && d_is_single(T2, T1, M, C) &&
                             gemm_lower(exchange_d_pairs(dtype, T2, C, T1, M, L, M));
        if (leading_upper) {
            rc = leading_upper_pass(u, /*Z*/ X, /*X2*/ T2, !lower_d);
        } else if (leading_pairs) {
            rc = exchange_pair_transpose(dtype, u, /*Xs*/ X, L, s);
            if (rc) return rc;
            rc = transpose_small(dtype, Ct, CT, M, L, s);
            if (rc) return rc;
            rc = trailing(/*Xs*/ X, T2, /*Xt*/ X, L, /*Ct^T*/ CT, Ct, nullptr);
            if (rc) return rc;
            rc = exchange_pair_transpose_back(dtype, /*Xt*/ X, /*X2*/ T2, L, M, s);
            if (rc) return rc;
            rc = transpose_small(dtype, C, CT, L, M, s);
        } else {
            rc = leading(u, /*X1*/ X, /*X2*/ T2, L * L);
        }
        if (rc) return rc;
        bool mirrored = false;
        rc = trailing(/*X2*/ T2, /*Y*/ T1, out, M, C, CT, &mirrored, lower_d);
        if (rc || mirrored) return rc;
        return exchange_mirror(dtype, out, M, M, 1, s);
    }
    rc = trailing(u, T1, T2, L, C, CT, nullptr);
    if (rc) return rc;
    rc = exchange_mirror(dtype, T2, L, M, 1, s);
    if (rc) return rc;
    rc = leading(T2, X, out, MM);
    if (rc) return rc;
    return exchange_mirror(dtype, out, M, M, blk, s);
}

// Argument checks and buffers of qs_transform_two_body; `exchange`: the route above, for a tensor that has the symmetry.
static int transform_two_body_impl(int in_dtype, int dtype, const void* u, const void* C, const void* Ct, void* out,
                                   void* work, int64_t work_bytes, int64_t L, int64_t M, void* stream, bool exchange = false) {
    dispatch_reset();
    if (!dtype_ok(dtype) || !dtype_ok(in_dtype) || (in_dtype == QS_C128 && dtype == QS_F64)) return QS_ERR_BAD_DTYPE;
    if (!extents_ok(L, M)) return QS_ERR_BAD_EXTENT;
    if (!u || !C || !Ct || !out || !work) return QS_ERR_NULL_POINTER;
    const size_t es = elem_size(dtype);
    if (!aligned(u, elem_size(in_dtype)) || !aligned(C, es) || !aligned(Ct, es) || !aligned(out, es) ||
        !aligned(work, 16))
        return QS_ERR_MISALIGNED;
    if (out == u || out == work) return QS_ERR_ALIAS;
    if (work_bytes < qs_transform_two_body_workspace(dtype, L, M)) return QS_ERR_WORKSPACE;
    hipStream_t s = (hipStream_t)stream;

    void* CT = work;
    void* WA = at(work, even_up(L * M), es);
    const int64_t wa = (L * L * L * M > L * M * M * M) ? L * L * L * M : L * M * M * M;
    void* WB = (M < L) ? at(WA, wa, es) : out;

    if (exchange) {
        if (in_dtype != dtype) return QS_ERR_BAD_DTYPE;
        if (!exchange_grids_fit(L, M)) return QS_ERR_BAD_EXTENT;
        return transform_two_body_exchange_route(dtype, u, C, Ct, CT, /*T1*/ WA, /*T2*/ WB, /*X*/ WA, out, L, M, s);
    }
    int rc = transform_two_body_fused(in_dtype, dtype, u, C, Ct, out, CT, WA, WB, L, M, s);
    if (rc != 1) return rc;
    rc = contract_dcb(in_dtype, dtype, u, C, CT, Ct, /*T1*/ WA, /*T2*/ WB, /*T3*/ WA, L, L, M, s);
    if (rc) return rc;
    return gemm(packed(dtype, Ct, WA, out, M, M * M * M, L), s);
}
}  // namespace qs

extern "C" {

int qs_transform_two_body(int dtype, const void* u, const void* C, const void* Ct, void* out,
                          void* work, int64_t work_bytes, int64_t L, int64_t M, void* stream) {
    return transform_two_body_impl(dtype, dtype, u, C, Ct, out, work, work_bytes, L, M, stream);
}

/* real fp64 u against complex128 coefficients -> complex128 result, without a complex copy of u: the d contraction
 * reads the real tensor (8 bytes per element) and runs as a real product against C seen as an (L, 2M) real matrix; the
 * other three contractions are complex.  Workspace: qs_transform_two_body_workspace(QS_C128, L, M). */
int qs_transform_two_body_mixed(const void* u_f64, const void* C, const void* Ct, void* out, void* work,
                                int64_t work_bytes, int64_t L, int64_t M, void* stream) {
    return transform_two_body_impl(QS_F64, QS_C128, u_f64, C, Ct, out, work, work_bytes, L, M, stream);
}

int64_t qs_transform_two_body_inplace_workspace(int dtype, int64_t L, int64_t M) {
    if (!dtype_ok(dtype)) return QS_ERR_BAD_DTYPE;
    if (!extents_ok(L, M) || M > L) return QS_ERR_BAD_EXTENT;
    return (even_up(L * M) + L * L * L * M) * (int64_t)elem_size(dtype);
}

}  // extern "C"

static int transform_two_body_inplace_impl(int dtype, void* u, const void* C, const void* Ct, void* work,
                                           int64_t work_bytes, int64_t L, int64_t M, void* stream, bool exchange) {
    dispatch_reset();
    if (!dtype_ok(dtype)) return QS_ERR_BAD_DTYPE;
    if (!extents_ok(L, M) || M > L) return QS_ERR_BAD_EXTENT;
    if (!u || !C || !Ct || !work) return QS_ERR_NULL_POINTER;
    const size_t es = elem_size(dtype);
    if (!aligned(u, es) || !aligned(C, es) || !aligned(Ct, es) || !aligned(work, 16)) return QS_ERR_MISALIGNED;
    if (work == u) return QS_ERR_ALIAS;
    if (work_bytes < qs_transform_two_body_inplace_workspace(dtype, L, M)) return QS_ERR_WORKSPACE;
    hipStream_t s = (hipStream_t)stream;
    void* CT = work;
    void* B = at(work, even_up(L * M), es);
    // the four contractions ping-pong between the tensor's own storage (A) and ONE spare buffer (B): every
    // product reads one and writes the other, and each intermediate fits where it goes (M <= L):
    //   d: A (L^4) -> B (L^3 M)   c: B -> A (L^2 M^2)   b: A -> B (L M^3)   a: B -> A (M^4)
    // (the exchange route the same way: T1 and X in B, T2 and the result in A)
    if (exchange) {
        if (!exchange_grids_fit(L, M)) return QS_ERR_BAD_EXTENT;
        return transform_two_body_exchange_route(dtype, u, C, Ct, CT, /*T1*/ B, /*T2*/ u, /*X*/ B, /*out*/ u, L, M, s);
    }
    int rc = transpose_small(dtype, C, CT, L, M, s);
    if (rc) return rc;
    rc = gemm(packed(dtype, u, C, B, L * L * L, M, L), s);
    if (rc) return rc;
    rc = gemm(packed(dtype, CT, B, u, M, M, L, L * L), s);
    if (rc) return rc;
    rc = gemm(packed(dtype, Ct, u, B, M, M * M, L, L), s);
    if (rc) return rc;
    return gemm(packed(dtype, Ct, B, u, M, M * M * M, L), s);
}

extern "C" {

int qs_transform_two_body_inplace(int dtype, void* u, const void* C, const void* Ct, void* work,
                                  int64_t work_bytes, int64_t L, int64_t M, void* stream) {
    return transform_two_body_inplace_impl(dtype, u, C, Ct, work, work_bytes, L, M, stream, false);
}

int qs_transform_two_body_exchange_wanted(int dtype, int64_t L, int64_t M) { return exchange_wanted(dtype, L, M) ? 1 : 0; }

int qs_two_body_exchange_symmetric(int dtype, const void* u, int64_t L, void* scratch, void* stream) {
    dispatch_reset();
    if (!dtype_ok(dtype)) return QS_ERR_BAD_DTYPE;
    if (L <= 0 || L > 4096) return QS_ERR_BAD_EXTENT;
    if (!u || !scratch) return QS_ERR_NULL_POINTER;
    if (!aligned(u, elem_size(dtype)) || !aligned(scratch, 4)) return QS_ERR_MISALIGNED;
    hipStream_t s = (hipStream_t)stream;
    hipStreamCaptureStatus capture = hipStreamCaptureStatusNone;
    if (int rc = hip_status(hipStreamIsCapturing(s, &capture), "hipStreamIsCapturing")) return rc;
    if (capture != hipStreamCaptureStatusNone) return 0;      // the verdict cannot be read back inside a capture: "not known to be symmetric"
    int* flag = (int*)scratch;
    if (int rc = hip_status(hipMemsetAsync(flag, 0, sizeof(int), s), "hipMemsetAsync(flag)")) return rc;
    if (int rc = exchange_check(dtype, u, L, flag, s)) return rc;
    int differs = 1;
    if (int rc = hip_status(hipMemcpyAsync(&differs, flag, sizeof(int), hipMemcpyDeviceToHost, s), "hipMemcpyAsync(flag)")) return rc;
    if (int rc = hip_status(hipStreamSynchronize(s), "hipStreamSynchronize")) return rc;
    return differs ? 0 : 1;
}

int qs_transform_two_body_exchange(int dtype, const void* u, const void* C, const void* Ct, void* out,
                                   void* work, int64_t work_bytes, int64_t L, int64_t M, void* stream) {
    return transform_two_body_impl(dtype, dtype, u, C, Ct, out, work, work_bytes, L, M, stream, true);
}

int qs_transform_two_body_inplace_exchange(int dtype, void* u, const void* C, const void* Ct, void* work,
                                           int64_t work_bytes, int64_t L, int64_t M, void* stream) {
    return transform_two_body_inplace_impl(dtype, u, C, Ct, work, work_bytes, L, M, stream, true);
}

int qs_exchange_mirror(int dtype, void* t, int64_t n, int64_t m, int64_t block, void* stream) {
    dispatch_reset();
    if (!dtype_ok(dtype)) return QS_ERR_BAD_DTYPE;
    if (n <= 0 || m <= 0 || block <= 0 || n > 4096 || m > 4096) return QS_ERR_BAD_EXTENT;
    if (!t) return QS_ERR_NULL_POINTER;
    if (!aligned(t, elem_size(dtype))) return QS_ERR_MISALIGNED;
    return exchange_mirror(dtype, t, n, m, block < n ? block : n, (hipStream_t)stream);
}

int qs_transform_two_body_exchange_leading_pairs(int dtype, int64_t L, int64_t M) {
    return dtype_ok(dtype) && extents_ok(L, M) && exchange_leading_first(dtype, L, M) && exchange_leading_pairs(dtype, L, M) ? 1 : 0;
}

int qs_transform_two_body_exchange_leading_upper(int dtype, int64_t L, int64_t M) {
    return dtype_ok(dtype) && extents_ok(L, M) && exchange_leading_first(dtype, L, M) && exchange_leading_upper(dtype, L, M) ? 1 : 0;
}

int qs_transform_two_body_exchange_lower_d(int dtype, int64_t L, int64_t M) {
    if (!qs_transform_two_body_exchange_leading_upper(dtype, L, M) || !exchange_lower_wanted(L) || !g_tune.exchange_pairs) return 0;
    // (16-byte aligned stand-ins for the buffers: the conditions on the extents are what is asked here; the route itself
    // also asks the dispatch's estimates whether d is one launch, which it is wherever L is a whole number of row tiles)
    const double* al = reinterpret_cast<const double*>(uintptr_t(256));
    return gemm_lower(exchange_d_pairs(dtype, al, al, const_cast<double*>(al), M, L, M)) ? 1 : 0;
}

int qs_exchange_mirror_lower(int dtype, void* t, int64_t n, int64_t m, void* stream) {
    dispatch_reset();
    if (dtype != QS_F64) return QS_ERR_BAD_DTYPE;                             // (complex128: not built)
    if (!exchange_mirror_lower_fits(n, m)) return QS_ERR_BAD_EXTENT;          // (n, m in 1 ... 4096 and fewer than 2^31 workgroups)
    if (!t) return QS_ERR_NULL_POINTER;
    if (!aligned(t, elem_size(dtype))) return QS_ERR_MISALIGNED;
    return exchange_mirror_lower(dtype, t, n, m, (hipStream_t)stream);
}

int qs_exchange_pair_transpose(int dtype, const void* src, void* dst, int64_t L, void* stream) {
    dispatch_reset();
    if (!dtype_ok(dtype)) return QS_ERR_BAD_DTYPE;
    if (L <= 0 || L > 4096 || !exchange_pair_grids_fit(dtype, L, 1)) return QS_ERR_BAD_EXTENT;      // (a grid of 2^31 workgroups or more)
    if (!src || !dst) return QS_ERR_NULL_POINTER;
    const int64_t es = (int64_t)elem_size(dtype), bytes = L * L * L * L * es;
    if (!aligned(src, es) || !aligned(dst, es)) return QS_ERR_MISALIGNED;
    if (overlaps(src, bytes, dst, bytes)) return QS_ERR_ALIAS;
    return exchange_pair_transpose(dtype, src, dst, L, (hipStream_t)stream);
}

int qs_exchange_pair_transpose_back(int dtype, const void* src, void* dst, int64_t L, int64_t M, void* stream) {
    dispatch_reset();
    if (!dtype_ok(dtype)) return QS_ERR_BAD_DTYPE;
    if (L <= 0 || M <= 0 || L > 4096 || M > 4096 || !exchange_pair_grids_fit(dtype, L, M)) return QS_ERR_BAD_EXTENT;
    if (!src || !dst) return QS_ERR_NULL_POINTER;
    const int64_t es = (int64_t)elem_size(dtype), bytes = L * L * M * M * es;
    if (!aligned(src, es) || !aligned(dst, es)) return QS_ERR_MISALIGNED;
    if (overlaps(src, bytes, dst, bytes)) return QS_ERR_ALIAS;
    return exchange_pair_transpose_back(dtype, src, dst, L, M, (hipStream_t)stream);
}

int64_t qs_transform_two_body_partial_workspace(int dtype, int64_t L, int64_t M, int64_t rows) {
    if (!dtype_ok(dtype)) return QS_ERR_BAD_DTYPE;
    if (!extents_ok(L, M) || rows <= 0 || rows > L) return QS_ERR_BAD_EXTENT;
    return (even_up(L * M) + rows * L * L * M + rows * L * M * M) * (int64_t)elem_size(dtype);
}

int qs_transform_two_body_partial(int dtype, const void* u_slab, const void* C, const void* Ct,
                                  void* v_slab, void* work, int64_t work_bytes, int64_t L,
                                  int64_t M, int64_t rows, void* stream) {
    dispatch_reset();
    if (!dtype_ok(dtype)) return QS_ERR_BAD_DTYPE;
    if (!extents_ok(L, M) || rows <= 0 || rows > L) return QS_ERR_BAD_EXTENT;
    if (!u_slab || !C || !Ct || !v_slab || !work) return QS_ERR_NULL_POINTER;
    const size_t es = elem_size(dtype);
    if (!aligned(u_slab, es) || !aligned(C, es) || !aligned(Ct, es) || !aligned(v_slab, es) ||
        !aligned(work, 16))
        return QS_ERR_MISALIGNED;
    if (v_slab == u_slab || v_slab == work) return QS_ERR_ALIAS;
    if (work_bytes < qs_transform_two_body_partial_workspace(dtype, L, M, rows)) return QS_ERR_WORKSPACE;
    hipStream_t s = (hipStream_t)stream;
    void* CT = work;
    void* T1 = at(work, even_up(L * M), es);
    void* T2 = at(T1, rows * L * L * M, es);
    return contract_dcb(dtype, dtype, u_slab, C, CT, Ct, T1, T2, v_slab, rows, L, M, s);
}

int qs_transform_one_body(int dtype, const void* h, const void* C, const void* Ct, void* out,
                          void* work, int64_t work_bytes, int64_t nmat, int64_t L, int64_t M,
                          void* stream) {
    dispatch_reset();
    if (!dtype_ok(dtype)) return QS_ERR_BAD_DTYPE;
    if (L <= 0 || M <= 0 || nmat <= 0 || L > 65536 || M > 65536) return QS_ERR_BAD_EXTENT;
    if (!h || !C || !Ct || !out || !work) return QS_ERR_NULL_POINTER;
    const size_t es = elem_size(dtype);
    if (!aligned(h, es) || !aligned(C, es) || !aligned(Ct, es) || !aligned(out, es) || !aligned(work, 16))
        return QS_ERR_MISALIGNED;
    if (out == h || out == work) return QS_ERR_ALIAS;
    if (work_bytes < nmat * L * M * (int64_t)es) return QS_ERR_WORKSPACE;
    hipStream_t s = (hipStream_t)stream;
    // T[(i,a), q] = sum_b h[i][a, b] C[b, q]
    int rc = gemm(packed(dtype, h, C, work, nmat * L, M, L), s);
    if (rc) return rc;
    // out[i][p, q] = sum_a Ct[p, a] T[i][a, q]
    return gemm(packed(dtype, Ct, work, out, M, M, L, nmat), s);
}

int qs_antisymmetrize(int dtype, const void* u, void* out, int64_t npq, int64_t l, void* stream) {
    dispatch_reset();
    if (!dtype_ok(dtype)) return QS_ERR_BAD_DTYPE;
    if (npq <= 0 || l <= 0 || l > 65536) return QS_ERR_BAD_EXTENT;
    if (!u || !out) return QS_ERR_NULL_POINTER;
    const size_t es = elem_size(dtype);
    if (!aligned(u, es) || !aligned(out, es)) return QS_ERR_MISALIGNED;
    return antisymmetrize(dtype, u, out, npq, l, (hipStream_t)stream);
}

int qs_spin_expand_two_body(int in_dtype, int out_dtype, const void* u, void* out, int64_t l,
                            int64_t p_lo, int64_t p_hi, int antisymmetrize_flag, void* stream) {
    dispatch_reset();
    if (!dtype_ok(in_dtype) || !dtype_ok(out_dtype)) return QS_ERR_BAD_DTYPE;
    if (in_dtype == QS_C128 && out_dtype == QS_F64) return QS_ERR_BAD_DTYPE;
    if (l <= 0 || l > 32768 || p_lo < 0 || p_hi > l || p_lo >= p_hi) return QS_ERR_BAD_EXTENT;
    if (!u || !out) return QS_ERR_NULL_POINTER;
    if (!aligned(u, elem_size(in_dtype)) || !aligned(out, elem_size(out_dtype))) return QS_ERR_MISALIGNED;
    if (out == u) return QS_ERR_ALIAS;
    return spin_expand(in_dtype, out_dtype, u, out, l, l, p_lo, p_hi, antisymmetrize_flag ? 1 : 0,
                       (hipStream_t)stream);
}

int qs_spin_expand_two_body_block(int in_dtype, int out_dtype, const void* u, void* out, int64_t l,
                                  int64_t np, int64_t nq, int antisymmetrize_flag, void* stream) {
    dispatch_reset();
    if (!dtype_ok(in_dtype) || !dtype_ok(out_dtype)) return QS_ERR_BAD_DTYPE;
    if (in_dtype == QS_C128 && out_dtype == QS_F64) return QS_ERR_BAD_DTYPE;
    if (l <= 0 || l > 32768 || np <= 0 || np > l || nq <= 0 || nq > l) return QS_ERR_BAD_EXTENT;
    if (!u || !out) return QS_ERR_NULL_POINTER;
    if (!aligned(u, elem_size(in_dtype)) || !aligned(out, elem_size(out_dtype))) return QS_ERR_MISALIGNED;
    if (out == u) return QS_ERR_ALIAS;
    return spin_expand(in_dtype, out_dtype, u, out, l, nq, 0, np, antisymmetrize_flag ? 1 : 0,
                       (hipStream_t)stream);
}

int qs_add_spin_one_body(int in_dtype, int out_dtype, const void* h, void* out, int64_t nmat,
                         int64_t l, void* stream) {
    dispatch_reset();
    if (!dtype_ok(in_dtype) || !dtype_ok(out_dtype)) return QS_ERR_BAD_DTYPE;
    if (in_dtype == QS_C128 && out_dtype == QS_F64) return QS_ERR_BAD_DTYPE;
    if (l <= 0 || nmat <= 0 || l > (1 << 20)) return QS_ERR_BAD_EXTENT;
    if (!h || !out) return QS_ERR_NULL_POINTER;
    if (!aligned(h, elem_size(in_dtype)) || !aligned(out, elem_size(out_dtype))) return QS_ERR_MISALIGNED;
    if (out == h) return QS_ERR_ALIAS;
    return kron_eye2(in_dtype, out_dtype, h, out, nmat, l, (hipStream_t)stream);
}

int qs_spin_squared_two_body(const void* S, void* out, int64_t n, int64_t p_lo, int64_t p_hi,
                             int antisymmetrize_flag, void* stream) {
    dispatch_reset();
    if (n <= 0 || n > 65536 || p_lo < 0 || p_hi > n || p_lo >= p_hi) return QS_ERR_BAD_EXTENT;
    if (!S || !out) return QS_ERR_NULL_POINTER;
    if (!aligned(S, 16) || !aligned(out, 16)) return QS_ERR_MISALIGNED;
    return spin2_two_body(S, out, n, p_lo, p_hi, antisymmetrize_flag ? 1 : 0, (hipStream_t)stream);
}

}  // extern "C"
