// Shared host-side helpers for the gfx950 basis-transformation library.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <atomic>

#include "qs_amd.h"

namespace qs {

// Record the text of a failed HIP call for qs_last_hip_error().
void note_hip_error(hipError_t e, const char* what);

inline int hip_status(hipError_t e, const char* what) {
    if (e == hipSuccess) return QS_OK;
    note_hip_error(e, what);
    return QS_ERR_HIP;
}

// Launch check: kernels are asynchronous, so this only catches launch-time
// failures (bad configuration, missing code object); it never synchronises.
inline int launch_status(const char* what) {
    return hip_status(hipGetLastError(), what);
}

inline bool aligned(const void* p, size_t a) {
    return (reinterpret_cast<uintptr_t>(p) & (a - 1)) == 0;
}

// Do the byte ranges [a, a + na) and [b, b + nb) share a byte?  (The alias test of every entry.)
inline bool overlaps(const void* a, int64_t na, const void* b, int64_t nb) {
    const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b;
    return x < y + (uintptr_t)nb && y < x + (uintptr_t)na;
}

inline size_t elem_size(int dtype) { return dtype == QS_C128 ? 16 : 8; }

inline bool dtype_ok(int dtype) { return dtype == QS_F64 || dtype == QS_C128; }

// Library state is keyed by DEVICE, never by process: one process may drive several GPUs
// (hipFuncSetAttribute, occupancy and the CU count are per-device facts).
constexpr int kMaxDevices = 64;

// Ordinal of the calling thread's current device (0 when the query fails).
int current_device();

// Compute units of the current device (cached per device: the property query costs far more
// than a kernel launch).
int device_cu_count();

// Largest dynamic-LDS size one kernel instantiation has been opted in to, per device (0 = never).
struct PerDeviceLds {
    std::atomic<uint32_t> bytes[kMaxDevices];
    PerDeviceLds() { for (auto& x : bytes) x.store(0); }
};

// Opt a kernel in to more than 64 KB of dynamic LDS on the current device.  The attribute is raised again whenever a
// launch asks for more than any earlier one did (kernels whose LDS size depends on run-time extents: spin2_tb,
// gemm_skinny), and never lowered.
int opt_in_dynamic_lds(const void* kern, size_t lds_bytes, PerDeviceLds& once, const char* what);

// Workgroups of `kern` (256 threads, no dynamic LDS) resident per CU on the current device,
// asked once per device and clamped to [1, 4]; `fallback` when the query fails.
struct PerDeviceInt {
    std::atomic<int> v[kMaxDevices];
    PerDeviceInt() { for (auto& x : v) x.store(0); }
};
int resident_workgroups(const void* kern, PerDeviceInt& cache, int fallback);

// Which kernels the calling thread's most recent entry point launched (qs_last_dispatch()):
// every launcher appends the name rocprofv3 shows for its instantiation.
void dispatch_reset();
void note_dispatch(const char* fmt, ...) __attribute__((format(printf, 1, 2)));

// Extents of a transform (L orbitals to M) for which every product keeps its n and grid inside 32 bits.
inline bool extents_ok(int64_t L, int64_t M) {
    return L > 0 && M > 0 && L <= 4096 && M <= 1024;      // M^3 < 2^31 needs M <= 1290
}

// ceil division for positive operands
inline int64_t cdiv(int64_t a, int64_t b) { return (a + b - 1) / b; }

// One batched product (qs_gemm.hip): C[t] (m x n) = A[t] (m x k) . B[t] (k x n) for t < batch, row-major, leading dimensions
// and batch strides in elements of `dtype` (a complex128 element is two interleaved doubles); accumulate: C += A.B.
struct Product {
    int dtype;
    const double* A;
    const double* B;
    double* C;
    int64_t m, n, k, lda, ldb, ldc, batch, sa, sb, sc;
    int accumulate;
    // Triangular batch: pairs = n > 0 makes entry t < batch = n (n + 1) / 2 the t-th pair (i, j >= i) of an n x n grid in
    // row-major order, with its operands at the pair's FLAT index f = i n + j (qs_triangle.h): A + f sa, B + f sb,
    // C + f sc.  0 = a plain batch, entry t at t.
    int64_t pairs = 0;
    // ... whose entry (i, j > i) is ALSO stored transposed at entry (j, i): element (r, c) at C + (j n + i) sc + c ldc + r.  Needs
    // pairs, m == n and no accumulate; entries (i, i) are stored once.  Only where gemm_mirrors() says yes.
    bool mirror = false;
    // Column triangle: upper = s > 0 makes the n columns a stack of n / s^2 row-major s x s matrices (c, d), of which only the
    // column blocks that meet d >= c are computed: a tile's 128 columns are R rows c of S contiguous columns d (R S = 128),
    // and a tile exists iff its last column >= its first row.  Elements with d < c inside such a block are computed and
    // stored; nothing else of B is read and nothing else of C is written.  A plain batch only (no pairs, mirror or
    // accumulate), s a multiple of S, and only where gemm_upper() says yes.
    int64_t upper = 0;
    // Lower blocks from the mirror pair: the A entries of a triangular batch are square (m == k == lda) and hold their
    // 16 x 16 blocks (G, J >= G) only, at ALL flat indices of the grid, with A(i, j) == A(j, i)^T.  The kernel takes block
    // (G, J < G) of entry (i, j) from block (J, G) of entry (j, i) and reads nothing else below the block diagonal.  Needs pairs,
    // fp64, no mirror, upper or accumulate, and only where gemm_lower() says yes.
    bool lower_from_mirror = false;
    // which operand is the stream that neighbouring tiles should share in L2: a shared (stride-0) A, or a short-and-wide
    // product, streams B (the tiled kernels walk the tiles of one B panel first)
    int group_along_m() const { return ((sa == 0 && batch > 1) || m < n) ? 1 : 0; }
};

// The one layout of the library's contractions: C[t] = A . B[t], A shared, B and C packed.
inline Product packed(int dtype, const void* A, const void* B, void* C, int64_t m, int64_t n, int64_t k, int64_t batch = 1) {
    return Product{dtype, (const double*)A, (const double*)B, (double*)C, m, n, k, k, n, n, batch, 0, k * n, m * n, 0};
}

// Validates the extents and strides, then launches the product on the first route that takes it (qs_gemm.hip).
int gemm(const Product& p, hipStream_t stream);

// Can gemm() honour Product::mirror for this product (read with the flag set or not) under the calling thread's tuning
// keys?  Only the exact fp64 128 x 128 form of qs_gemm_fast.hip has the mirrored epilogue; gemm() refuses a mirrored product
// that fails this with QS_ERR_BAD_EXTENT and launches nothing.
bool gemm_mirrors(const Product& p);

// Does gemm() take this product with its Product::upper under the calling thread's tuning keys?  Only the exact fp64 DMA
// forms of qs_gemm_fast.hip walk the column triangle (fp64, 16-byte items, k % 16 == 0, m % 64 == 0, s a multiple of the
// segment length, 32-bit lane offsets); gemm() refuses one that fails this with QS_ERR_BAD_EXTENT and launches nothing.
bool gemm_upper(const Product& p);

// Does gemm() take this product with Product::lower_from_mirror (read with the flag set or not) under the calling thread's
// tuning keys?  Only the exact fp64 DMA forms of qs_gemm_fast.hip fetch the mirror pair's blocks (a triangular fp64 batch,
// m == k == lda a multiple of 64, n of 128, entries at least m^2 apart, 16-byte items, no accumulate); gemm() refuses one that
// fails this with QS_ERR_BAD_EXTENT and launches nothing.
bool gemm_lower(const Product& p);
// Columns d of one segment of such a tile (16 or 32: g_tune.gemm_upper_s, 0 = the shipped choice) and the tiles of one s x s matrix
int64_t gemm_upper_segment();
int64_t gemm_upper_tiles(int64_t s);

// The dispatch's own estimate of a product's time on its tiled kernels (the smaller of the general kernel's best shape
// and qs_gemm_fast.hip's best form, in the latter's units: rounds of the tile list x tile area / relative rate).  For a
// caller that may cut the same work into launches in two ways; launches nothing.
double gemm_cost(const Product& p);

// A real (m x k, fp64) times B complex (k x n) -> out complex (m x n), packed row-major.  Interleaved complex storage makes
// this EXACTLY the real product A . [B as k x 2n] -> [out as m x 2n]: the real kernels run it with 2 MFMAs per fragment
// pair and 8 bytes read per element of A -- no complex copy of A (the d contraction of a real u against complex
// coefficients, basis_set.py:341-342 with NumPy's promotion).
int matmul_real_by_complex(const void* A, const void* B, void* out, int64_t m, int64_t n, int64_t k, hipStream_t stream);

// The d contraction T1[(abc), s] = u[(abc), d] C[d, s]: `in_dtype` is the tensor's type, `dtype` that of C and T1; the plain
// product, or the mixed one above for a real tensor against complex coefficients (qs_api.hip).
int gemm_d(int in_dtype, int dtype, const void* u, const void* C, void* T1, int64_t rows3, int64_t L, int64_t M, hipStream_t s);

// The product families that gemm() tries before its general tiled kernel: QS_OK / error after launching, 1 = not eligible.
// They take the product as gemm() validated it.
// VALU-free fast path, exact and edge forms (qs_gemm_fast.hip).  general_cost: the general kernel's estimated time for
// this product (its best shape, in this kernel's units): the edge form runs when its own estimate is not worse.
int gemm_fast_try(const Product& p, double general_cost, hipStream_t stream);
// ... and whether that would be the form with the mirrored epilogue (Product::mirror)
bool gemm_fast_mirrors(const Product& p);
// ... the column-triangle form (Product::upper): whether the exact DMA forms take it, and its launch
bool gemm_fast_upper(const Product& p);
int gemm_fast_upper_launch(const Product& p, hipStream_t stream);
// ... the lower-from-mirror form (Product::lower_from_mirror): the same two
bool gemm_fast_lower(const Product& p);
int gemm_fast_lower_launch(const Product& p, hipStream_t stream);

// Small-coefficient streaming product, m, k <= 64 (qs_gemm_stream.hip).
int gemm_stream_try(const Product& p, hipStream_t stream);

// Strip kernels (qs_gemm_strip.hip); other_cost: the other tiled kernels' best estimate, as general_cost above.
int gemm_strip_try(const Product& p, double other_cost, hipStream_t stream);

// Short-and-wide streaming product (qs_gemm_skinny.hip).
int gemm_skinny_try(const Product& p, hipStream_t stream);

// Fused pair of contractions on contiguous L x L slabs, L, M <= 64 (qs_slab_pair.hip): Z[s] = B^T.X[s].B.
int slab_pair_try(int dtype, const void* X, const void* B, void* Z, int64_t nslabs, int64_t L, int64_t M,
                  hipStream_t stream);

// One fused pass of the small-basis kernels: Out_t = Lm . In_t . R for t < nitems, a batch of L x L matrices In_t with
// arbitrary element strides, ceil(L/4) == ceil(M/4).  The common head of every family's kernel arguments
// (S4Args, Small4Args, Quad4Args, Pair4Args derive from it and add their own fields): kernel symbols name those structs,
// and their layout is the kernels' argument layout -- `ntuples` stays in here, so that the base has no tail padding.
struct FusedPass {
    const double* in;
    double* out;
    const double* R;      // R[k][j]  = R[k * r_sk + j * r_sj],   L x M
    const double* Lm;     // Lm[p][a] = Lm[p * l_sp + a * l_sa],  M x L
    int64_t r_sk, r_sj, l_sp, l_sa;
    int64_t in_item, in_row, in_col;       // element strides of In_t[i][k]: in_col == 1 (a slab) or in_item == 1 (a column)
    int64_t out_item, out_row, out_col;    // element strides of Out_t[p][j]
    int L, M;
    unsigned nitems;
    unsigned ntuples;     // the item tuples one matrix instruction takes: quads, pairs in the pair kernels (set by the family)
};
static_assert(sizeof(FusedPass) == 128, "a family's own fields start at offset 128");

// A family's kernel arguments: `pass` and its item tuples of `per` items; the family's own fields zero.
template <class Args>
inline Args fused_args(const FusedPass& pass, int per) {
    Args g{};
    static_cast<FusedPass&>(g) = pass;
    g.ntuples = (unsigned)cdiv(pass.nitems, per);
    return g;
}

// The fused passes (qs_sandwich4.hip, qs_small4.hip, qs_quad4s.hip, qs_pair4c.hip): QS_OK / error after launching,
// 1 = not eligible.
// 4-wide matrix instruction, fp64, L, M <= 64.  dry_run: launch nothing, QS_OK = the call would launch.
int sandwich4_try(int dtype, const FusedPass& pass, int dry_run, hipStream_t stream);

// SMALL bases, L, M <= 32, fp64 and complex128: item quads staged in LDS.  tensor_is_b: complex only -- in the 16-wide
// kernels' call for the first product the tensor is the B operand (the b contraction), which fixes the order of the two
// imaginary-part products.
int small4_try(int dtype, const FusedPass& pass, int tensor_is_b, hipStream_t stream);

// fp64, 5 ... 96 orbitals, streamed: item quads through a ring of row quads, one wave per column group.
int quad4s_try(int dtype, const FusedPass& pass, hipStream_t stream);
// The same for complex128, 5 ... 64 orbitals (qs_pair4s.h): two items per matrix instruction, blocks = (item, re | im), streamed.
int pair4c_try(int dtype, const FusedPass& pass, int tensor_is_b, hipStream_t stream);
// ... and for REAL items against complex R and Lm (the first pass of a real tensor against complex coefficients), streamed form only
int pair4m_try(const FusedPass& pass, hipStream_t stream);

// out (cols, rows) = in (rows, cols)^T, element = 8 or 16 bytes (tiny helper
// for the coefficient matrices).
int transpose_small(int dtype, const void* in, void* out, int64_t rows,
                    int64_t cols, hipStream_t stream);

// Bandwidth kernels (qs_permute.hip).
int antisymmetrize(int dtype, const void* u, void* out, int64_t npq, int64_t l, hipStream_t stream);
int spin_expand(int in_dtype, int out_dtype, const void* u, void* out, int64_t l, int64_t nq, int64_t p_lo,
                int64_t p_hi, int as, hipStream_t stream);
int kron_eye2(int in_dtype, int out_dtype, const void* h, void* out, int64_t nmat, int64_t l,
              hipStream_t stream);
int spin2_two_body(const void* S, void* out, int64_t n, int64_t p_lo, int64_t p_hi, int as,
                   hipStream_t stream);
// Particle-exchange symmetry t[a,b,r,s] == t[b,a,s,r].  Check: *flag (zeroed by the caller) becomes nonzero iff u (l, l, l, l)
// lacks it bit for bit.  Mirror, in place on t (n, n, m, m): t[a,b,r,s] = t[b,a,s,r] where a / block > b / block.
int exchange_check(int dtype, const void* u, int64_t l, int* flag, hipStream_t stream);
int exchange_mirror(int dtype, void* t, int64_t n, int64_t m, int64_t block, hipStream_t stream);
// Do the grids of the check and of both mirrors of an (L -> M) transform fit their 31 bits?
bool exchange_grids_fit(int64_t L, int64_t M);
// The route's leading indices on pairs: dst[c,d][a,b] = src[a,b,c,d] on the pairs d >= c (both (l, l, l, l)), and the way back
// with the other half filled in, src (l, l, m, m) stored on d >= c -> dst (m, m, l, l) on the pairs q >= p:
// dst[p,q][c,d] = src[c,d][p,q] where d >= c, src[d,c][q,p] where d < c.  Nothing else is written; src and dst are distinct.
int exchange_pair_transpose(int dtype, const void* src, void* dst, int64_t l, hipStream_t stream);
int exchange_pair_transpose_back(int dtype, const void* src, void* dst, int64_t l, int64_t m, hipStream_t stream);
// ... and whether their grids fit (fewer than 2^31 workgroups, at most 65535 along y and z)
bool exchange_pair_grids_fit(int dtype, int64_t L, int64_t M);
// In place on t (n, n, m, m): t[i,j][r,s] = t[j,i][s,r] for every pair i <= j and every s < r; nothing else is written
// (fp64 only).  The fill after the route's column-triangle products.
int exchange_mirror_lower(int dtype, void* t, int64_t n, int64_t m, hipStream_t stream);
bool exchange_mirror_lower_fits(int64_t n, int64_t m);

// Tuning knobs (qs_tuning_set / qs_tuning_reset): state of the CALLING THREAD only, so a tuning
// run or a test cannot change the dispatch of another thread's calls; every thread starts from the
// automatic policy.
struct Tuning {
    int gemm_f64_cfg = 0;        // tile shape of the general kernel, 0 = automatic
    int gemm_c128_cfg = 0;
    int gemm_pipe = 1;           // 1: rotated K-loop schedule, 0: plain schedule (A/B reference)
    int gemm_fast = 1;           // 0 general kernel only, 1 automatic, 2 exact form only, 3 edge form wherever legal
    int gemm_fast_persist = 1;   // 0 one workgroup per tile, 1 automatic, 2 always persistent, >= 3 tiles per workgroup
    int gemm_pick = 1;           // tile shape of the general kernel: 1 by rounds over the resident workgroups x tile work, 0 by padded area
    int sandwich_tail = 1;       // balanced small-basis kernel: the quads of a partly filled last round split over all workgroups
    int gemm_fast_shape = 0;     // forces edge-form shape 1..N (0 = by padded-work cost)
    int gemm_fit = 1;            // fitted tile shapes of the general kernel (the basis size covered by one tile, to the next multiple of
                                 // 16): 1 by estimated time, 2 wherever they exist, 0 off
    int gemm_skinny = 1;         // 0 disables the short-and-wide streaming product
    int gemm_stream = 1;         // 0 disables the small-coefficient streaming product, 2 = never split rows over two waves
    int gemm_stream_wgs = 0;     // most workgroups of a stream launch, 1 ... 4096 (0 = as many as stay resident): a short block list walks on few
                                 // waves, across batch slices -- tests reach the walk at the smallest eligible shape (tests/test_gpu_stream_forms.py)
    int slab_pair = 1;           // 0 disables the fused (d, c) pass, 2 = one wave per slab always
    int sandwich_t2 = -1;        // the intermediate of the two fused passes stored transposed, (r, s, a, b): -1 automatic, 0 never, 1 always
    int sandwich_v2 = -1;        // the balanced small-basis kernel with a cooperative fetch (qs_sandwich4b.hip): -1 automatic, 0 never, 1 wherever it exists,
                                 // 2 also every odd ceil(l/4) on the instantiation for the next even one
    int sandwich_mode = -1;      // work split of the fused passes: -1 automatic, 0 one item quad per workgroup, 1 four adjacent quads, 3 + step barrier
    int small4 = 1;              // both fused passes of a basis of <= 32 orbitals on the LDS-staged 4-wide kernel (qs_small4.hip), fp64 and
                                 // complex128: 1 automatic (fp64 up to 16, complex128 up to 24 orbitals), 2 wherever it exists (up to 32), 0 off
    int quad4s = 1;              // fp64 17 ... 64 orbitals on the streamed fused kernel (qs_quad4s.hip): 0 never, 1 where measured faster, 2 wherever it exists
    int pair4c = 1;              // complex128 up to 56 orbitals: both fused passes on the two-items-per-instruction kernel (qs_pair4c.hip):
                                 // 1 automatic, 2 wherever it exists, 0 off
    int gemm_strip = 1;          // strip kernels (qs_gemm_strip.hip: the small extent of a product, <= 256, covered by ONE tile to the next
                                 // multiple of 16, eight waves): 0 never, 1 by estimated time, 2 wherever they exist
    int gemm_strip_w = 0;        // (tuning runs: relative rate of the strip kernels in percent, 0 = the built-in weights)
    int gemm_strip_wide = 0;     // the strip kernels' 256-wide form (fp64, up to 10 blocks): 0 automatic (where the tile list fills the chip a few
                                 // times over), 1 never, 2 wherever it exists -- tests reach it at kilobyte sizes (tests/test_gpu_strip_forms.py)
    int gemm_strip_wgs = 0;      // most workgroups of a strip launch, 1 ... 4096 (0 = one per CU): a short tile list walks on few workgroups
    int gemm_fast_unaligned = 1; // 16-byte items of the VALU-free kernel's edge form also at odd strides / extents (0: 8-byte items there)
    int comm_drop_wait = 0;      // TEST HOOK (qs_comm.hip): bit mask of stream waits of the sharded entry points to leave out -- the negative
                                 // test of the asynchronous stand-in transport; never set outside tests/
    int lead_rows_max = 8;       // qs_transform_two_body_blocks: most leading rows M0 that take qs_lead_contract.hip's streaming kernel for
                                 // step a (0 = never, at most 32 = the kernel's own limit); above it step a is one tiled product.
                                 // 8 = the 8-row instantiation, the largest measured one that beats the product (profiles/r08_blocks.txt)
    int mean_field_batch_g = 0;  // qs_mean_field_batch: densities per load of u, 0 = the shipped group size of the form; 1, 2, 4, 8 = tuning runs
                                 // (the chunk length follows the group size: results of different settings agree to rounding, not bit for bit)
    int pair_contract_g = 0;     // qs_pair_contract, qs_pair_contract_antisym, qs_pair_contract_exchange: vectors per load of U, 0 = the shipped group size of the form; 1, 2, 4, 8 = tuning runs
                                 // (every setting gives the same bits: the fma chains and the closing butterfly do not know G)
    int det_ci_g = 0;            // qs_det_ci_sigma: vectors per walk of a determinant's excitations, 0 = the shipped group size of the form;
                                 // 1, 2, 4, 8 = tuning runs (every setting gives the same bits: a vector's fma chain does not know G)
    int64_t string_ci_bytes = 0; // qs_string_ci_group: byte budget of the D and G panels of one qs_string_ci_sigma call, 0 = the caller's shipped value
    int64_t triples_bytes = 0;   // qs_triples_energy_budget: byte budget of the blocks of one pass of RCCD.triples, 0 = the caller's shipped value
    int exchange = 1;            // the transform's route for a tensor with particle-exchange symmetry (qs_transform_two_body_exchange_wanted):
                                 // 0 never, 1 where it measured faster, 2 wherever it exists (any size, ahead of the fused small-basis routes)
    int exchange_block = 0;      // rows per block of that route's closing product (and of its mirror), 0 = automatic
    int exchange_block_d = 0;    // rows per block of that route's d contraction, 0 = automatic (never above exchange_block when that is set)
    int exchange_pairs = 1;      // that route's c contraction (and d, where it pads no more) as ONE product over the pairs b >= a (Product::pairs):
                                 // 0 = one launch per row a / per block of exchange_block_d rows (the A/B baseline.  Same bits: c runs the same
                                 // kernel on the same tiles; d may tile differently, and every tiled form sums along k in the same order)
    int exchange_order = 1;      // that route's order of the contractions: 0 = the trailing indices first (d, c on the pairs of u, mirror, a, closing
                                 // blocks, mirror), 2 = the leading ones first (a, closing blocks, d, c on the pairs of the result's grid, ONE
                                 // mirror), 1 = the second where M >= L from the smallest size measured to gain, else the first
    int gemm_upper_s = 0;        // segment length S of a column-triangle tile (Product::upper): 16 or 32, 0 = the shipped choice
    int exchange_upper = 1;      // the leading indices of that route's second order as two products on the column blocks d >= c of u's
                                 // trailing indices and one fill of the other triangles (no pair movers): 0 = never, 2 = wherever
                                 // gemm_upper() takes both products, 1 = where it measured faster (and only while exchange_leading is 1)
    int exchange_lower = 1;      // that column-triangle pass without its fill: the d launch takes the blocks below the block diagonal from
                                 // the mirror pair (Product::lower_from_mirror): 0 = never, 2 = wherever gemm_lower() takes that launch,
                                 // 1 = where it measured faster (and only while exchange_upper is 1)
    int exchange_leading = 1;    // the leading indices of that route's second order (exchange_order): 0 = one product and the closing blocks,
                                 // 2 = on the pairs d >= c of u's trailing indices, between two transposes of the pair matrix (M >= L only:
                                 // below that, and where a mover's grid does not fit, the launches of 0), 1 = the second from the smallest
                                 // size measured to gain
    int sandwich = 1;            // 4-wide fused passes of a small-basis transform: 0 off, 1 both (d, c) and (b, a), 2 (d, c) only, 3 (b, a) only;
                                 // tuning runs, wherever the kernel exists (not only where it measured faster): 4 both, 5 (d, c) only, 6 (b, a) only
};
extern thread_local Tuning g_tune;

}  // namespace qs
