// Fast path of the batched row-major product (see qs_gemm.hip for the general
// kernel and the contraction -> GEMM map).
//
// Why a second kernel: on gfx950 the fp64 MFMA shares the SIMD's vector issue
// with ordinary VALU work -- every VALU instruction in the K loop takes its
// issue cycles away from the matrix pipe (measured with tools/probe_mix.hip:
// 32 integer adds per 16 MFMAs cost 12 % of the MFMA rate, and two co-resident
// waves do not hide it).  The general kernel spends ~130 VALU instructions per
// K step on 64-bit address arithmetic and edge handling.  The K loop of this
// kernel contains no VALU work at all:
//   * global loads use the scalar-base form (SGPR buffer descriptor + one
//     loop-invariant 32-bit lane offset); the bases advance on the scalar ALU;
//   * LDS addresses are one VGPR + immediates (the loop is unrolled by two so
//     the stage buffer is a compile-time constant; the DMA form's A fragments
//     take one VGPR per k-step and 16-row block, set before the loop);
//   * no per-lane bounds checks.
// Two forms (template parameter EDGE):
//   * exact: every extent a whole multiple of the tile (l = 128, 256, 512, ...);
//   * edge: any extent.  Memory safety comes from the buffer descriptors
//     (num_records = bytes left in the operand, kept on the scalar ALU; the
//     hardware returns 0 for dwords past it), exactness from zeroing the
//     k >= K part of the LAST k-stage in registers before it is written to
//     LDS (selects, so stray non-finite values cannot leak), and the epilogue
//     of a border tile stores under a per-lane predicate.  Rows >= m and
//     columns >= n of a border tile multiply whatever the loads returned and
//     are never stored.
// VEC = 16-byte global accesses (even extents and strides, 16-byte aligned
// bases), otherwise 8-byte ones (odd l, e.g. the 55 orbitals of config 2).
//
// Persistent workgroups: 2 per CU, each walks its share of the tile list
// (virtual block ids bid, bid + P, bid + 2P, ... of the XCD-chunked order the
// general kernel uses, so concurrently running workgroups still share operand
// panels in their XCD's L2).  The global stage stream is flat across tiles:
// the loads for the first stages of tile n+1 are issued during the last stages
// of tile n and its first fragments are read before tile n's epilogue, so the
// MFMA stream only pauses for the issue of the epilogue stores.  (With one
// workgroup per tile the prologue + epilogue + launch gap cost 8 % at K = 256.)
//
// Schedule inside a stage (rotated): fragments are double-buffered in
// registers, k-step kk+1 is read while kk multiplies; the last k-step of a
// stage runs after the stage barrier while the next stage's first fragments and
// the global loads of the stage after are in flight.

#include <type_traits>

#include <cmath>

#include "qs_common.h"
#include "qs_fast_items.h"
#include "qs_triangle.h"

// Epilogue stores are non-temporal: the product's output is read again only by the NEXT contraction, after the
// whole tensor has passed through the caches (same-box A/B, three alternating runs each: l = 256 66.9-67.2 ->
// 67.1-67.2 TFLOP/s, l = 128 57.7-58.1 -> 58.2-58.7; -DQS_FAST_NT=0 builds the plain-store form).
#ifndef QS_FAST_NT
#define QS_FAST_NT 1
#endif
#if QS_FAST_NT
#define QS_FAST_STORE(dst, v) __builtin_nontemporal_store((v), (dst))
#else
#define QS_FAST_STORE(dst, v) (*(dst) = (v))
#endif

// Exact fp64 form (!CX && VEC && !EDGE): stages go HBM -> LDS directly (buffer_load_dwordx4 ... lds, no VGPR
// destination, no ds_write) instead of through two staging register sets.  -DQS_FAST_DMA=0 builds the register-staged
// form of round 4 (the A/B baseline).
#ifndef QS_FAST_DMA
#define QS_FAST_DMA 1
#endif

// Measurement only (wrong results): -DQS_FAST_ABLATE_EPI_COPIES=1 stores each accumulator block's own register quads as the
// 16-byte items of the DMA forms' epilogue (same stores, bytes and addresses, none of the 124 vector moves that put an item
// together from two accumulator blocks).  It bounds what any cheaper epilogue can gain: 0.03 ms of the exchange route's 74 ms
// in this kernel at l = 256 (profiles/gemm_fast_epilogue_ab.txt), so the epilogue stays as it is.
#ifndef QS_FAST_ABLATE_EPI_COPIES
#define QS_FAST_ABLATE_EPI_COPIES 0
#endif
// The overloads (triangular batch, mirror, column triangle, lower from mirror) form the LDS destinations of a stage's DMA from
// one opaque base per stage, so that none of them is a spilled scalar reloaded in every stage (qs_gemm_fast_body.h,
// fetch_dma).  Results are unchanged, so this is also the ablation that bounds its own gain; -DQS_FAST_STAGE_M0=0 builds the
// hoisted form for A/B.
#ifndef QS_FAST_STAGE_M0
#define QS_FAST_STAGE_M0 1
#endif

namespace qs {

struct FastArgs {
    const double* A;
    const double* B;
    double* C;
    int64_t lda, ldb, ldc;   // elements
    int64_t sa, sb, sc;      // elements
    uint64_t a_end, b_end;   // address one past the last byte of each operand (edge form)
    int64_t m;               // extents (edge form: epilogue predicate, k-tail)
    int n, k;
    int nk;                  // ceil(K / KT)
    int tiles_m, tiles_n;
    unsigned total;          // tiles_m * tiles_n * batch = size of the virtual grid
    int group_along_m;
    int accumulate;
};

// ... of a product over a triangular batch (Product::pairs): the batch is the upper triangle of an n x n grid, entry t at its
// flat index.  A type of its own: the kernel for it is an OVERLOAD of gemm_fast_kernel (same name and template arguments,
// as the profiler and the dispatch record show them), so the plain batch's kernels carry none of the remap's code or
// registers.  Behind a run-time `if (g.pairs)` in ONE kernel the remap cost the flagship form 4 VGPRs and 19 spilled
// SGPRs, and every product of the plain route 0.8-1.4 ms of 32 at l = 256 (profiles/exchange_pairs_ab.txt).
struct FastPairsArgs : FastArgs {
    unsigned pairs;          // n > 0
};

// ... whose epilogue also stores the tile of pair (i, j > i) transposed at pair (j, i) (Product::mirror): a third overload,
// for the same reason.  Only what fast_mirror_form() names is ever instantiated.
struct FastPairsMirrorArgs : FastPairsArgs {};

// ... of a product on the column triangle (Product::upper): the n columns are a stack of side x side matrices, tiles_n counts
// the tiles that exist (per_matrix of each), and a tile's 128 columns are 128 >> sshift rows of 1 << sshift columns.  A
// fourth overload, for the same reason; only the exact fp64 DMA forms are instantiated.
struct FastUpperArgs : FastArgs {
    unsigned side, per_matrix, sshift;
};

template <bool CX, int TM, int TN, bool VEC, bool EDGE>
__global__ __launch_bounds__(256, 2)
void gemm_fast_kernel(const FastArgs g) {
#define QS_FAST_PAIRS 0
#include "qs_gemm_fast_body.h"
#undef QS_FAST_PAIRS
}

template <bool CX, int TM, int TN, bool VEC, bool EDGE>
__global__ __launch_bounds__(256, 2)
void gemm_fast_kernel(const FastPairsArgs g) {
#define QS_FAST_PAIRS 1
#include "qs_gemm_fast_body.h"
#undef QS_FAST_PAIRS
}

template <bool CX, int TM, int TN, bool VEC, bool EDGE>
__global__ __launch_bounds__(256, 2)
void gemm_fast_kernel(const FastPairsMirrorArgs g) {
#define QS_FAST_PAIRS 2
#include "qs_gemm_fast_body.h"
#undef QS_FAST_PAIRS
}

// (`g` must stay this kernel's FIRST parameter: the body reads the fields that only a tile change needs from offset 0 of the
// kernarg segment as a FastUpperArgs -- tile_args() in qs_gemm_fast_body.h.)
static_assert(std::is_trivially_copyable<FastUpperArgs>::value && std::is_base_of<FastArgs, FastUpperArgs>::value,
              "the kernarg segment begins with the argument's own bytes");
template <bool CX, int TM, int TN, bool VEC, bool EDGE>
__global__ __launch_bounds__(256, 2)
void gemm_fast_kernel(const FastUpperArgs g) {
#define QS_FAST_PAIRS 3
#include "qs_gemm_fast_body.h"
#undef QS_FAST_PAIRS
}

// ... of a triangular batch whose A entries are square (m == k == lda) and stored on their 16 x 16 blocks (G, J >= G) only, for
// ALL entries of the grid (Product::lower_from_mirror).  For every entry (i, j >= i) the kernel reads these blocks and
// nothing else of A:
//   of entry (i, j): the blocks (G, J >= G);
//   of entry (j, i): the blocks (J, G) with J < G, each taken for block (G, J) of entry (i, j) transposed.
// A fifth overload, for the same reason; only the exact fp64 DMA forms are instantiated.
struct FastPairsLowerArgs : FastPairsArgs {};

template <bool CX, int TM, int TN, bool VEC, bool EDGE>
__global__ __launch_bounds__(256, 2)
void gemm_fast_kernel(const FastPairsLowerArgs g) {
#define QS_FAST_PAIRS 4
#include "qs_gemm_fast_body.h"
#undef QS_FAST_PAIRS
}

template <bool CX, int TM, int TN, bool VEC, bool EDGE>
static int launch_fast(const Product& p, hipStream_t stream) {
    constexpr int KT = CX ? 8 : 16;
    constexpr int NP = CX ? 2 : 1;
    constexpr int BM = 32 * TM, BN = 32 * TN;
    constexpr int64_t ESZ = CX ? 16 : 8;
    constexpr int IPR_B = BN / ((!CX && VEC) ? 2 : 1);
    // a wave-instruction of the B loads spans 64 / IPR_B rows through its 32-bit lane offset
    if (IPR_B < 64 && (64 / IPR_B) * p.ldb * ESZ + 4096 >= (int64_t(1) << 32)) return 1;
    FastArgs g;
    g.A = p.A; g.B = p.B; g.C = p.C;
    g.lda = p.lda; g.ldb = p.ldb; g.ldc = p.ldc;
    g.sa = p.sa; g.sb = p.sb; g.sc = p.sc;
    // the last entry of a triangular batch is the grid's last pair (n - 1, n - 1), flat index n^2 - 1
    const int64_t last = p.pairs ? p.pairs * p.pairs - 1 : p.batch - 1;
    g.a_end = reinterpret_cast<uint64_t>(p.A) + (uint64_t)((last * p.sa + (p.m - 1) * p.lda + p.k) * ESZ);
    g.b_end = reinterpret_cast<uint64_t>(p.B) + (uint64_t)((last * p.sb + (p.k - 1) * p.ldb + p.n) * ESZ);
    g.m = p.m; g.n = (int)p.n; g.k = (int)p.k;
    g.nk = (int)cdiv(p.k, KT);
    g.tiles_m = (int)cdiv(p.m, BM);
    g.tiles_n = p.upper ? (int)((p.n / (p.upper * p.upper)) * gemm_upper_tiles(p.upper)) : (int)cdiv(p.n, BN);
    g.group_along_m = p.group_along_m();
    g.accumulate = p.accumulate ? 1 : 0;
    const int64_t total = (int64_t)g.tiles_m * g.tiles_n * p.batch;
    if (total <= 0 || total >= (int64_t(1) << 31)) return QS_ERR_BAD_EXTENT;
    g.total = (unsigned)total;
    // two persistent workgroups per CU (the LDS and register budget admits exactly two)
    const int n_cu = device_cu_count();
    int64_t P = 2 * (int64_t)n_cu;
    P -= P % 8;
    // How many tiles a workgroup walks (cross-tile prefetch hides the next tile's first loads
    // behind the current tile's last stages and epilogue):
    //   short tile lists (<= 8 per resident workgroup): fully persistent grid, +7 % at l = 64;
    //   long lists: 4 tiles per workgroup -- the dispatcher keeps balancing the grid, which a
    //   static split of a long list loses more on than the prefetch wins (-4 % at l = 256 when
    //   fully persistent, +1.5 % with 4 tiles; profiles/r01_gemm_notes.txt).
    // g_tune.gemm_fast_persist: 0 one tile per workgroup, 1 this policy, 2 always fully
    // persistent, >= 3 that many tiles per workgroup.
    int64_t tiles_per_wg = 1;
    bool full = false;
    if (g_tune.gemm_fast_persist == 1) { full = total <= 8 * P; tiles_per_wg = 4; }
    else if (g_tune.gemm_fast_persist == 2) full = true;
    else if (g_tune.gemm_fast_persist >= 3) tiles_per_wg = g_tune.gemm_fast_persist;
    if (!full) {
        P = (total + tiles_per_wg - 1) / tiles_per_wg;
        P = (P + 7) & ~int64_t(7);
    }
    if (P > total) P = total;
#if defined(QS_FAST_CX_PAD)
    const size_t lds = sizeof(double) * 2 * NP * (BM * (KT + 2) + KT * (CX ? BN + 16 : BN));
#else
    constexpr bool DMA = QS_FAST_DMA && !CX && VEC && !EDGE;     // unpadded A rows (the kernel's kDma)
    const size_t lds = sizeof(double) * 2 * NP * (BM * (CX || DMA ? KT : KT + 2) + KT * (CX ? BN + 16 : BN));
#endif
    static PerDeviceLds lds_opt_in[5];   // per instantiation, batch kind and device
    constexpr bool kMirrors = !CX && TM == 4 && TN == 4 && VEC && !EDGE;      // (fast_mirror_form)
    constexpr bool kUpper = QS_FAST_DMA && !CX && VEC && !EDGE && (TM == 4 || TM == 2) && TN == 4;      // (gemm_fast_upper, gemm_fast_lower)
    if (p.lower_from_mirror) {
        if constexpr (kUpper) {
            FastPairsLowerArgs gl;
            static_cast<FastArgs&>(gl) = g;
            gl.pairs = (unsigned)p.pairs;
            void (*kern)(const FastPairsLowerArgs) = gemm_fast_kernel<CX, TM, TN, VEC, EDGE>;
            if (int rc = opt_in_dynamic_lds((const void*)kern, lds, lds_opt_in[4], "hipFuncSetAttribute(gemm_fast)")) return rc;
            hipLaunchKernelGGL(kern, dim3((unsigned)P), dim3(256), lds, stream, gl);
            note_dispatch("qs::gemm_fast_kernel<false, %d, 4, true, false>(qs::FastPairsLowerArgs)", TM);
            return launch_status("gemm_fast launch");
        } else {
            return QS_ERR_BAD_EXTENT;      // not reached: gemm() asks gemm_lower() first
        }
    }
    if (p.upper) {
        if constexpr (kUpper) {
            FastUpperArgs gu;
            static_cast<FastArgs&>(gu) = g;
            gu.side = (unsigned)p.upper;
            gu.per_matrix = (unsigned)gemm_upper_tiles(p.upper);
            gu.sshift = gemm_upper_segment() == 32 ? 5u : 4u;
            void (*kern)(const FastUpperArgs) = gemm_fast_kernel<CX, TM, TN, VEC, EDGE>;
            if (int rc = opt_in_dynamic_lds((const void*)kern, lds, lds_opt_in[3], "hipFuncSetAttribute(gemm_fast)")) return rc;
            hipLaunchKernelGGL(kern, dim3((unsigned)P), dim3(256), lds, stream, gu);
            note_dispatch("qs::gemm_fast_kernel<false, %d, 4, true, false>(qs::FastUpperArgs)", TM);
            return launch_status("gemm_fast launch");
        } else {
            return QS_ERR_BAD_EXTENT;      // not reached: gemm() asks gemm_upper() first
        }
    }
    if (p.mirror) {
        if constexpr (kMirrors) {
            FastPairsMirrorArgs gm;
            static_cast<FastArgs&>(gm) = g;
            gm.pairs = (unsigned)p.pairs;
            void (*kern)(const FastPairsMirrorArgs) = gemm_fast_kernel<CX, TM, TN, VEC, EDGE>;
            if (int rc = opt_in_dynamic_lds((const void*)kern, lds, lds_opt_in[2], "hipFuncSetAttribute(gemm_fast)")) return rc;
            hipLaunchKernelGGL(kern, dim3((unsigned)P), dim3(256), lds, stream, gm);
            // (same name and template arguments as the other two: the record says which overload ran)
            note_dispatch("qs::gemm_fast_kernel<false, 4, 4, true, false>(qs::FastPairsMirrorArgs)");
            return launch_status("gemm_fast launch");
        } else {
            return QS_ERR_BAD_EXTENT;      // not reached: gemm() asks gemm_fast_mirrors() first
        }
    }
    if (p.pairs) {
        FastPairsArgs gp;
        static_cast<FastArgs&>(gp) = g;
        gp.pairs = (unsigned)p.pairs;
        void (*kern)(const FastPairsArgs) = gemm_fast_kernel<CX, TM, TN, VEC, EDGE>;
        if (int rc = opt_in_dynamic_lds((const void*)kern, lds, lds_opt_in[1], "hipFuncSetAttribute(gemm_fast)")) return rc;
        hipLaunchKernelGGL(kern, dim3((unsigned)P), dim3(256), lds, stream, gp);
    } else {
        void (*kern)(const FastArgs) = gemm_fast_kernel<CX, TM, TN, VEC, EDGE>;
        if (int rc = opt_in_dynamic_lds((const void*)kern, lds, lds_opt_in[0], "hipFuncSetAttribute(gemm_fast)")) return rc;
        hipLaunchKernelGGL(kern, dim3((unsigned)P), dim3(256), lds, stream, g);
    }
    note_dispatch("qs::gemm_fast_kernel<%s, %d, %d, %s, %s>", CX ? "true" : "false", TM, TN, VEC ? "true" : "false",
                  EDGE ? "true" : "false");
    return launch_status("gemm_fast launch");
}

namespace {
struct FastShape { int id, tm, tn; double weight; };
// Edge-form shapes: BM = 32 tm rows (any tm: two waves of 16 tm rows each), BN = 32 tn columns with tn a power of two (the
// B stage is handed out row-wise to the 256 threads).  Round 3 added the tall-and-narrow shapes 5-9: in the c, b and a
// contractions the NEW basis size M is the m extent of the product, and 128-row tiles waste up to half of the matrix pipe
// on bases just above a multiple of 128 (l = 130: 256 rows for 130; with tm = 5: 160); the 2-D oscillator shells (66, 78,
// 91, 105, 120, 136, 153, 171, 190, 210 ...) are such sizes.  Weights: relative full-tile rates (shapes 1-4 measured in
// round 1, profiles/r01_gemm_notes.txt; 5-9 from the round-3 sweep, profiles/r03_mid_size_shapes.txt).
const FastShape kF64Shapes[] = {{1, 4, 4, 1.00}, {2, 2, 4, 0.93}, {3, 4, 2, 0.93}, {4, 2, 2, 0.85}, {5, 3, 4, 0.91},
                                {6, 5, 2, 0.92}, {7, 6, 2, 0.89}, {8, 7, 2, 0.92}, {9, 3, 2, 0.87}};
const FastShape kC128Shapes[] = {{1, 4, 2, 1.00}, {2, 2, 4, 1.00}, {3, 2, 2, 0.95}};

// Shape of the smallest estimated time -- rounds of the tile list over the resident workgroups (two per CU) times the
// work of a tile over its relative rate (the rule of the general kernel, qs_gemm.hip pick_shape) -- and that estimate.
template <size_t N>
int pick_fast_shape(const FastShape (&cand)[N], int64_t m, int64_t n, int64_t batch, double* cost_out) {
    const double slots = 2.0 * device_cu_count();
    int best = cand[0].id;
    double best_cost = 1e300;
    for (const FastShape& c : cand) {
        if (g_tune.gemm_fast_shape >= 1 && g_tune.gemm_fast_shape <= (int)N && c.id != g_tune.gemm_fast_shape) continue;
        const double tiles = (double)cdiv(m, 32 * c.tm) * (double)cdiv(n, 32 * c.tn) * (double)batch;
        const double rounds = tiles > 8 * slots ? tiles / slots : ceil(tiles / slots);
        const double cost = rounds * (32.0 * c.tm) * (32.0 * c.tn) / c.weight;
        if (cost < best_cost) { best_cost = cost; best = c.id; }
    }
    if (cost_out) *cost_out = best_cost;
    return best;
}
}  // namespace

double gemm_fast_estimate(const Product& p, bool even) {
    if (!g_tune.gemm_fast) return 1e300;
    const bool cx = p.dtype == QS_C128;
    const int64_t m = p.m, n = p.n, k = p.k, batch = p.batch;
    const double slots = 2.0 * device_cu_count();
    auto whole = [&](int bm, int bn, double w) {
        // (a column triangle: its real tile list)
        const double tiles_n = p.upper ? (double)((n / (p.upper * p.upper)) * gemm_upper_tiles(p.upper)) : (double)(n / bn);
        const double tiles = (double)(m / bm) * tiles_n * (double)batch;
        const double rounds = tiles > 8 * slots ? tiles / slots : ceil(tiles / slots);
        return rounds * bm * bn / w;
    };
    // (the exact form against the edge form of the same shape: no guards, no range arithmetic: l = 128 58.4 TFLOP/s against the
    // ~51 the edge form's l = 120 scales to)
    if (p.upper) return gemm_fast_upper(p) ? (m % 128 == 0 ? whole(128, 128, 1.12) : whole(64, 128, 1.04)) : 1e300;
    if (!cx && even && k % 16 == 0) {
        if (m % 128 == 0 && n % 128 == 0) return whole(128, 128, 1.12);
        if (m % 64 == 0 && n % 128 == 0) return whole(64, 128, 1.04);
    }
    if (cx) {      // (units of the complex tile shapes: the 64 x 128 tile = 1)
        if (k % 8 == 0 && ((m % 128 == 0 && n % 64 == 0) || (m % 64 == 0 && n % 128 == 0))) return whole(m % 128 == 0 ? 128 : 64, m % 128 == 0 ? 64 : 128, 1.10);
        if (k % 8 == 0 && m % 64 == 0 && n % 64 == 0) return whole(64, 64, 1.04);
        return 1e300;
    }
    double cost = 1e300;
    pick_fast_shape(kF64Shapes, m, n, batch, &cost);
    if (!even && !g_tune.gemm_fast_unaligned) cost /= 0.85;
    return cost;
}

// fp64 edge form, shape id of kF64Shapes
template <bool VEC>
static int launch_edge_f64(int shape, const Product& p, hipStream_t stream) {
    switch (shape) {
        case 1: return launch_fast<false, 4, 4, VEC, true>(p, stream);
        case 2: return launch_fast<false, 2, 4, VEC, true>(p, stream);
        case 3: return launch_fast<false, 4, 2, VEC, true>(p, stream);
        case 5: return launch_fast<false, 3, 4, VEC, true>(p, stream);
        case 6: return launch_fast<false, 5, 2, VEC, true>(p, stream);
        case 7: return launch_fast<false, 6, 2, VEC, true>(p, stream);
        case 8: return launch_fast<false, 7, 2, VEC, true>(p, stream);
        case 9: return launch_fast<false, 3, 2, VEC, true>(p, stream);
        default: return launch_fast<false, 2, 2, VEC, true>(p, stream);
    }
}

// Is this product one that gemm_fast_try() below puts on the exact fp64 128 x 128 form -- the one form that has a mirrored
// epilogue?  (m == n, so the 64 x 128 form, which needs n % 128 == 0 too, is never what a mirrored product gets; complex128:
// not built.)  The conditions are those of gemm_fast_try and launch_fast up to that form, in their order.
bool gemm_fast_mirrors(const Product& p) {
    if (!g_tune.gemm_fast || p.dtype != QS_F64 || !p.pairs || p.m != p.n || p.accumulate) return false;
    if (32 * p.lda * 8 + 256 >= (int64_t(1) << 32)) return false;
    if (p.m >= (int64_t(1) << 31) - 256 || p.k >= (int64_t(1) << 31) - 256) return false;
    const bool even = aligned(p.A, 16) && aligned(p.B, 16) && aligned(p.C, 16) && !(p.lda & 1) && !(p.ldb & 1) &&
                      !(p.ldc & 1) && !(p.sa & 1) && !(p.sb & 1) && !(p.sc & 1) && !(p.n & 1);
    return (even || g_tune.gemm_fast_unaligned != 0) && p.k % 16 == 0 && p.m % 128 == 0;
}

// Segment length of a column-triangle tile and the tiles of one s x s matrix (s a multiple of it): S x S super-blocks on
// and above the diagonal, S^2 / 128 tiles each.
// (shipped: S = 16, 272 of 512 tiles at s = 256 where S = 32 keeps 288)
int64_t gemm_upper_segment() { return g_tune.gemm_upper_s == 32 ? 32 : 16; }

int64_t gemm_upper_tiles(int64_t s) {
    const int64_t S = gemm_upper_segment(), ns = s / S;
    return ns * (ns + 1) / 2 * (S * S / 128);
}

// Does a product with Product::upper go on the exact fp64 DMA forms (the only ones that walk the column triangle)?  The
// conditions are those of gemm_fast_try and launch_fast up to those forms, and the form's own.
bool gemm_fast_upper(const Product& p) {
    const int64_t s = p.upper, S = gemm_upper_segment();
    if (!g_tune.gemm_fast || !QS_FAST_DMA || p.dtype != QS_F64 || s <= 0 || p.pairs || p.mirror || p.accumulate) return false;
    if (s % S || s > 65535 || p.n % (s * s)) return false;
    if (32 * p.lda * 8 + 256 >= (int64_t(1) << 32)) return false;
    if ((128 / S) * s * 8 + 256 >= (int64_t(1) << 32)) return false;      // the B lane offset spans the tile's R rows of (c, d)
    if (p.m >= (int64_t(1) << 31) - 256 || p.n >= (int64_t(1) << 31) - 256 || p.k >= (int64_t(1) << 31) - 256) return false;
    const bool even = aligned(p.A, 16) && aligned(p.B, 16) && aligned(p.C, 16) && !(p.lda & 1) && !(p.ldb & 1) &&
                      !(p.ldc & 1) && !(p.sa & 1) && !(p.sb & 1) && !(p.sc & 1);
    return (even || g_tune.gemm_fast_unaligned != 0) && p.k % 16 == 0 && p.m % 64 == 0;
}

int gemm_fast_upper_launch(const Product& p, hipStream_t stream) {
    if (!gemm_fast_upper(p)) return QS_ERR_BAD_EXTENT;
    return p.m % 128 == 0 ? launch_fast<false, 4, 4, true, false>(p, stream) : launch_fast<false, 2, 4, true, false>(p, stream);
}

// Does a product go on the lower-from-mirror forms (Product::lower_from_mirror, read with the flag set or not)?  A triangular
// fp64 batch of square A entries, side x side with lda == side and the entries at least side^2 apart, side a multiple of the
// 16-column block and of the row tile (128 rows, or 64 where side is no multiple of 128), no accumulate; and the conditions
// of gemm_fast_try and launch_fast up to the exact DMA forms.
bool gemm_fast_lower(const Product& p) {
    if (!g_tune.gemm_fast || !QS_FAST_DMA || p.dtype != QS_F64 || p.pairs <= 0 || p.mirror || p.upper || p.accumulate) return false;
    if (p.m != p.k || p.lda != p.k || p.sa < p.k * p.k) return false;
    if (32 * p.lda * 8 + 256 >= (int64_t(1) << 32)) return false;
    if (p.m >= (int64_t(1) << 31) - 256 || p.n >= (int64_t(1) << 31) - 256) return false;
    const bool even = aligned(p.A, 16) && aligned(p.B, 16) && aligned(p.C, 16) && !(p.lda & 1) && !(p.ldb & 1) &&
                      !(p.ldc & 1) && !(p.sa & 1) && !(p.sb & 1) && !(p.sc & 1);
    // (16-byte items at 16-byte addresses only: the turned blocks were not probed at odd strides)
    return even && p.k % 16 == 0 && p.m % 64 == 0 && p.n % 128 == 0;
}

int gemm_fast_lower_launch(const Product& p, hipStream_t stream) {
    if (!p.lower_from_mirror || !gemm_fast_lower(p)) return QS_ERR_BAD_EXTENT;
    return p.m % 128 == 0 ? launch_fast<false, 4, 4, true, false>(p, stream) : launch_fast<false, 2, 4, true, false>(p, stream);
}

// Returns QS_OK after launching, or 1 when the product does not qualify
// (caller falls back to the general kernel).
int gemm_fast_try(const Product& p, double general_cost, hipStream_t stream) {
    if (!g_tune.gemm_fast) return 1;
    const bool cx = p.dtype == QS_C128;
    const int64_t esz = cx ? 16 : 8;
    const int64_t m = p.m, n = p.n, k = p.k;
    if (cx && (!aligned(p.A, 16) || !aligned(p.B, 16) || !aligned(p.C, 16))) return 1;
    // the lane offsets of the loads are 32-bit: one item step of rows must fit
    if (32 * p.lda * esz + 256 >= (int64_t(1) << 32)) return 1;
    if (m >= (int64_t(1) << 31) - 256 || n >= (int64_t(1) << 31) - 256 || k >= (int64_t(1) << 31) - 256) return 1;
    // 16-byte accesses: aligned bases, even strides (complex elements are 16 bytes by themselves)
    // gfx950 carries out 16-byte buffer loads and global stores at ANY 8-byte-aligned address (tools/probe_unaligned.hip), so odd
    // strides and extents -- every odd basis size -- stage with 16-byte items too (g_tune.gemm_fast_unaligned = 0: 8-byte items
    // there, the rule of rounds 1-3); LDS accesses stay 16-byte aligned (the stage layout does not depend on the strides).
    const bool even = aligned(p.A, 16) && aligned(p.B, 16) && aligned(p.C, 16) && !(p.lda & 1) && !(p.ldb & 1) &&
                      !(p.ldc & 1) && !(p.sa & 1) && !(p.sb & 1) && !(p.sc & 1) && !(n & 1);
    const bool vec = cx || even || g_tune.gemm_fast_unaligned != 0;
    // ---- exact form: every extent a whole number of tiles
    if (!cx && vec && k % 16 == 0) {
        if (m % 128 == 0 && n % 128 == 0) return launch_fast<false, 4, 4, true, false>(p, stream);
        if (m % 64 == 0 && n % 128 == 0) return launch_fast<false, 2, 4, true, false>(p, stream);
    }
    if (cx && k % 8 == 0) {
        if (m >= n && m % 128 == 0 && n % 64 == 0) return launch_fast<true, 4, 2, true, false>(p, stream);
        if (m % 64 == 0 && n % 128 == 0) return launch_fast<true, 2, 4, true, false>(p, stream);
        if (m % 128 == 0 && n % 64 == 0) return launch_fast<true, 4, 2, true, false>(p, stream);
        if (m % 64 == 0 && n % 64 == 0) return launch_fast<true, 2, 2, true, false>(p, stream);
    }
    // ---- edge form.  Round 1 measured it against the general kernel with the four shapes of that time: +3...9 % for fp64
    // products whose m and n are both >= 100, slower below (short tile lists: the general kernel's small and 96-wide shapes
    // won) and for complex128 (whose general kernel is already light on VALU work per MFMA).  With the tall shapes the
    // rule is an estimate: the edge form runs when its best shape's estimated time beats the general kernel's best
    // (`general_cost`, same formula, scaled by the general kernel's full-tile rate relative to this one).
    // g_tune.gemm_fast: 1 = that policy, 3 = edge form wherever it applies (tests, tuning).
    if (g_tune.gemm_fast != 1 && g_tune.gemm_fast != 3) return 1;
    if (cx) {
        if (g_tune.gemm_fast == 1) return 1;
        switch (pick_fast_shape(kC128Shapes, m, n, p.batch, nullptr)) {
            case 1: return launch_fast<true, 4, 2, true, true>(p, stream);
            case 2: return launch_fast<true, 2, 4, true, true>(p, stream);
            default: return launch_fast<true, 2, 2, true, true>(p, stream);
        }
    }
    double cost = 0.0;
    const int shape = pick_fast_shape(kF64Shapes, m, n, p.batch, &cost);
    if (!vec) cost /= 0.85;                 // 8-byte staging (l = 255 against 256: 52.9 / 67.3 TFLOP/s with the K tail and the padding taken out)
    if (g_tune.gemm_fast == 1 && !(cost <= general_cost)) return 1;
    return vec ? launch_edge_f64<true>(shape, p, stream) : launch_edge_f64<false>(shape, p, stream);
}

}  // namespace qs
