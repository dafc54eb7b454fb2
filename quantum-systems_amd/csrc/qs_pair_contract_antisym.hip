// Pair contraction of an anti-symmetrised tensor with amplitudes anti-symmetric in their pair, from the quarter of the
// tensor that the two symmetries do not repeat:
//   S[k,p,q] = 2 * sum_{r<s} U[p,q,r,s] T[k,r,s]   for p < q,      S[k,q,p] = -S[k,p,q],   S[k,p,p] = +0
// (no conjugation).  U is (l, l, l, l) with consecutive (p, q) rows ldu >= l^2 elements apart, T and S are (K, l, l).
// Only the elements of U with p < q and r < s and the elements r < s of T are ever addressed: the particle-particle
// ladder of coupled-cluster doubles on the untransformed tensor, and the sigma vector of two particles in spin orbitals.
//
// The r < s part of a (p, q) row is l - 1 runs of l - 1 - r elements that start at r l + r + 1: at any 8-byte alignment,
// so the unit of a load is ONE element (8 bytes fp64, 16 bytes complex128).  The kernel walks the PACKED triangle
// t = 0 ... n - 1, n = l (l - 1) / 2, t <-> (r, s) in row-major order of the runs, so that every lane of every load
// carries a term of the sum.  A workgroup of 256 threads takes 16 consecutive pair rows (p < q, row-major), wave w the
// kPaRows rows from row 4 w of them; the 64 lanes of a wave cover 64 consecutive packed positions of ONE row per load and
// walk along t in steps of 64, the next step's elements issued before the current step's fmas.  A lane carries its
// (r, s) along: a step adds 64 to s and wraps into the following runs, so only the first position of a lane needs the
// inverse of the triangle map (a square root and a correction).  The T values of a chunk of kPaSteps steps are staged in LDS
// already packed in the order of the walk, as [position][g] (records padded to an odd number of 16-byte units), two
// buffers, chunk c + 1 staged while chunk c is consumed: the staging threads are the only other users of the map.
// A lane past the end of the triangle, and a wave row past the last pair, re-reads an element of the quarter (position
// 0 / the last pair row) and drops it by a select.
// After the last step a wave closes its kPaRows * G row sums with one xor butterfly over masks 32 ... 1 in which every
// stage also halves the values a lane carries (the reduce-scatter of qs_pair_contract.hip); the lane left with the sum
// of (row, g) doubles it -- exact -- and stores it at (p, q), its negation at (q, p) and the zeros of the diagonal that
// its row owns: plain vector stores, no atomics, no workspace, no closing launch.
//
// Reproducible: every product is an explicit fma in a fixed order, a row's positions are dealt to the lanes by l alone
// and every sum goes through the same butterfly stages whatever G.  So S[k] has the same bits alone, anywhere in a batch
// and under any group size; a non-finite value stays in its row of U or its T[k].

#include "qs_contract_common.h"

namespace qs {

constexpr int kPaRows = 4;             // pair rows per wave; a workgroup takes 4 * kPaRows of them
constexpr int kPaSteps = 3;            // steps of 64 positions per staged chunk of T
constexpr int64_t kPaMaxL = 4096;      // l^2 <= 2^24 elements: every byte offset inside a row stays below 2^32
// Shipped group size per form {fp64, complex128}: the largest that keeps two workgroups per CU in VGPRs and in LDS
constexpr int kPaGroup[2] = {8, 8};

struct PaArgs {
    const double* U;
    const double* T;          // first amplitude of the group, [ng][l][l]
    double* S;                // first result of the group, [ng][l][l]
    int64_t ldu;
    int l, ng;                // ng: amplitudes of this launch, 1 ... G of the instantiation
};

// First packed position of run r: the elements (r, r + 1 ... l - 1) follow those of the runs before it
__host__ __device__ inline int pa_run_start(int r, int l) { return (int)(((int64_t)r * (2 * l - r - 1)) / 2); }

// (r, s) of packed position t < l (l - 1) / 2: the root of the quadratic, then a correction of its rounding
__host__ __device__ inline void pa_unpack(int t, int l, int& r, int& s) {
    const double b = 2.0 * l - 1.0;
    int rr = (int)((b - sqrt(b * b - 8.0 * t)) * 0.5);
    if (rr < 0) rr = 0;
    if (rr > l - 2) rr = l - 2;
    while (rr > 0 && pa_run_start(rr, l) > t) --rr;
    while (rr < l - 2 && pa_run_start(rr + 1, l) <= t) ++rr;
    r = rr;
    s = rr + 1 + (t - pa_run_start(rr, l));
}

// doubles of one position's record in LDS: G * AW, padded to an odd number of 16-byte units
static constexpr int pa_record_words(int form, int G) { return (((G * form_widths(form).aw) / 2) | 1) * 2; }

static constexpr size_t pa_lds_bytes(int form, int G) {
    return (size_t)2 * kPaSteps * 64 * pa_record_words(form, G) * 8;
}

// Sum of v[j] over the 64 lanes for every j, N a power of two <= 64 (as pc_close of qs_pair_contract.hip): butterfly
// stages 32 ... 1; while a lane carries more than one value a stage hands half of them to the partner lane.  Returns the
// index j of the finished sum left in v[0].
template <int CNT, int M, int N>
__device__ __forceinline__ int pa_close_stage(double (&v)[N], int lane) {
    if constexpr (M == 0) {
        return 0;
    } else if constexpr (CNT > 1) {
        constexpr int half = CNT / 2;
        const bool up = (lane & M) != 0;
#pragma unroll
        for (int j = 0; j < half; ++j) {
            const double keep = up ? v[j + half] : v[j];
            const double send = up ? v[j] : v[j + half];
            v[j] = keep + __shfl_xor(send, M);
        }
        return (up ? half : 0) + pa_close_stage<half, M / 2, N>(v, lane);
    } else {
        v[0] += __shfl_xor(v[0], M);
        return pa_close_stage<1, M / 2, N>(v, lane);
    }
}

// FORM 0: U, T, S real; 1: all complex128.  G: amplitudes per load of U.
template <int FORM, int G>
__global__ __launch_bounds__(256) void pair_contract_antisym_kernel(const PaArgs g) {
    constexpr int W = FORM == 1 ? 2 : 1;                   // doubles per element of U, T and S
    constexpr int TA = kPaRows;
    constexpr int RW = pa_record_words(FORM, G);
    constexpr int NS = kPaSteps;
    constexpr int CW = NS * 64 * RW;                       // doubles of one buffer
    constexpr int NV = TA * G * W;
    typedef typename std::conditional<FORM == 1, f64x2, double>::type elem_t;
    extern __shared__ __attribute__((aligned(16))) double pa_lds[];

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int l = g.l;
    const int n = l * (l - 1) / 2;                          // packed positions of a row = pair rows of U
    const int nsteps = (n + 63) >> 6, nchunks = (nsteps + NS - 1) / NS;
    const int row0 = __builtin_amdgcn_readfirstlane((blockIdx.x * 4 + wave) * TA);

    // the wave's rows: (p, q) of pair row0 + i, or the last pair for a row past the end (loaded, never stored)
    const elem_t* urow[TA];
    int rp[TA], rq[TA];
#pragma unroll
    for (int i = 0; i < TA; ++i) {
        const int row = row0 + i < n ? row0 + i : n - 1;
        int p, q;
        pa_unpack(row, l, p, q);
        rp[i] = __builtin_amdgcn_readfirstlane(p);
        rq[i] = __builtin_amdgcn_readfirstlane(q);
        urow[i] = reinterpret_cast<const elem_t*>(g.U) + ((int64_t)rp[i] * l + rq[i]) * g.ldu;
    }

    // T values of chunk c -> buffer c & 1, packed in the order of the walk: zero past n and past the launch's amplitudes
    auto stage = [&](int c) {
        double* buf = pa_lds + (c & 1) * CW;
        for (int idx = tid; idx < NS * 64; idx += 256) {
            const int t = c * (NS * 64) + idx;
            const bool ok = t < n;
            int r, s;
            pa_unpack(ok ? t : 0, l, r, s);
            const double* src = g.T + (int64_t)(r * l + s) * W;
            double* dst = buf + idx * RW;
#pragma unroll
            for (int gg = 0; gg < G; ++gg) {
                const bool use = ok && gg < g.ng;
                const double* sg = src + (use ? (int64_t)gg * l * l * W : 0);
#pragma unroll
                for (int w = 0; w < W; ++w) {
                    const double v = sg[w];
                    dst[gg * W + w] = use ? v : 0.0;
                }
            }
        }
    };

    double acc[NV];
#pragma unroll
    for (int j = 0; j < NV; ++j) acc[j] = 0.0;

    // the lane's position: t = 64 st + lane <-> (r, s); off = r l + s, position 0 (element (0, 1)) once t is past n
    int t = lane, r = 0, s = 1;
    if (t < n) pa_unpack(t, l, r, s);
    auto offset = [&]() { return t < n ? (unsigned)(r * l + s) : 1u; };
    auto advance = [&]() {
        t += 64;
        if (t < n) {
            s += 64;
            while (s >= l) {
                s += r + 2 - l;
                ++r;
            }
        }
    };
    auto fetch = [&](elem_t (&dst)[TA]) {
        const unsigned off = offset();
#pragma unroll
        for (int i = 0; i < TA; ++i) dst[i] = urow[i][off];
    };

    elem_t cur[TA], nxt[TA];
    fetch(cur);
#pragma unroll
    for (int i = 0; i < TA; ++i) nxt[i] = cur[i];
    stage(0);
    __syncthreads();

    for (int c = 0; c < nchunks; ++c) {
        if (c + 1 < nchunks) stage(c + 1);
        const double* buf = pa_lds + (c & 1) * CW;
        const int s_hi = nsteps - c * NS < NS ? nsteps - c * NS : NS;
        for (int ss = 0; ss < s_hi; ++ss) {
            const int st = c * NS + ss;
            const bool mine = t < n;                        // this step's position is a term of the sum
            advance();
            if (st + 1 < nsteps) fetch(nxt);
            const double* rec = buf + (ss * 64 + lane) * RW;
            double tv[G * W];
#pragma unroll
            for (int j = 0; j < G * W; ++j) tv[j] = rec[j];
#pragma unroll
            for (int i = 0; i < TA; ++i) {
                if constexpr (FORM == 0) {
                    const double v = mine ? cur[i] : 0.0;
#pragma unroll
                    for (int q = 0; q < G; ++q) acc[i * G + q] = fma(v, tv[q], acc[i * G + q]);
                } else {
                    f64x2 v = cur[i];
                    if (!mine) v = f64x2{0.0, 0.0};
#pragma unroll
                    for (int q = 0; q < G; ++q) {
                        double* a = acc + (i * G + q) * 2;
                        a[0] = fma(-v.y, tv[2 * q + 1], fma(v.x, tv[2 * q], a[0]));
                        a[1] = fma(v.y, tv[2 * q], fma(v.x, tv[2 * q + 1], a[1]));
                    }
                }
            }
#pragma unroll
            for (int i = 0; i < TA; ++i) cur[i] = nxt[i];
        }
        __syncthreads();
    }

    // close the wave's sums; the lane that holds value (i, q, w) doubles it and stores it, its mirror and its zeros
    const int idx = pa_close_stage<NV, 32, NV>(acc, lane);
    const int w = idx % W, q = (idx / W) % G, i = idx / (W * G);
    const bool first = NV >= 64 || (lane & (64 / NV - 1)) == 0;       // the lanes below a halving-stage bit hold copies
    if (first && q < g.ng && row0 + i < n) {
        int pp = rp[0], qq = rq[0];
#pragma unroll
        for (int j = 1; j < TA; ++j)
            if (i == j) { pp = rp[j]; qq = rq[j]; }
        double* Sk = g.S + (int64_t)q * l * l * W + w;
        const double v = 2.0 * acc[0];
        Sk[((int64_t)pp * l + qq) * W] = v;
        Sk[((int64_t)qq * l + pp) * W] = -v;
        if (qq == pp + 1) Sk[((int64_t)pp * l + pp) * W] = 0.0;          // the first pair of p owns (p, p)
        if (pp == l - 2) Sk[((int64_t)qq * l + qq) * W] = 0.0;           // ... the last pair (l - 2, l - 1) also (l - 1, l - 1)
    }
}

// One group of g.ng amplitudes on the smallest instantiation that holds it.
static void pa_launch(int form, const PaArgs& g, unsigned grid, hipStream_t s) {
    with_width(form + 1, [&](auto WW) {
        constexpr int F = decltype(WW)::value - 1;
        with_group(g.ng, [&](auto G) {
            hipLaunchKernelGGL((pair_contract_antisym_kernel<F, G>), dim3(grid), dim3(256), pa_lds_bytes(F, G), s, g);
            note_dispatch("qs::pair_contract_antisym_kernel<%d, %d>", F, (int)G);
        });
    });
}

// The two forms: both operands fp64, or both complex128 (a real U against complex T is two fp64 columns per amplitude)
static inline int pa_form(int u_dtype, int t_dtype) {
    if (!dtype_ok(u_dtype) || !dtype_ok(t_dtype) || u_dtype != t_dtype) return QS_ERR_BAD_DTYPE;
    return u_dtype == QS_C128 ? 1 : 0;
}

static inline bool pa_extents_ok(int64_t l, int64_t K) { return l >= 2 && l <= kPaMaxL && K >= 1 && K <= 65536; }

}  // namespace qs

using namespace qs;

extern "C" {

int64_t qs_pair_contract_antisym_workspace(int u_dtype, int t_dtype, int64_t l, int64_t K) {
    const int form = pa_form(u_dtype, t_dtype);
    if (form < 0) return form;
    if (!pa_extents_ok(l, K)) return QS_ERR_BAD_EXTENT;
    return 0;          // the triangle of a row is never split: every sum is closed inside its wave
}

int qs_pair_contract_antisym(int u_dtype, int t_dtype, const void* U, const void* T, void* S, int64_t l, int64_t K,
                             int64_t ldu, void* work, int64_t work_elems, void* stream) {
    dispatch_reset();
    (void)work;
    const int form = pa_form(u_dtype, t_dtype);
    if (form < 0) return form;
    if (!pa_extents_ok(l, K) || ldu < l * l || ldu > (int64_t(1) << 24)) return QS_ERR_BAD_EXTENT;
    if (!U || !T || !S) return QS_ERR_NULL_POINTER;
    const int64_t es = (int64_t)elem_size(t_dtype);
    if (!aligned(U, (size_t)es) || !aligned(T, (size_t)es) || !aligned(S, (size_t)es)) return QS_ERR_MISALIGNED;
    const int64_t s_bytes = K * l * l * es;
    if (overlaps(S, s_bytes, U, ((l * l - 1) * ldu + l * l) * es) || overlaps(S, s_bytes, T, s_bytes)) return QS_ERR_ALIAS;
    if (work_elems < qs_pair_contract_antisym_workspace(u_dtype, t_dtype, l, K)) return QS_ERR_WORKSPACE;

    const int w = form + 1;
    PaArgs g{};
    g.U = (const double*)U;
    g.l = (int)l;
    g.ldu = ldu;
    const unsigned grid = (unsigned)cdiv(l * (l - 1) / 2, 4 * kPaRows);
    hipStream_t s = (hipStream_t)stream;
    return for_each_group(K, group_size(g_tune.pair_contract_g, kPaGroup[form]), [&](int64_t k0, int ng) {
        g.ng = ng;
        g.T = (const double*)T + k0 * l * l * w;
        g.S = (double*)S + k0 * l * l * w;
        pa_launch(form, g, grid, s);
        return launch_status("pair contract antisym launch");
    });
}

}  // extern "C"
