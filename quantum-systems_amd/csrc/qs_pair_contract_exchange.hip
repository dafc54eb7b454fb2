// Pair contraction of a tensor with particle-exchange symmetry, U[p,q,r,s] = U[q,p,s,r] (no conjugation: the two-body
// integrals of spatial orbitals), with ANY amplitudes, from the half of the tensor that the symmetry does not repeat:
//   S[k,p,q] = sum_rs U[p,q,r,s] T[k,r,s]      for all p, q
// U is (l, l, l, l) with consecutive (p, q) rows ldu >= l^2 elements apart, T and S are (K, l, l).  Only the elements of
// U with r <= s are ever addressed; all of T is read.  For p <= q and r <= s, with
//   a = U[p,q,r,s],   b = U[q,p,r,s] (= U[p,q,s,r] by the symmetry: the SAME column of the mirror row)
//   u+- = a +- b,     T+-[r,s] = T[r,s] +- T[s,r],     w_rs = 1/2 on the diagonal, 1 off it
//   S+-[p,q] = sum_{r<=s} w_rs u+-[pq,rs] T+-[r,s]
// the result is S[p,q] = (S+ + S-) / 2 and S[q,p] = (S+ - S-) / 2: half the bytes and half the fmas of the full sum.
// The particle-particle ladder of spin-adapted closed-shell coupled-cluster doubles on the untransformed tensor.
//
// The r <= s part of a row is l runs of l - r elements that start at r l + r: at any 8-byte alignment, so the unit of a
// load is ONE element.  The kernel walks the PACKED triangle WITH its diagonal, t = 0 ... n - 1, n = l (l + 1) / 2,
// t <-> (r, s) in row-major order of the runs.  A workgroup of 256 threads takes 8 consecutive row PAIRS {(p,q), (q,p)},
// p <= q, row-major over the same triangle, wave w the kPxPairs pairs from pair 2 w of them: four row loads per step, the
// 64 lanes on 64 consecutive packed positions of ONE row per load, the next step's elements issued before the current
// step's fmas.  A lane carries its (r, s) along (qs_pair_contract_antisym.hip): only the first position of a lane and
// the staging invert the triangle map.  A diagonal pair p = q loads its row twice and needs no arithmetic of its own:
// u- = +0.  T is staged in LDS already combined and packed in the order of the walk, as [position][g][+-] (records
// padded to an odd number of 16-byte units), the halved diagonal of T+ applied there (exact), two buffers, chunk c + 1
// staged while chunk c is consumed.  A lane past the end of the triangle, and a wave pair past the last pair, re-reads
// an element of the half (position 0 / the last pair) and drops it by a select.
// After the last step a wave closes its S+ and its S- sums with the same xor butterfly over masks 32 ... 1 in which every
// stage also halves the values a lane carries (the reduce-scatter of qs_pair_contract.hip), so that one lane is left
// with S+ and S- of the same (pair, g); it forms (S+ +- S-) / 2 and stores (p, q) and (q, p): plain vector stores, no
// atomics, no workspace, no closing launch.
//
// Reproducible: every product is an explicit fma in a fixed order, a row's positions are dealt to the lanes by l alone
// and every sum goes through the same butterfly stages whatever G.  So S[k] has the same bits alone, anywhere in a batch
// and under any group size; a non-finite value stays in its row pair of U or its T[k].  If T[k] equals its transpose
// bit for bit, T- and with it S- is a zero and (p, q), (q, p) get the same bits; if T[k] = -T[k]^T, S+ is +0 and they
// differ in the sign bit only.

#include "qs_contract_common.h"

namespace qs {

constexpr int kPxPairs = 2;            // row pairs per wave (four row loads per step); a workgroup takes 4 * kPxPairs of them
constexpr int64_t kPxMaxL = 4096;      // l^2 <= 2^24 elements: every byte offset inside a row stays below 2^32
// Shipped group size per form {fp64, complex128}: the largest that keeps two workgroups per CU in VGPRs and in LDS
constexpr int kPxGroup[2] = {8, 8};
// steps of 64 positions per staged chunk of T, per form: the record of a position is twice the antisym kernel's
static constexpr int px_steps(int form) { return form == 1 ? 2 : 3; }

struct PxArgs {
    const double* U;
    const double* T;          // first amplitude of the group, [ng][l][l]
    double* S;                // first result of the group, [ng][l][l]
    int64_t ldu;
    int l, ng;                // ng: amplitudes of this launch, 1 ... G of the instantiation
};

// First packed position of run r: the elements (r, r ... l - 1) follow those of the runs before it
__host__ __device__ inline int px_run_start(int r, int l) { return (int)(((int64_t)r * (2 * l - r + 1)) / 2); }

// (r, s) of packed position t < l (l + 1) / 2: the root of the quadratic, then a correction of its rounding
__host__ __device__ inline void px_unpack(int t, int l, int& r, int& s) {
    const double b = 2.0 * l + 1.0;
    int rr = (int)((b - sqrt(b * b - 8.0 * t)) * 0.5);
    if (rr < 0) rr = 0;
    if (rr > l - 1) rr = l - 1;
    while (rr > 0 && px_run_start(rr, l) > t) --rr;
    while (rr < l - 1 && px_run_start(rr + 1, l) <= t) ++rr;
    r = rr;
    s = rr + (t - px_run_start(rr, l));
}

// doubles of one position's record in LDS: G * 2 * W (T+ and T- of every amplitude), padded to an odd number of 16-byte units
static constexpr int px_record_words(int form, int G) { return ((G * (form == 1 ? 2 : 1)) | 1) * 2; }

static constexpr size_t px_lds_bytes(int form, int G) {
    return (size_t)2 * px_steps(form) * 64 * px_record_words(form, G) * 8;
}

// Sum of v[j] over the 64 lanes for every j, N a power of two <= 64 (as pc_close of qs_pair_contract.hip and pa_close_stage
// of qs_pair_contract_antisym.hip): butterfly stages 32 ... 1; while a lane carries more than one value a stage hands half
// of them to the partner lane.  Returns the index j of the finished sum left in v[0]: a function of the lane alone.
template <int CNT, int M, int N>
__device__ __forceinline__ int px_close_stage(double (&v)[N], int lane) {
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
        return (up ? half : 0) + px_close_stage<half, M / 2, N>(v, lane);
    } else {
        v[0] += __shfl_xor(v[0], M);
        return px_close_stage<1, M / 2, N>(v, lane);
    }
}

// FORM 0: U, T, S real; 1: all complex128.  G: amplitudes per load of U.
template <int FORM, int G>
__global__ __launch_bounds__(256) void pair_contract_exchange_kernel(const PxArgs g) {
    constexpr int W = FORM == 1 ? 2 : 1;                   // doubles per element of U, T and S
    constexpr int TP = kPxPairs;
    constexpr int RW = px_record_words(FORM, G);
    constexpr int NS = px_steps(FORM);
    constexpr int CW = NS * 64 * RW;                       // doubles of one buffer
    constexpr int NH = TP * G * W;                         // sums of one sign
    typedef typename std::conditional<FORM == 1, f64x2, double>::type elem_t;
    extern __shared__ __attribute__((aligned(16))) double px_lds[];

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int l = g.l;
    const int n = l * (l + 1) / 2;                          // packed positions of a row = row pairs of U
    const int nsteps = (n + 63) >> 6, nchunks = (nsteps + NS - 1) / NS;
    const int pair0 = __builtin_amdgcn_readfirstlane((blockIdx.x * 4 + wave) * TP);

    // the wave's pairs: (p, q) of pair pair0 + i, or the last pair for one past the end (loaded, never stored)
    const elem_t* ua[TP];
    const elem_t* ub[TP];
#pragma unroll
    for (int i = 0; i < TP; ++i) {
        const int pr = pair0 + i < n ? pair0 + i : n - 1;
        int p, q;
        px_unpack(pr, l, p, q);
        p = __builtin_amdgcn_readfirstlane(p);
        q = __builtin_amdgcn_readfirstlane(q);
        ua[i] = reinterpret_cast<const elem_t*>(g.U) + ((int64_t)p * l + q) * g.ldu;
        ub[i] = reinterpret_cast<const elem_t*>(g.U) + ((int64_t)q * l + p) * g.ldu;
    }

    // T+ (its diagonal halved) and T- of chunk c -> buffer c & 1, packed in the order of the walk: zero past n and past
    // the launch's amplitudes
    auto stage = [&](int c) {
        double* buf = px_lds + (c & 1) * CW;
        for (int idx = tid; idx < NS * 64; idx += 256) {
            const int t = c * (NS * 64) + idx;
            const bool ok = t < n;
            int r, s;
            px_unpack(ok ? t : 0, l, r, s);
            const double* src = g.T + (int64_t)(r * l + s) * W;
            const double* mir = g.T + (int64_t)(s * l + r) * W;
            const double wt = r == s ? 0.5 : 1.0;
            double* dst = buf + idx * RW;
#pragma unroll
            for (int gg = 0; gg < G; ++gg) {
                const bool use = ok && gg < g.ng;
                const int64_t go = use ? (int64_t)gg * l * l * W : 0;
#pragma unroll
                for (int w = 0; w < W; ++w) {
                    const double x = src[go + w], y = mir[go + w];
                    dst[(gg * 2 + 0) * W + w] = use ? (x + y) * wt : 0.0;
                    dst[(gg * 2 + 1) * W + w] = use ? x - y : 0.0;
                }
            }
        }
    };

    double accp[NH], accm[NH];
#pragma unroll
    for (int j = 0; j < NH; ++j) accp[j] = accm[j] = 0.0;

    // the lane's position: t = 64 st + lane <-> (r, s); off = r l + s, position 0 (element (0, 0)) once t is past n
    int t = lane, r = 0, s = 0;
    if (t < n) px_unpack(t, l, r, s);
    auto offset = [&]() { return t < n ? (unsigned)(r * l + s) : 0u; };
    auto advance = [&]() {
        t += 64;
        if (t < n) {
            s += 64;
            while (s >= l) {
                s += r + 1 - l;
                ++r;
            }
        }
    };
    auto fetch = [&](elem_t (&da)[TP], elem_t (&db)[TP]) {
        const unsigned off = offset();
#pragma unroll
        for (int i = 0; i < TP; ++i) {
            da[i] = ua[i][off];
            db[i] = ub[i][off];
        }
    };

    elem_t ca[TP], cb[TP], na[TP], nb[TP];
    fetch(ca, cb);
#pragma unroll
    for (int i = 0; i < TP; ++i) {
        na[i] = ca[i];
        nb[i] = cb[i];
    }
    stage(0);
    __syncthreads();

    for (int c = 0; c < nchunks; ++c) {
        if (c + 1 < nchunks) stage(c + 1);
        const double* buf = px_lds + (c & 1) * CW;
        const int s_hi = nsteps - c * NS < NS ? nsteps - c * NS : NS;
        for (int ss = 0; ss < s_hi; ++ss) {
            const int st = c * NS + ss;
            const bool mine = t < n;                        // this step's position is a term of the sum
            advance();
            if (st + 1 < nsteps) fetch(na, nb);
            const double* rec = buf + (ss * 64 + lane) * RW;
            double tv[2 * G * W];
#pragma unroll
            for (int j = 0; j < 2 * G * W; ++j) tv[j] = rec[j];
#pragma unroll
            for (int i = 0; i < TP; ++i) {
                if constexpr (FORM == 0) {
                    const double up = mine ? ca[i] + cb[i] : 0.0;
                    const double um = mine ? ca[i] - cb[i] : 0.0;
#pragma unroll
                    for (int q = 0; q < G; ++q) {
                        accp[i * G + q] = fma(up, tv[2 * q], accp[i * G + q]);
                        accm[i * G + q] = fma(um, tv[2 * q + 1], accm[i * G + q]);
                    }
                } else {
                    f64x2 up = f64x2{ca[i].x + cb[i].x, ca[i].y + cb[i].y};
                    f64x2 um = f64x2{ca[i].x - cb[i].x, ca[i].y - cb[i].y};
                    if (!mine) up = um = f64x2{0.0, 0.0};
#pragma unroll
                    for (int q = 0; q < G; ++q) {
                        double* ap = accp + (i * G + q) * 2;
                        double* am = accm + (i * G + q) * 2;
                        const double* tp = tv + 4 * q;
                        ap[0] = fma(-up.y, tp[1], fma(up.x, tp[0], ap[0]));
                        ap[1] = fma(up.y, tp[0], fma(up.x, tp[1], ap[1]));
                        am[0] = fma(-um.y, tp[3], fma(um.x, tp[2], am[0]));
                        am[1] = fma(um.y, tp[2], fma(um.x, tp[3], am[1]));
                    }
                }
            }
#pragma unroll
            for (int i = 0; i < TP; ++i) {
                ca[i] = na[i];
                cb[i] = nb[i];
            }
        }
        __syncthreads();
    }

    // close the wave's sums: both signs through the same stages, so that value (i, q, w) of S+ and of S- end in one lane,
    // which forms the two results and stores them
    const int idx = px_close_stage<NH, 32, NH>(accp, lane);
    (void)px_close_stage<NH, 32, NH>(accm, lane);
    const int w = idx % W, q = (idx / W) % G, i = idx / (W * G);
    const bool first = NH >= 64 || (lane & (64 / NH - 1)) == 0;       // the lanes below a halving-stage bit hold copies
    if (first && q < g.ng && pair0 + i < n) {
        int pp, qq;
        px_unpack(pair0 + i, l, pp, qq);                    // once per stored value: cheaper than carrying every (p, q) along
        double* Sk = g.S + (int64_t)q * l * l * W + w;
        Sk[((int64_t)pp * l + qq) * W] = (accp[0] + accm[0]) * 0.5;
        if (pp != qq) Sk[((int64_t)qq * l + pp) * W] = (accp[0] - accm[0]) * 0.5;
    }
}

// One group of g.ng amplitudes on the smallest instantiation that holds it.
static int px_launch(int form, const PxArgs& g, unsigned grid, hipStream_t s) {
    return with_width(form + 1, [&](auto WW) {
        constexpr int F = decltype(WW)::value - 1;
        return with_group(g.ng, [&](auto G) {
            constexpr size_t lds = px_lds_bytes(F, G);
            static PerDeviceLds lds_opt_in;
            if (int rc = opt_in_dynamic_lds((const void*)pair_contract_exchange_kernel<F, G>, lds, lds_opt_in,
                                            "hipFuncSetAttribute(pair_contract_exchange)"))
                return rc;
            hipLaunchKernelGGL((pair_contract_exchange_kernel<F, G>), dim3(grid), dim3(256), lds, s, g);
            note_dispatch("qs::pair_contract_exchange_kernel<%d, %d>", F, (int)G);
            return launch_status("pair contract exchange launch");
        });
    });
}

// The two forms: both operands fp64, or both complex128 (a real U against complex T is two fp64 columns per amplitude)
static inline int px_form(int u_dtype, int t_dtype) {
    if (!dtype_ok(u_dtype) || !dtype_ok(t_dtype) || u_dtype != t_dtype) return QS_ERR_BAD_DTYPE;
    return u_dtype == QS_C128 ? 1 : 0;
}

static inline bool px_extents_ok(int64_t l, int64_t K) { return l >= 1 && l <= kPxMaxL && K >= 1 && K <= 65536; }

}  // namespace qs

using namespace qs;

extern "C" {

int64_t qs_pair_contract_exchange_workspace(int u_dtype, int t_dtype, int64_t l, int64_t K) {
    const int form = px_form(u_dtype, t_dtype);
    if (form < 0) return form;
    if (!px_extents_ok(l, K)) return QS_ERR_BAD_EXTENT;
    return 0;          // the triangle of a row is never split: every sum is closed inside its wave
}

int qs_pair_contract_exchange(int u_dtype, int t_dtype, const void* U, const void* T, void* S, int64_t l, int64_t K,
                              int64_t ldu, void* work, int64_t work_elems, void* stream) {
    dispatch_reset();
    (void)work;
    const int form = px_form(u_dtype, t_dtype);
    if (form < 0) return form;
    if (!px_extents_ok(l, K) || ldu < l * l || ldu > (int64_t(1) << 24)) return QS_ERR_BAD_EXTENT;
    if (!U || !T || !S) return QS_ERR_NULL_POINTER;
    const int64_t es = (int64_t)elem_size(t_dtype);
    if (!aligned(U, (size_t)es) || !aligned(T, (size_t)es) || !aligned(S, (size_t)es)) return QS_ERR_MISALIGNED;
    const int64_t s_bytes = K * l * l * es;
    if (overlaps(S, s_bytes, U, ((l * l - 1) * ldu + l * l) * es) || overlaps(S, s_bytes, T, s_bytes)) return QS_ERR_ALIAS;
    if (work_elems < qs_pair_contract_exchange_workspace(u_dtype, t_dtype, l, K)) return QS_ERR_WORKSPACE;

    const int w = form + 1;
    PxArgs g{};
    g.U = (const double*)U;
    g.l = (int)l;
    g.ldu = ldu;
    const unsigned grid = (unsigned)cdiv(l * (l + 1) / 2, 4 * kPxPairs);
    hipStream_t s = (hipStream_t)stream;
    return for_each_group(K, group_size(g_tune.pair_contract_g, kPxGroup[form]), [&](int64_t k0, int ng) {
        g.ng = ng;
        g.T = (const double*)T + k0 * l * l * w;
        g.S = (double*)S + k0 * l * l * w;
        return px_launch(form, g, grid, s);
    });
}

}  // extern "C"
