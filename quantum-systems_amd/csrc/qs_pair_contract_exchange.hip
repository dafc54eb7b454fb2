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
// step's fmas.  A lane carries its (r, s) along (PairCursor<true> of qs_pair_walk.h): only the first position of a lane,
// the staging and a wave's (p, q) invert the triangle map (pair_unpack<true>: qs_triangle.h's map).  A diagonal pair
// p = q loads its row twice and needs no arithmetic of its own:
// u- = +0.  T is staged in LDS already combined and packed in the order of the walk, as [position][g][+-] (records
// padded to an odd number of 16-byte units), the halved diagonal of T+ applied there (exact), two buffers, chunk c + 1
// staged while chunk c is consumed (pair_chunk_walk).  A lane past the end of the triangle, and a wave pair past the last
// pair, re-reads an element of the half (position 0 / the last pair) and drops it by a select.
// After the last step a wave closes its S+ and its S- sums with the same xor butterfly over masks 32 ... 1 in which every
// stage also halves the values a lane carries (pair_close), so that one lane is left
// with S+ and S- of the same (pair, g); it forms (S+ +- S-) / 2 and stores (p, q) and (q, p): plain vector stores, no
// atomics, no workspace, no closing launch.
//
// Reproducible: every product is an explicit fma in a fixed order, a row's positions are dealt to the lanes by l alone
// and every sum goes through the same butterfly stages whatever G.  So S[k] has the same bits alone, anywhere in a batch
// and under any group size; a non-finite value stays in its row pair of U or its T[k].  If T[k] equals its transpose
// bit for bit, T- and with it S- is a zero and (p, q), (q, p) get the same bits; if T[k] = -T[k]^T, S+ is +0 and they
// differ in the sign bit only.

#include "qs_pair_walk.h"

namespace qs {

constexpr int kPxPairs = 2;            // row pairs per wave (four row loads per step); a workgroup takes 4 * kPxPairs of them
// Shipped group size per form {fp64, complex128}: the largest that keeps two workgroups per CU in VGPRs and in LDS
constexpr int kPxGroup[2] = {8, 8};
// steps of 64 positions per staged chunk of T, per form: the record of a position is twice the antisym kernel's
static constexpr int px_steps(int form) { return form == 1 ? 2 : 3; }

// doubles of one position's record in LDS: G * 2 * W (T+ and T- of every amplitude), padded to an odd number of 16-byte units
static constexpr int px_record_words(int form, int G) { return ((G * (form == 1 ? 2 : 1)) | 1) * 2; }

static constexpr size_t px_lds_bytes(int form, int G) {
    return (size_t)2 * px_steps(form) * 64 * px_record_words(form, G) * 8;
}

// FORM 0: U, T, S real; 1: all complex128.  G: amplitudes per load of U.
template <int FORM, int G>
__global__ __launch_bounds__(256) void pair_contract_exchange_kernel(const PairTriArgs g) {
    constexpr int W = FORM == 1 ? 2 : 1;                   // doubles per element of U, T and S
    constexpr int TP = kPxPairs;
    constexpr int RW = px_record_words(FORM, G);
    constexpr int NS = px_steps(FORM);
    constexpr int CW = NS * 64 * RW;                       // doubles of one buffer
    constexpr int NH = TP * G * W;                         // sums of one sign
    typedef typename std::conditional<FORM == 1, f64x2, double>::type elem_t;
    typedef PairCursor<true> Cursor;
    extern __shared__ __attribute__((aligned(16))) double px_lds[];

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int l = g.l;
    const int n = pair_count<true>(l);                      // packed positions of a row = row pairs of U
    const int pair0 = __builtin_amdgcn_readfirstlane((blockIdx.x * 4 + wave) * TP);

    // the wave's pairs: (p, q) of pair pair0 + i, or the last pair for one past the end (loaded, never stored)
    const elem_t* ua[TP];
    const elem_t* ub[TP];
#pragma unroll
    for (int i = 0; i < TP; ++i) {
        const int pr = pair0 + i < n ? pair0 + i : n - 1;
        int p, q;
        pair_unpack<true>(pr, l, p, q);
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
            const Cursor at(c * (NS * 64) + idx, l);
            const bool ok = at.term();
            const double* src = g.T + (int64_t)(at.r * l + at.s) * W;
            const double* mir = g.T + (int64_t)(at.s * l + at.r) * W;
            const double wt = at.r == at.s ? 0.5 : 1.0;
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

    // the lane's position t = 64 st + lane of the step that is fetched next
    Cursor pos(lane, l);
    auto fetch = [&](elem_t (&da)[TP], elem_t (&db)[TP]) {
        const unsigned off = pos.offset();
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
    bool mine = pos.term();                                 // the position in `ca`, `cb` is a term of the sum
    pos.advance();

    pair_chunk_walk<NS>(
        (n + 63) >> 6, stage, [&](int) { fetch(na, nb); },
        [&](int b, int ss, int) {
            const double* rec = px_lds + b * CW + (ss * 64 + lane) * RW;
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
            mine = pos.term();
            pos.advance();
        });

    // close the wave's sums: both signs through the same stages, so that value (i, q, w) of S+ and of S- end in one lane,
    // which forms the two results and stores them
    const int idx = pair_close<NH>(accp, lane);
    (void)pair_close<NH>(accm, lane);
    const int w = idx % W, q = (idx / W) % G, i = idx / (W * G);
    const bool first = NH >= 64 || (lane & (64 / NH - 1)) == 0;       // the lanes below a halving-stage bit hold copies
    if (first && q < g.ng && pair0 + i < n) {
        int pp, qq;
        pair_unpack<true>(pair0 + i, l, pp, qq);            // once per stored value: cheaper than carrying every (p, q) along
        double* Sk = g.S + (int64_t)q * l * l * W + w;
        Sk[((int64_t)pp * l + qq) * W] = (accp[0] + accm[0]) * 0.5;
        if (pp != qq) Sk[((int64_t)qq * l + pp) * W] = (accp[0] - accm[0]) * 0.5;
    }
}

// One group of g.ng amplitudes on the smallest instantiation that holds it.
static int px_launch(int form, const PairTriArgs& g, unsigned grid, hipStream_t s) {
    return with_width(form + 1, [&](auto WW) {
        constexpr int F = decltype(WW)::value - 1;
        return with_group(g.ng, [&](auto G) {
            static PerDeviceLds once;
            return pair_launch(pair_contract_exchange_kernel<F, G>, g, px_lds_bytes(F, G), once, grid, s,
                               "hipFuncSetAttribute(pair_contract_exchange)", "pair contract exchange launch",
                               "qs::pair_contract_exchange_kernel<%d, %d>", F, (int)G);
        });
    });
}

}  // namespace qs

using namespace qs;

extern "C" {

int64_t qs_pair_contract_exchange_workspace(int u_dtype, int t_dtype, int64_t l, int64_t K) {
    return pair_tri_workspace<true>(u_dtype, t_dtype, l, K);
}

int qs_pair_contract_exchange(int u_dtype, int t_dtype, const void* U, const void* T, void* S, int64_t l, int64_t K,
                              int64_t ldu, void* work, int64_t work_elems, void* stream) {
    (void)work;
    return pair_tri_entry<true>(4 * kPxPairs, kPxGroup, px_launch, u_dtype, t_dtype, U, T, S, l, K, ldu, work_elems, stream);
}

}  // extern "C"
