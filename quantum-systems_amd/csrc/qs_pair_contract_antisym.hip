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
// (r, s) along (PairCursor<false> of qs_pair_walk.h), so only the first position of a lane needs the inverse of the
// triangle map (pair_unpack<false>: qs_triangle.h's map of l - 1).  The T values of a chunk of kPaSteps steps are staged
// in LDS already packed in the order of the walk, as [position][g] (records padded to an odd number of 16-byte units), two
// buffers, chunk c + 1 staged while chunk c is consumed (pair_chunk_walk): the staging threads and the wave's (p, q) are
// the only other users of the map.
// A lane past the end of the triangle, and a wave row past the last pair, re-reads an element of the quarter (position
// 0 / the last pair row) and drops it by a select.
// After the last step a wave closes its kPaRows * G row sums with one xor butterfly over masks 32 ... 1 in which every
// stage also halves the values a lane carries (pair_close); the lane left with the sum
// of (row, g) doubles it -- exact -- and stores it at (p, q), its negation at (q, p) and the zeros of the diagonal that
// its row owns: plain vector stores, no atomics, no workspace, no closing launch.
//
// Reproducible: every product is an explicit fma in a fixed order, a row's positions are dealt to the lanes by l alone
// and every sum goes through the same butterfly stages whatever G.  So S[k] has the same bits alone, anywhere in a batch
// and under any group size; a non-finite value stays in its row of U or its T[k].

#include "qs_pair_walk.h"

namespace qs {

constexpr int kPaRows = 4;             // pair rows per wave; a workgroup takes 4 * kPaRows of them
constexpr int kPaSteps = 3;            // steps of 64 positions per staged chunk of T
// Shipped group size per form {fp64, complex128}: the largest that keeps two workgroups per CU in VGPRs and in LDS
constexpr int kPaGroup[2] = {8, 8};

// doubles of one position's record in LDS: G * AW, padded to an odd number of 16-byte units
static constexpr int pa_record_words(int form, int G) { return (((G * form_widths(form).aw) / 2) | 1) * 2; }

static constexpr size_t pa_lds_bytes(int form, int G) {
    return (size_t)2 * kPaSteps * 64 * pa_record_words(form, G) * 8;
}

// FORM 0: U, T, S real; 1: all complex128.  G: amplitudes per load of U.
template <int FORM, int G>
__global__ __launch_bounds__(256) void pair_contract_antisym_kernel(const PairTriArgs g) {
    constexpr int W = FORM == 1 ? 2 : 1;                   // doubles per element of U, T and S
    constexpr int TA = kPaRows;
    constexpr int RW = pa_record_words(FORM, G);
    constexpr int NS = kPaSteps;
    constexpr int CW = NS * 64 * RW;                       // doubles of one buffer
    constexpr int NV = TA * G * W;
    typedef typename std::conditional<FORM == 1, f64x2, double>::type elem_t;
    typedef PairCursor<false> Cursor;
    extern __shared__ __attribute__((aligned(16))) double pa_lds[];

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int l = g.l;
    const int n = pair_count<false>(l);                     // packed positions of a row = pair rows of U
    const int row0 = __builtin_amdgcn_readfirstlane((blockIdx.x * 4 + wave) * TA);

    // the wave's rows: (p, q) of pair row0 + i, or the last pair for a row past the end (loaded, never stored)
    const elem_t* urow[TA];
    int rp[TA], rq[TA];
#pragma unroll
    for (int i = 0; i < TA; ++i) {
        const int row = row0 + i < n ? row0 + i : n - 1;
        int p, q;
        pair_unpack<false>(row, l, p, q);
        rp[i] = __builtin_amdgcn_readfirstlane(p);
        rq[i] = __builtin_amdgcn_readfirstlane(q);
        urow[i] = reinterpret_cast<const elem_t*>(g.U) + ((int64_t)rp[i] * l + rq[i]) * g.ldu;
    }

    // T values of chunk c -> buffer c & 1, packed in the order of the walk: zero past n and past the launch's amplitudes
    auto stage = [&](int c) {
        double* buf = pa_lds + (c & 1) * CW;
        for (int idx = tid; idx < NS * 64; idx += 256) {
            const Cursor at(c * (NS * 64) + idx, l);
            const bool ok = at.term();
            const double* src = g.T + (int64_t)at.offset() * W;
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

    // the lane's position t = 64 st + lane of the step that is fetched next
    Cursor pos(lane, l);
    auto fetch = [&](elem_t (&dst)[TA]) {
        const unsigned off = pos.offset();
#pragma unroll
        for (int i = 0; i < TA; ++i) dst[i] = urow[i][off];
    };

    elem_t cur[TA], nxt[TA];
    fetch(cur);
#pragma unroll
    for (int i = 0; i < TA; ++i) nxt[i] = cur[i];
    bool mine = pos.term();                                 // the position in `cur` is a term of the sum
    pos.advance();

    pair_chunk_walk<NS>(
        (n + 63) >> 6, stage, [&](int) { fetch(nxt); },
        [&](int b, int ss, int) {
            const double* rec = pa_lds + b * CW + (ss * 64 + lane) * RW;
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
            mine = pos.term();
            pos.advance();
        });

    // close the wave's sums; the lane that holds value (i, q, w) doubles it and stores it, its mirror and its zeros
    const int idx = pair_close<NV>(acc, lane);
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
static int pa_launch(int form, const PairTriArgs& g, unsigned grid, hipStream_t s) {
    return with_width(form + 1, [&](auto WW) {
        constexpr int F = decltype(WW)::value - 1;
        return with_group(g.ng, [&](auto G) {
            static PerDeviceLds once;
            return pair_launch(pair_contract_antisym_kernel<F, G>, g, pa_lds_bytes(F, G), once, grid, s,
                               "hipFuncSetAttribute(pair_contract_antisym)", "pair contract antisym launch",
                               "qs::pair_contract_antisym_kernel<%d, %d>", F, (int)G);
        });
    });
}

}  // namespace qs

using namespace qs;

extern "C" {

int64_t qs_pair_contract_antisym_workspace(int u_dtype, int t_dtype, int64_t l, int64_t K) {
    return pair_tri_workspace<false>(u_dtype, t_dtype, l, K);
}

int qs_pair_contract_antisym(int u_dtype, int t_dtype, const void* U, const void* T, void* S, int64_t l, int64_t K,
                             int64_t ldu, void* work, int64_t work_elems, void* stream) {
    (void)work;
    return pair_tri_entry<false>(4 * kPaRows, kPaGroup, pa_launch, u_dtype, t_dtype, U, T, S, l, K, ldu, work_elems, stream);
}

}  // extern "C"
