// Contraction of a row-major matrix with a few vectors over its TRAILING index, one read of the matrix per group:
//   S[k, x] = sum_y U[x * ldu + y] * T[k * Y + y],   k = 0 ... K-1   (no conjugation)
// With U = u viewed as (l^2, l^2) this is S[k,p,q] = sum_rs u[p,q,r,s] T[k,r,s]: the u-dependent part of the sigma
// vector of a two-particle full CI, and the particle-particle ladder of coupled-cluster doubles on the AO tensor.
// 2 K flop per element of U: a row-dot-product stream, HBM-bound like qs_mean_field.hip, with the cross-lane reduction
// at the end of a row.
//
// A workgroup of 256 threads takes kPcRows * 4 consecutive rows, wave w the kPcRows rows from row 4 w of them.  The 64
// lanes of a wave cover 64 consecutive 16-byte items (1 KB) of ONE row per load; a lane keeps kPcRows x G running sums
// in registers and walks along y in steps of 64 items, the next step's items issued before the current step's fmas.
// Raw buffer loads whose range ends with the last addressed element of U: an item past a row's end is never fetched
// (its lane offset is out of range), 16-byte items start at the row's first element whatever its alignment (odd Y or
// ldu, an 8-byte-aligned base), and the second half of the item that straddles an odd row's end is dropped by a select.
// The four waves share the T values of a chunk of up to kPcSteps steps, staged in LDS as [item][y in item][g]: the G values
// one product needs are adjacent (records padded to an odd number of 16-byte units, so that a wave's 128-bit reads
// spread over the banks); two buffers, chunk c + 1 is staged while chunk c is consumed.
// After the last step a wave closes its kPcRows * G row sums once with ONE xor butterfly over masks 32, 16, ... 1 in
// which every stage also halves the number of values a lane carries (the lane pair splits them: pair_close of
// qs_pair_walk.h, shared with the two triangle kernels like the launch), so that each lane ends
// with one finished sum and stores it: plain vector stores, no floating-point atomics, no workspace, no closing launch.
//
// Reproducible: every product is an explicit fma in a fixed order, a row's items are dealt to the lanes by Y alone, and
// every sum goes through the same butterfly stages whatever G.  The geometry depends on (Y, dtypes) only -- here on
// nothing at all -- so row x has the same bits whatever X, ldu, K, the position of k in the batch or the instantiation
// its group runs on (a partial last group takes the smallest instantiation that holds it).

#include "qs_pair_walk.h"

namespace qs {

constexpr int kPcRows = 4;             // rows per wave (TA); a workgroup takes 4 * kPcRows rows
constexpr int kPcSteps = 3;            // most steps of 64 items per staged chunk of T (two buffers of it within 64 KB of LDS)
constexpr int kPcMaxG = 8;
constexpr unsigned kPcRoomMax = 0x80000000u;      // buffer ranges are cut to 2 GB: every lane offset stays below it
// Shipped group size per form {fp64, complex128, mixed}: the largest G of the form that keeps two workgroups per CU in
// VGPRs and in LDS (DESIGN.md 3.6 has the code-object figures).
constexpr int kPcGroup[3] = {8, 8, 4};

struct PcArgs {
    const double* U;
    const double* T;          // first vector of the group, [ng][Y]
    double* S;                // first result row of the group, [ng][X]
    int64_t X, Y, ldu;
    int ng;                   // vectors of this launch, 1 ... G of the instantiation
};

// 16-byte units of one item's record in LDS: CPI * G * AW doubles, padded to an odd number of units
static constexpr int pc_record_units(int form, int G) {
    const int words = form_widths(form).cpi * G * form_widths(form).aw;
    return (words / 2) | 1;
}

// Steps per chunk: kPcSteps, fewer where two buffers of that would pass 64 KB (the 8-vector instantiation of the mixed form)
static constexpr int pc_steps(int form, int G) {
    int n = kPcSteps;
    while (n > 1 && 2 * n * 64 * pc_record_units(form, G) * 16 > 65536) --n;
    return n;
}

static constexpr size_t pc_lds_bytes(int form, int G) {
    return (size_t)2 * pc_steps(form, G) * 64 * pc_record_units(form, G) * 16;
}

// FORM 0: U, T, S real; 1: all complex128; 2: real U, complex T and S.  G: vectors per load of U.
template <int FORM, int G>
__global__ __launch_bounds__(256) void pair_contract_kernel(const PcArgs g) {
    constexpr auto W = form_widths(FORM);
    constexpr int UW = W.uw, AW = W.aw, CPI = W.cpi;
    constexpr int TA = kPcRows;
    constexpr int RW = pc_record_units(FORM, G) * 2;       // doubles of one item's record
    constexpr int NS = pc_steps(FORM, G);                  // steps per staged chunk
    constexpr int CW = NS * 64 * RW;                       // doubles of one buffer
    constexpr int NV = TA * G * AW;
    extern __shared__ __attribute__((aligned(16))) double pc_lds[];

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t Y = g.Y, X = g.X;
    const int64_t nitems = (Y + CPI - 1) / CPI;
    const int nsteps = (int)((nitems + 63) >> 6), nchunks = (nsteps + NS - 1) / NS;
    const int64_t row0 = ((int64_t)blockIdx.x * 4 + wave) * TA;

    // the wave's window of U: from its first row to the last addressed element of the matrix
    const uint64_t row_bytes = (uint64_t)g.ldu * (UW * 8);
    const uint64_t end = reinterpret_cast<uint64_t>(g.U) + ((uint64_t)(X - 1) * (uint64_t)g.ldu + (uint64_t)Y) * (UW * 8);
    const uint64_t base0 = uniform64(reinterpret_cast<uint64_t>(g.U) + (uint64_t)row0 * row_bytes);
    unsigned off[TA];
    bool rowok[TA];
#pragma unroll
    for (int i = 0; i < TA; ++i) {
        rowok[i] = row0 + i < X;
        off[i] = (unsigned)(i * row_bytes) + (unsigned)lane * 16u;
    }

    // T values of chunk c -> buffer c & 1: zero beyond Y and beyond the launch's vectors
    auto stage = [&](int c) {
        double* buf = pc_lds + (c & 1) * CW;
        const int64_t y0 = (int64_t)c * (NS * 64 * CPI);
        for (int idx = tid; idx < NS * 64 * CPI * G; idx += 256) {
            const int yy = idx % (NS * 64 * CPI), gg = idx / (NS * 64 * CPI);
            const bool ok = y0 + yy < Y && gg < g.ng;
            const double* src = g.T + (ok ? ((int64_t)gg * Y + y0 + yy) * AW : 0);
            double* dst = buf + (yy / CPI) * RW + ((yy % CPI) * G + gg) * AW;
#pragma unroll
            for (int w = 0; w < AW; ++w) dst[w] = ok ? src[w] : 0.0;
        }
    };

    double acc[NV];
#pragma unroll
    for (int j = 0; j < NV; ++j) acc[j] = 0.0;

    // items of step st: lane offsets, or the out-of-range offset for an item past the row's end / a row past X
    auto fetch = [&](int st, f64x2 (&dst)[TA]) {
        const uint64_t base = base0 + (uint64_t)st * 1024u;
        const uint64_t left = end > base ? end - base : 0;
        const unsigned room = left > kPcRoomMax ? kPcRoomMax : (unsigned)left;
        const bool inrow = ((int64_t)st * 64 + lane) < nitems;
#pragma unroll
        for (int i = 0; i < TA; ++i) dst[i] = FastItem<true>::load(base, room, (inrow && rowok[i]) ? off[i] : kPcRoomMax);
    };

    f64x2 cur[TA], nxt[TA];
    fetch(0, cur);
#pragma unroll
    for (int i = 0; i < TA; ++i) nxt[i] = cur[i];
    stage(0);
    __syncthreads();

    // the chunk loop of pair_chunk_walk (qs_pair_walk.h), kept in place: through the template this kernel's shipped
    // instantiations ran 1-5 % slower on the same registers (profiles/pair_walk_ab.txt)
    for (int c = 0; c < nchunks; ++c) {
        if (c + 1 < nchunks) stage(c + 1);
        const double* buf = pc_lds + (c & 1) * CW;
        const int s_hi = nsteps - c * NS < NS ? nsteps - c * NS : NS;
        for (int ss = 0; ss < s_hi; ++ss) {
            const int st = c * NS + ss;
            if (st + 1 < nsteps) fetch(st + 1, nxt);
            const double* rec = buf + (ss * 64 + lane) * RW;
            double t[CPI][G][AW];
#pragma unroll
            for (int k = 0; k < CPI; ++k)
#pragma unroll
                for (int q = 0; q < G; ++q)
#pragma unroll
                    for (int w = 0; w < AW; ++w) t[k][q][w] = rec[(k * G + q) * AW + w];
            // odd Y: the second half of the row's last item belongs to the next row
            const bool full = FORM == 1 || ((int64_t)st * 64 + lane) * CPI + 1 < Y;
#pragma unroll
            for (int i = 0; i < TA; ++i) {
                f64x2 v = cur[i];
                if (!full) v.y = 0.0;
#pragma unroll
                for (int q = 0; q < G; ++q) {
                    double* a = acc + (i * G + q) * AW;
                    if (FORM == 0) {
                        a[0] = fma(v.y, t[CPI - 1][q][0], fma(v.x, t[0][q][0], a[0]));
                    } else if (FORM == 2) {
#pragma unroll
                        for (int w = 0; w < AW; ++w) a[w] = fma(v.y, t[CPI - 1][q][w], fma(v.x, t[0][q][w], a[w]));
                    } else {
                        a[0] = fma(-v.y, t[0][q][AW - 1], fma(v.x, t[0][q][0], a[0]));
                        a[AW - 1] = fma(v.y, t[0][q][0], fma(v.x, t[0][q][AW - 1], a[AW - 1]));
                    }
                }
            }
#pragma unroll
            for (int i = 0; i < TA; ++i) cur[i] = nxt[i];
        }
        __syncthreads();
    }

    // close the wave's row sums; the lane that holds value (i, q, w) stores it
    const int idx = pair_close<NV>(acc, lane);
    const int w = idx % AW, q = (idx / AW) % G, i = idx / (AW * G);
    const bool first = NV >= 64 || (lane & (64 / NV - 1)) == 0;       // the lanes below a halving-stage bit hold copies
    if (first && q < g.ng && row0 + i < X) g.S[((int64_t)q * X + row0 + i) * AW + w] = acc[0];
}

// One group of g.ng vectors on the smallest instantiation that holds it.
static int pc_launch(int form, const PcArgs& g, unsigned grid, hipStream_t s) {
    return with_form(form, [&](auto F) {
        return with_group(g.ng, [&](auto G) {
            static PerDeviceLds once;
            return pair_launch(pair_contract_kernel<F, G>, g, pc_lds_bytes(F, G), once, grid, s,
                               "hipFuncSetAttribute(pair_contract)", "pair contract launch",
                               "qs::pair_contract_kernel<%d, %d>", (int)F, (int)G);
        });
    });
}

// ldu <= 2^24 elements keeps the lane offsets of a wave's rows below the 2 GB buffer range
static inline bool pc_extents_ok(int64_t X, int64_t Y, int64_t K) {
    return X > 0 && X <= (int64_t(1) << 32) && Y > 0 && Y <= (int64_t(1) << 24) && K > 0 && K <= 65536;
}

// The form's group size: the shipped one, or the tuning run's (pair_contract_g = 1, 2, 4, 8).
static inline int pc_group(int form) { return group_size(g_tune.pair_contract_g, kPcGroup[form]); }

}  // namespace qs

using namespace qs;

extern "C" {

int64_t qs_pair_contract_workspace(int u_dtype, int t_dtype, int64_t X, int64_t Y, int64_t K) {
    const int form = tensor_form(u_dtype, t_dtype);
    if (form < 0) return form;
    if (!pc_extents_ok(X, Y, K)) return QS_ERR_BAD_EXTENT;
    return 0;          // y is never split: every row sum is closed inside its wave
}

int qs_pair_contract(int u_dtype, int t_dtype, const void* U, const void* T, void* S, int64_t X, int64_t Y, int64_t K,
                     int64_t ldu, void* work, int64_t work_elems, void* stream) {
    dispatch_reset();
    (void)work;
    const int form = tensor_form(u_dtype, t_dtype);
    if (form < 0) return form;
    if (!pc_extents_ok(X, Y, K) || ldu < Y || ldu > (int64_t(1) << 24)) return QS_ERR_BAD_EXTENT;
    if (!U || !T || !S) return QS_ERR_NULL_POINTER;
    const int64_t es = (int64_t)elem_size(t_dtype), ues = (int64_t)elem_size(u_dtype);
    if (!aligned(U, (size_t)ues) || !aligned(T, (size_t)es) || !aligned(S, (size_t)es)) return QS_ERR_MISALIGNED;
    const int64_t s_bytes = K * X * es;
    if (overlaps(S, s_bytes, U, ((X - 1) * ldu + Y) * ues) || overlaps(S, s_bytes, T, K * Y * es)) return QS_ERR_ALIAS;
    if (work_elems < qs_pair_contract_workspace(u_dtype, t_dtype, X, Y, K)) return QS_ERR_WORKSPACE;

    const int aw = form_widths(form).aw;
    PcArgs g{};
    g.U = (const double*)U;
    g.X = X; g.Y = Y; g.ldu = ldu;
    const unsigned grid = (unsigned)cdiv(X, 4 * kPcRows);
    hipStream_t s = (hipStream_t)stream;
    return for_each_group(K, pc_group(form), [&](int64_t k0, int ng) {
        g.ng = ng;
        g.T = (const double*)T + k0 * Y * aw;
        g.S = (double*)S + k0 * X * aw;
        return pc_launch(form, g, grid, s);
    });
}

}  // extern "C"
