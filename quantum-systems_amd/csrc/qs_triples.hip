// Closed-shell perturbative triples: the six-fold permuted combine, divide and reduce, one read of the blocks.
//
// A triple (i, j, k) of occupied orbitals owns six blocks X_0 ... X_5 = X_ijk, X_ikj, X_jik, X_jki, X_kij, X_kji, each
// (v, v, v) row-major (a product of the amplitudes with the integrals; the host forms them).  With
//   W[a,b,c] = X_0[a,b,c] + X_1[a,c,b] + X_2[b,a,c] + X_3[b,c,a] + X_4[c,a,b] + X_5[c,b,a]
//   Z[a,b,c] = (4 W[abc] + W[bca] + W[cab] - 2 W[acb] - 2 W[cba] - 2 W[bac]) / 3
//   e        = sum_abc Re(conj(W[abc]) Z[abc]) / (eo3 - ev[a] - ev[b] - ev[c])
// neither W nor Z is ever stored.  The six W of the orbit of one (a, b, c) are sums of the SAME 36 elements (every block
// at every order of the three indices), the denominator is the same on the whole orbit, and Z on the orbit is a
// combination of those six W alone: with S_e = W[abc] + W[bca] + W[cab], S_o = W[acb] + W[cba] + W[bac],
//   sum_orbit Re(conj(W) Z) = sum_orbit |W|^2 + (|S_e|^2 + |S_o|^2 - 4 Re(conj(S_e) S_o)) / 3
// (Z[pi] = W[pi] + (S_same - 2 S_other) / 3).  So one thread takes one a <= b <= c, reads its 36 elements once and adds the
// whole orbit; an orbit with two equal indices is counted twice by the six orders and one with three six times: the
// weights 1/2 and 1/6.
//
// Work unit: (triple, tile set ta <= tb <= tc) with tiles of edge T along a, b, c.  The workgroup loads the tiles of the
// six blocks at the six orders of (ta, tb, tc) into LDS -- 36 tiles of T^3 elements, fewer where two tile indices or two
// block indices of the triple coincide: an order (a block) that repeats an earlier one is not loaded again, its reads go to
// the earlier copy -- so that every element of the blocks comes from memory once, in runs of T contiguous elements, and
// the permuted reads are LDS reads.  T = 8 for fp64 (36 tiles of 8 x 69 elements, the leading stride padded from 64 so that
// the permuted reads of a wave spread over the banks: 158976 bytes) and 6 for complex128 (36 x 216 x 16 = 124416 bytes)
// against the 160 KiB of a CU: one workgroup per CU, 512 / 256 threads.
//
// No atomics: a workgroup's threads are added up in a fixed order (wave shuffles, then the waves in order) into ONE
// partial per (triple, tile set); triples_close_kernel adds the partials of a triple in a fixed order that depends on the
// number of tile sets alone.  The bits of e[x] depend on the triple's own blocks, eo3[x], ev and v, on nothing else: not on
// the batch, not on the run.
//
// The singles term of (T) (triples_energy_singles_kernel): a second permuted family V' built like W from blocks that are
// outer products, Y_beta[p,q,r] = A[sa][p] G[sg][q,r], and never stored: the thread of an orbit reads its 18 elements of A
// and 36 of G from memory (small, L2-resident; LDS is full), forms the six V' beside the six W and adds
//   sum_orbit Re(conj(V') Z) = sum_orbit Re(conj(V') W) + Re(conj(S'_e) (S_e - 2 S_o) + conj(S'_o) (S_o - 2 S_e)) / 3
// into a second partial of the work unit.  Everything else -- work units, load, LDS image, reduction, close -- is shared,
// and the connected part e[x] is the one of triples_energy_kernel, operation for operation.

#include <cmath>

#include "qs_common.h"

namespace qs {

// the six orders of three things, as positions into (a, b, c): abc, acb, bac, bca, cab, cba.  Block X_beta enters W[p,q,r]
// at order beta of (p, q, r); orders 0, 3, 4 are the even ones.
__host__ __device__ constexpr int order_at(int s, int pos) {
    constexpr int kOrders[6][3] = {{0, 1, 2}, {0, 2, 1}, {1, 0, 2}, {1, 2, 0}, {2, 0, 1}, {2, 1, 0}};
    return kOrders[s][pos];
}

// the order "first pi, then rho" of (a, b, c): position x of it is pi[rho[x]]
__host__ __device__ constexpr int order_of_orders(int pi, int rho) {
    for (int s = 0; s < 6; ++s)
        if (order_at(s, 0) == order_at(pi, order_at(rho, 0)) && order_at(s, 1) == order_at(pi, order_at(rho, 1)) &&
            order_at(s, 2) == order_at(pi, order_at(rho, 2)))
            return s;
    return -1;
}

template <int W>
struct TriplesGeo {
    static constexpr int T = W == 1 ? 8 : 6;                 // tile edge
    static constexpr int S1 = T;                             // element strides of a tile in LDS: (S2, S1, 1)
    static constexpr int S2 = W == 1 ? 69 : 36;
    static constexpr int tile = T * S2;                      // elements of one tile's LDS image
    static constexpr int cube = T * T * T;
    static constexpr int threads = (cube + 63) / 64 * 64;    // one thread per element of a tile
    static constexpr size_t lds_bytes = (size_t)36 * tile * W * sizeof(double);
};
static_assert(TriplesGeo<1>::lds_bytes + 1024 <= 160 * 1024 && TriplesGeo<2>::lds_bytes + 1024 <= 160 * 1024, "LDS of one CU");

struct TriplesArgs {
    const double* X;
    const int32_t* slots;   // (n, 6)
    const double* eo3;      // n
    const double* ev;       // v
    double* part;           // (n, nsets)
    double* e;              // n
    int64_t v, nblocks;
    int nt;                 // tiles along one index
    unsigned nsets;         // nt (nt + 1) (nt + 2) / 6
};

struct TriplesSingles {
    const double* A;        // (na, v)
    const double* G;        // (ng, v, v)
    const int32_t* sslots;  // (n, 6, 2): (sa, sg) of the six blocks
    double* part;           // (n, nsets): the singles partials
    int64_t na, ng;
};

// first entry of key[0 ... 5] equal to key[s]
__device__ inline int first_equal(const int64_t (&key)[6], int s) {
    int f = s;
#pragma unroll
    for (int x = 5; x >= 0; --x)
        if (x < s && key[x] == key[s]) f = x;
    return f;
}

// one work unit; SINGLES adds the singles partial (q is not looked at without it)
template <int W, bool SINGLES>
__device__ __forceinline__ void triples_unit(const TriplesArgs& g, const TriplesSingles& q) {
    using G = TriplesGeo<W>;
    constexpr int T = G::T;
    extern __shared__ __align__(16) double tiles[];
    __shared__ double s_wave[SINGLES ? 2 : 1][G::threads / 64];
    const int tid = threadIdx.x;
    const unsigned triple = blockIdx.x / g.nsets;
    unsigned rest = blockIdx.x - triple * g.nsets;
    // the tile set: sets in the order of tc, then tb, then ta
    int t[3] = {0, 0, 0};
    while (rest >= (unsigned)((t[2] + 1) * (t[2] + 2) / 2)) { rest -= (unsigned)((t[2] + 1) * (t[2] + 2) / 2); ++t[2]; }
    while (rest >= (unsigned)(t[1] + 1)) { rest -= (unsigned)(t[1] + 1); ++t[1]; }
    t[0] = (int)rest;

    // which of the 36 tiles are their own: an order of the tile set / a block that repeats an earlier one reads that one's copy
    int64_t okey[6], bkey[6];
    bool bad = false;
#pragma unroll
    for (int s = 0; s < 6; ++s) {
        okey[s] = ((int64_t)t[order_at(s, 0)] * g.nt + t[order_at(s, 1)]) * g.nt + t[order_at(s, 2)];
        bkey[s] = g.slots[(int64_t)triple * 6 + s];
        bad = bad || bkey[s] < 0 || bkey[s] >= g.nblocks;
    }
    int64_t akey[6], gkey[6];
    if constexpr (SINGLES) {
#pragma unroll
        for (int s = 0; s < 6; ++s) {
            akey[s] = q.sslots[((int64_t)triple * 6 + s) * 2];
            gkey[s] = q.sslots[((int64_t)triple * 6 + s) * 2 + 1];
            bad = bad || akey[s] < 0 || akey[s] >= q.na || gkey[s] < 0 || gkey[s] >= q.ng;
        }
    }
    if (bad) {          // a block index outside X (A, G): nothing is read, the triple's energy is a NaN
        if (tid == 0) {
            g.part[blockIdx.x] = NAN;
            if constexpr (SINGLES) q.part[blockIdx.x] = NAN;
        }
        return;
    }
    int omap[6], bmap[6];
#pragma unroll
    for (int s = 0; s < 6; ++s) {
        omap[s] = first_equal(okey, s);
        bmap[s] = first_equal(bkey, s);
    }

    // -- the load: thread (p, q, r) of a tile, r along the contiguous index; all loads of a thread in flight together
    const int lp = tid / (T * T), lq = tid / T % T, lr = tid % T;
    const bool in_cube = tid < G::cube;
    const int64_t v = g.v;
    double val[36][W];
#pragma unroll
    for (int b = 0; b < 6; ++b) {
#pragma unroll
        for (int s = 0; s < 6; ++s) {
#pragma unroll
            for (int w = 0; w < W; ++w) val[b * 6 + s][w] = 0.0;
            if (bmap[b] != b || omap[s] != s) continue;
            const int64_t gp = (int64_t)t[order_at(s, 0)] * T + lp, gq = (int64_t)t[order_at(s, 1)] * T + lq,
                          gr = (int64_t)t[order_at(s, 2)] * T + lr;
            if (in_cube && gp < v && gq < v && gr < v) {
                const double* src = g.X + ((((int64_t)bkey[b] * v + gp) * v + gq) * v + gr) * W;
#pragma unroll
                for (int w = 0; w < W; ++w) val[b * 6 + s][w] = src[w];
            }
        }
    }
#pragma unroll
    for (int b = 0; b < 6; ++b) {
#pragma unroll
        for (int s = 0; s < 6; ++s) {
            if (bmap[b] != b || omap[s] != s || !in_cube) continue;
            double* dst = tiles + ((int64_t)(b * 6 + s) * G::tile + lp * G::S2 + lq * G::S1 + lr) * W;
#pragma unroll
            for (int w = 0; w < W; ++w) dst[w] = val[b * 6 + s][w];
        }
    }
    __syncthreads();

    // -- the orbit of (a, b, c) = tile set + (lp, lq, lr), a <= b <= c < v
    const int l[3] = {lp, lq, lr};
    const int64_t a = (int64_t)t[0] * T + lp, b = (int64_t)t[1] * T + lq, c = (int64_t)t[2] * T + lr;
    double mine = 0.0, mine_s = 0.0;
    if (in_cube && a <= b && b <= c && c < v) {
        int off[6];         // where (a, b, c) at order s sits in a tile of order s
#pragma unroll
        for (int s = 0; s < 6; ++s) off[s] = l[order_at(s, 0)] * G::S2 + l[order_at(s, 1)] * G::S1 + l[order_at(s, 2)];
        double Wv[6][W];
#pragma unroll
        for (int pi = 0; pi < 6; ++pi) {
#pragma unroll
            for (int w = 0; w < W; ++w) Wv[pi][w] = 0.0;
#pragma unroll
            for (int beta = 0; beta < 6; ++beta) {
                const int s = order_of_orders(pi, beta);      // (a constant once the loops are unrolled)
                const double* src = tiles + ((int64_t)(bmap[beta] * 6 + omap[s]) * G::tile + off[s]) * W;
#pragma unroll
                for (int w = 0; w < W; ++w) Wv[pi][w] += src[w];
            }
        }
        double sq = 0.0, Se[W], So[W];
#pragma unroll
        for (int w = 0; w < W; ++w) {
            Se[w] = (Wv[0][w] + Wv[3][w]) + Wv[4][w];
            So[w] = (Wv[1][w] + Wv[2][w]) + Wv[5][w];
#pragma unroll
            for (int pi = 0; pi < 6; ++pi) sq = __builtin_fma(Wv[pi][w], Wv[pi][w], sq);
        }
        double cross = 0.0;
#pragma unroll
        for (int w = 0; w < W; ++w) cross += (Se[w] * Se[w] + So[w] * So[w]) - 4.0 * (Se[w] * So[w]);
        const double D = ((g.eo3[triple] - g.ev[a]) - g.ev[b]) - g.ev[c];
        const double weight = (a == b && b == c) ? 1.0 / 6.0 : (a == b || b == c) ? 0.5 : 1.0;
        mine = weight * (sq + cross / 3.0) / D;
        if constexpr (SINGLES) {
            // V'[pi] = sum_beta Y_beta at order s of (a, b, c): A at the first index of the order, G at the other two
            const int64_t abc[3] = {a, b, c};
            double Vv[6][W];
#pragma unroll
            for (int pi = 0; pi < 6; ++pi) {
#pragma unroll
                for (int w = 0; w < W; ++w) Vv[pi][w] = 0.0;
            }
#pragma unroll
            for (int beta = 0; beta < 6; ++beta) {
                const double* Ab = q.A + akey[beta] * v * W;
                const double* Gb = q.G + gkey[beta] * v * v * W;
                double Av[3][W];
#pragma unroll
                for (int x = 0; x < 3; ++x) {
#pragma unroll
                    for (int w = 0; w < W; ++w) Av[x][w] = Ab[abc[x] * W + w];
                }
#pragma unroll
                for (int pi = 0; pi < 6; ++pi) {
                    const int s = order_of_orders(pi, beta);
                    const double* gs = Gb + (abc[order_at(s, 1)] * v + abc[order_at(s, 2)]) * W;
                    const double* as = Av[order_at(s, 0)];
                    if constexpr (W == 1) {
                        Vv[pi][0] += as[0] * gs[0];
                    } else {
                        Vv[pi][0] += as[0] * gs[0] - as[1] * gs[1];
                        Vv[pi][1] += as[0] * gs[1] + as[1] * gs[0];
                    }
                }
            }
            double dot = 0.0, mixed = 0.0;
#pragma unroll
            for (int w = 0; w < W; ++w) {
                const double Te = (Vv[0][w] + Vv[3][w]) + Vv[4][w], To = (Vv[1][w] + Vv[2][w]) + Vv[5][w];
#pragma unroll
                for (int pi = 0; pi < 6; ++pi) dot = __builtin_fma(Vv[pi][w], Wv[pi][w], dot);
                mixed += Te * (Se[w] - 2.0 * So[w]) + To * (So[w] - 2.0 * Se[w]);
            }
            mine_s = weight * (dot + mixed / 3.0) / D;
        }
    }

    // -- the workgroup's partial: lanes by shuffles, waves in order
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) mine += __shfl_down(mine, d, 64);
    if constexpr (SINGLES) {
#pragma unroll
        for (int d = 32; d > 0; d >>= 1) mine_s += __shfl_down(mine_s, d, 64);
    }
    if ((tid & 63) == 0) {
        s_wave[0][tid >> 6] = mine;
        if constexpr (SINGLES) s_wave[1][tid >> 6] = mine_s;
    }
    __syncthreads();
    if (tid == 0) {
        double sum = s_wave[0][0];
#pragma unroll
        for (int x = 1; x < G::threads / 64; ++x) sum += s_wave[0][x];
        g.part[blockIdx.x] = sum;
        if constexpr (SINGLES) {
            double sum_s = s_wave[1][0];
#pragma unroll
            for (int x = 1; x < G::threads / 64; ++x) sum_s += s_wave[1][x];
            q.part[blockIdx.x] = sum_s;
        }
    }
}

template <int W>
__global__ __launch_bounds__(TriplesGeo<W>::threads) void triples_energy_kernel(const TriplesArgs g) {
    triples_unit<W, false>(g, TriplesSingles{});
}

template <int W>
__global__ __launch_bounds__(TriplesGeo<W>::threads) void triples_energy_singles_kernel(const TriplesArgs g, const TriplesSingles q) {
    triples_unit<W, true>(g, q);
}

// e[x] = the partials of triple x: thread-strided sums, then a tree, both in a fixed order
__global__ __launch_bounds__(256) void triples_close_kernel(const TriplesArgs g) {
    __shared__ double s_sum[256];
    const int tid = threadIdx.x;
    const double* part = g.part + (int64_t)blockIdx.x * g.nsets;
    double sum = 0.0;
    for (unsigned x = tid; x < g.nsets; x += 256) sum += part[x];
    s_sum[tid] = sum;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if (tid < w) s_sum[tid] += s_sum[tid + w];
        __syncthreads();
    }
    if (tid == 0) g.e[blockIdx.x] = s_sum[0];
}

static inline int64_t triples_tile(int dtype) { return dtype == QS_C128 ? TriplesGeo<2>::T : TriplesGeo<1>::T; }

// tile sets of one triple; 0 where the extents do not fit (v <= 4096: at most 683 tiles, 53 million sets)
static inline int64_t triples_sets(int dtype, int64_t v, int64_t n) {
    if (v < 1 || v > 4096 || n < 1) return 0;
    const int64_t nt = cdiv(v, triples_tile(dtype)), nsets = nt * (nt + 1) * (nt + 2) / 6;
    return n <= ((int64_t(1) << 31) - 1) / nsets ? nsets : 0;        // one workgroup per (triple, set)
}

template <int W>
static int launch_triples(const TriplesArgs& g, int64_t n, hipStream_t stream) {
    using G = TriplesGeo<W>;
    auto kern = triples_energy_kernel<W>;
    static PerDeviceLds lds_opt_in;
    if (int rc = opt_in_dynamic_lds((const void*)kern, G::lds_bytes, lds_opt_in, "hipFuncSetAttribute(triples_energy)")) return rc;
    hipLaunchKernelGGL(kern, dim3((unsigned)(n * g.nsets)), dim3(G::threads), G::lds_bytes, stream, g);
    note_dispatch("qs::triples_energy_kernel<%d>", W);
    return launch_status("triples_energy launch");
}

template <int W>
static int launch_triples_singles(const TriplesArgs& g, const TriplesSingles& q, int64_t n, hipStream_t stream) {
    using G = TriplesGeo<W>;
    auto kern = triples_energy_singles_kernel<W>;
    static PerDeviceLds lds_opt_in;
    if (int rc = opt_in_dynamic_lds((const void*)kern, G::lds_bytes, lds_opt_in, "hipFuncSetAttribute(triples_energy_singles)")) return rc;
    hipLaunchKernelGGL(kern, dim3((unsigned)(n * g.nsets)), dim3(G::threads), G::lds_bytes, stream, g, q);
    note_dispatch("qs::triples_energy_singles_kernel<%d>", W);
    return launch_status("triples_energy_singles launch");
}

}  // namespace qs

using namespace qs;

extern "C" {

int64_t qs_triples_energy_tile(int dtype) {
    if (!dtype_ok(dtype)) return QS_ERR_BAD_DTYPE;
    return triples_tile(dtype);
}

int64_t qs_triples_energy_budget(int64_t budget_bytes) {
    if (budget_bytes < 0) return QS_ERR_BAD_EXTENT;
    return g_tune.triples_bytes > 0 ? g_tune.triples_bytes : budget_bytes;
}

int64_t qs_triples_energy_workspace(int dtype, int64_t v, int64_t n) {
    if (!dtype_ok(dtype)) return QS_ERR_BAD_DTYPE;
    const int64_t nsets = triples_sets(dtype, v, n);
    if (!nsets) return QS_ERR_BAD_EXTENT;
    return n * nsets * (int64_t)sizeof(double);
}

int qs_triples_energy(int dtype, const void* X, int64_t nblocks, const int32_t* slots, const double* eo3, const double* ev,
                      int64_t v, int64_t n, double* e, void* work, int64_t work_bytes, void* stream) {
    dispatch_reset();
    if (!dtype_ok(dtype)) return QS_ERR_BAD_DTYPE;
    const int64_t nsets = triples_sets(dtype, v, n);
    const int64_t es = (int64_t)elem_size(dtype);
    if (!nsets || nblocks < 1 || nblocks > INT32_MAX || nblocks > INT64_MAX / (v * v * v * es)) return QS_ERR_BAD_EXTENT;
    if (!X || !slots || !eo3 || !ev || !e || !work) return QS_ERR_NULL_POINTER;
    if (!aligned(X, (size_t)es) || !aligned(slots, 4) || !aligned(eo3, 8) || !aligned(ev, 8) || !aligned(e, 8) || !aligned(work, 8))
        return QS_ERR_MISALIGNED;
    const int64_t need = n * nsets * (int64_t)sizeof(double);
    if (work_bytes < need) return QS_ERR_WORKSPACE;
    const int64_t xbytes = nblocks * v * v * v * es;
    if (overlaps(e, n * 8, X, xbytes) || overlaps(work, need, X, xbytes) || overlaps(e, n * 8, work, need) ||
        overlaps(e, n * 8, slots, n * 24) || overlaps(e, n * 8, eo3, n * 8) || overlaps(e, n * 8, ev, v * 8))
        return QS_ERR_ALIAS;

    hipStream_t s = (hipStream_t)stream;
    const TriplesArgs g{(const double*)X, slots, eo3, ev, (double*)work, e, v, nblocks, (int)cdiv(v, triples_tile(dtype)),
                        (unsigned)nsets};
    if (int rc = dtype == QS_C128 ? launch_triples<2>(g, n, s) : launch_triples<1>(g, n, s)) return rc;
    hipLaunchKernelGGL(triples_close_kernel, dim3((unsigned)n), dim3(256), 0, s, g);
    note_dispatch("qs::triples_close_kernel");
    return launch_status("triples_close launch");
}

int64_t qs_triples_energy_singles_workspace(int dtype, int64_t v, int64_t n) {
    if (!dtype_ok(dtype)) return QS_ERR_BAD_DTYPE;
    const int64_t nsets = triples_sets(dtype, v, n);
    if (!nsets) return QS_ERR_BAD_EXTENT;
    return 2 * n * nsets * (int64_t)sizeof(double);     // the connected and the singles partial of every (triple, tile set)
}

int qs_triples_energy_singles(int dtype, const void* X, int64_t nblocks, const int32_t* slots, const double* eo3,
                              const double* ev, const void* A, int64_t na, const void* G, int64_t ng, const int32_t* sslots,
                              int64_t v, int64_t n, double* e, double* es_out, void* work, int64_t work_bytes, void* stream) {
    dispatch_reset();
    if (!dtype_ok(dtype)) return QS_ERR_BAD_DTYPE;
    const int64_t nsets = triples_sets(dtype, v, n);
    const int64_t es = (int64_t)elem_size(dtype);
    if (!nsets || nblocks < 1 || nblocks > INT32_MAX || nblocks > INT64_MAX / (v * v * v * es)) return QS_ERR_BAD_EXTENT;
    if (na < 1 || na > INT32_MAX || ng < 1 || ng > INT32_MAX) return QS_ERR_BAD_EXTENT;     // (v <= 4096: no product overflows)
    if (!X || !slots || !eo3 || !ev || !A || !G || !sslots || !e || !es_out || !work) return QS_ERR_NULL_POINTER;
    if (!aligned(X, (size_t)es) || !aligned(slots, 4) || !aligned(eo3, 8) || !aligned(ev, 8) || !aligned(A, (size_t)es) ||
        !aligned(G, (size_t)es) || !aligned(sslots, 4) || !aligned(e, 8) || !aligned(es_out, 8) || !aligned(work, 8))
        return QS_ERR_MISALIGNED;
    const int64_t half = n * nsets * (int64_t)sizeof(double), need = 2 * half;
    if (work_bytes < need) return QS_ERR_WORKSPACE;
    const int64_t xbytes = nblocks * v * v * v * es, abytes = na * v * es, gbytes = ng * v * v * es;
    const struct { const void* p; int64_t bytes; } inputs[] = {{X, xbytes},   {slots, n * 24}, {eo3, n * 8},     {ev, v * 8},
                                                               {A, abytes}, {G, gbytes},     {sslots, n * 48}};
    for (const auto& in : inputs)
        if (overlaps(e, n * 8, in.p, in.bytes) || overlaps(es_out, n * 8, in.p, in.bytes) || overlaps(work, need, in.p, in.bytes))
            return QS_ERR_ALIAS;
    if (overlaps(e, n * 8, work, need) || overlaps(es_out, n * 8, work, need) || overlaps(e, n * 8, es_out, n * 8)) return QS_ERR_ALIAS;

    hipStream_t s = (hipStream_t)stream;
    TriplesArgs g{(const double*)X, slots, eo3, ev, (double*)work, e, v, nblocks, (int)cdiv(v, triples_tile(dtype)),
                  (unsigned)nsets};
    const TriplesSingles q{(const double*)A, (const double*)G, sslots, (double*)work + n * nsets, na, ng};
    if (int rc = dtype == QS_C128 ? launch_triples_singles<2>(g, q, n, s) : launch_triples_singles<1>(g, q, n, s)) return rc;
    // the close, once per output: the connected partials into e, the singles partials into es
    hipLaunchKernelGGL(triples_close_kernel, dim3((unsigned)n), dim3(256), 0, s, g);
    note_dispatch("qs::triples_close_kernel");
    if (int rc = launch_status("triples_close launch")) return rc;
    g.part = q.part;
    g.e = es_out;
    hipLaunchKernelGGL(triples_close_kernel, dim3((unsigned)n), dim3(256), 0, s, g);
    note_dispatch("qs::triples_close_kernel");
    return launch_status("triples_close launch");
}

}  // extern "C"
