// Bandwidth-bound kernels of the path: anti-symmetrisation, spin doubling
// (Kronecker scatter) fused with anti-symmetrisation and complex cast, the
// two-body S^2 outer products, kron(h, I2) and a small-matrix transpose.
//
// All of them are HBM-bound byte movers.  Common shape: a (p,q) pair selects an
// l x l matrix over (r,s); a workgroup takes one 32 x 32 tile of it together
// with the mirrored tile, stages both in LDS (rows read coalesced), and writes
// whole contiguous runs of the output.  Every input element is read once and
// every output element written once; the (r,s) <-> (s,r) exchange happens in
// LDS (row stride 33 elements: conflict-free column reads).
//
// Algorithmic bytes: antisymmetrise 2*e*l^4; spin expansion of a
// real tensor into complex128: 8*l^4 read + 16*(2l)^4 written = 264*l^4.

#include "qs_common.h"
#include "qs_triangle.h"

namespace qs {

typedef double f64x2 __attribute__((ext_vector_type(2)));

// Store that will not be read again soon: bypasses the write-back path of L2 (measured on the
// anti-symmetrisation: 5.41 -> 5.77 TB/s at l = 256; the spin expansion, whose lanes fill a line from
// several instructions, LOSES 4 % with it and keeps plain stores).
template <typename T> __device__ __forceinline__ void stream_store(T* p, T v) { __builtin_nontemporal_store(v, p); }
// Load of what this launch reads once (the exchange check and mirrors at l = 256: 4-5 % faster than plain loads).
template <typename T> __device__ __forceinline__ T stream_load(const T* p) { return __builtin_nontemporal_load(p); }
#ifndef QS_SPIN_NT
#define QS_SPIN_NT 0          // non-temporal stores in the spin-expansion / two-body S^2 kernels (A/B switch, profiles/r03_*)
#endif

static constexpr int PT = 32;        // tile edge (elements)
static constexpr int PS = PT + 1;    // LDS row stride

template <typename T> __device__ __forceinline__ T zero_of();
template <> __device__ __forceinline__ double zero_of<double>() { return 0.0; }
template <> __device__ __forceinline__ f64x2 zero_of<f64x2>() { return f64x2{0.0, 0.0}; }

template <typename TO, typename TI> __device__ __forceinline__ TO widen(TI v);
template <> __device__ __forceinline__ double widen<double, double>(double v) { return v; }
template <> __device__ __forceinline__ f64x2 widen<f64x2, f64x2>(f64x2 v) { return v; }
template <> __device__ __forceinline__ f64x2 widen<f64x2, double>(double v) { return f64x2{v, 0.0}; }

// (ti, tj) with ti <= tj from a linear index over the upper triangle of an
// nt x nt tile grid, row by row.
__device__ __forceinline__ void tile_pair(int idx, int nt, int& ti, int& tj) {
    int i = 0;
    while (idx >= nt - i) { idx -= nt - i; ++i; }
    ti = i; tj = i + idx;
}

// Load a PT x PT tile of the l x l matrix `m` (row r0.., col c0..) into LDS; STREAM: with non-temporal loads.
template <typename T, bool STREAM = false>
__device__ __forceinline__ void load_tile(T (*t)[PS], const T* m, int l, int r0, int c0) {
    const int tx = threadIdx.x & (PT - 1), ty = threadIdx.x / PT;   // 256 threads: ty in 0..7
#pragma unroll
    for (int rr = ty; rr < PT; rr += 8) {
        const int r = r0 + rr, c = c0 + tx;
        const T* p = &m[(int64_t)r * l + c];
        t[rr][tx] = (r < l && c < l) ? (STREAM ? stream_load(p) : *p) : zero_of<T>();
    }
}

// ----------------------------------------------------------------------------
// out[pq][r][s] = u[pq][r][s] - u[pq][s][r]         (basis_set.py:776-778)
// ----------------------------------------------------------------------------
// `out` may be `u` itself (in-place form): a workgroup owns a tile and its mirror tile, reads both
// into LDS, and only stores after the barrier -- so the pointers carry no __restrict__.
template <typename T>
__global__ __launch_bounds__(256) void antisym_kernel(const T* u, T* out, int l, int nt, int npairs) {
    __shared__ T t1[PT][PS];
    __shared__ T t2[PT][PS];
    const int64_t pq = blockIdx.x / npairs;
    const int pair = blockIdx.x % npairs;
    int ti, tj;
    tile_pair(pair, nt, ti, tj);
    const T* m = u + pq * (int64_t)l * l;
    T* o = out + pq * (int64_t)l * l;
    load_tile(t1, m, l, ti * PT, tj * PT);
    if (ti != tj) load_tile(t2, m, l, tj * PT, ti * PT);
    __syncthreads();
    const int tx = threadIdx.x & (PT - 1), ty = threadIdx.x / PT;
    if (ti == tj) {
#pragma unroll
        for (int rr = ty; rr < PT; rr += 8) {
            const int r = ti * PT + rr, c = tj * PT + tx;
            if (r < l && c < l) stream_store(&o[(int64_t)r * l + c], (T)(t1[rr][tx] - t1[tx][rr]));
        }
    } else {
#pragma unroll
        for (int rr = ty; rr < PT; rr += 8) {
            int r = ti * PT + rr, c = tj * PT + tx;
            if (r < l && c < l) stream_store(&o[(int64_t)r * l + c], (T)(t1[rr][tx] - t2[tx][rr]));
            r = tj * PT + rr; c = ti * PT + tx;
            if (r < l && c < l) stream_store(&o[(int64_t)r * l + c], (T)(t2[rr][tx] - t1[tx][rr]));
        }
    }
}

// ----------------------------------------------------------------------------
// Spin doubling (+ anti-symmetrisation + cast).  P = 2p+s1, Q = 2q+s2,
// R = 2r+s3, S = 2s+s4:
//   out[P,Q,R,S] = [s1==s3][s2==s4] u[p,q,r,s] - as [s1==s4][s2==s3] u[p,q,s,r]
// (basis_set.py:772-778).  One workgroup = one (p,q) and one tile pair; it
// writes, for each of the 4 (s1,s2) output matrices, the two 64 x 64 output
// blocks fed by its input tiles, zeros included.
// ----------------------------------------------------------------------------
template <typename TI, typename TO>
__device__ __forceinline__ void spin_write_block(TO* __restrict__ o, int n2, const TI (*ta)[PS],
                                                 const TI (*tb)[PS], int l, int r0, int c0,
                                                 int s1, int s2, bool as) {
    // o: (2l x 2l) output matrix of this (P,Q); ta = u tile [r][s], tb = u tile [s][r]
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int sc = lane >> 1, s4 = lane & 1;              // local column, spin of S
    const int c = c0 + sc;
    // 64 output rows (32 local r x 2 spins), 16 per wave
#pragma unroll 4
    for (int k = 0; k < 16; ++k) {
        const int orow = wave * 16 + k;                   // 0..63
        const int rr = orow >> 1, s3 = orow & 1;
        const int r = r0 + rr;
        if (r < l && c < l) {
            TI v = zero_of<TI>();
            if (s1 == s3 && s2 == s4) v = ta[rr][sc];
            if (as && s1 == s4 && s2 == s3) v = v - tb[sc][rr];
#if QS_SPIN_NT
            stream_store(&o[(int64_t)(2 * r + s3) * n2 + (2 * c + s4)], widen<TO, TI>(v));
#else
            o[(int64_t)(2 * r + s3) * n2 + (2 * c + s4)] = widen<TO, TI>(v);
#endif
        }
    }
}

template <typename TI, typename TO>
__global__ __launch_bounds__(256) void spin_expand_kernel(const TI* __restrict__ u, TO* __restrict__ out,
                                                          int l, int nq, int nt, int npairs, int p_lo, int as) {
    // u is a block (rows, nq, l, l) of the tensor: nq = l for a leading-index slab, fewer for a slab of
    // the second index; the output block is (2 rows, 2 nq, 2l, 2l)
    __shared__ TI t1[PT][PS];
    __shared__ TI t2[PT][PS];
    const int64_t pq = blockIdx.x / npairs;                // local (p - p_lo) * nq + q
    const int pair = blockIdx.x % npairs;
    int ti, tj;
    tile_pair(pair, nt, ti, tj);
    const int64_t pl = pq / nq, q = pq % nq;
    const TI* m = u + ((pl + p_lo) * (int64_t)nq + q) * (int64_t)l * l;
    load_tile(t1, m, l, ti * PT, tj * PT);
    if (ti != tj) load_tile(t2, m, l, tj * PT, ti * PT);
    __syncthreads();
    const int n2 = 2 * l;
    const int64_t mat = (int64_t)n2 * n2;
#pragma unroll
    for (int s12 = 0; s12 < 4; ++s12) {
        const int s1 = s12 >> 1, s2 = s12 & 1;
        TO* o = out + ((2 * pl + s1) * (int64_t)(2 * nq) + (2 * q + s2)) * mat;
        if (ti == tj) {
            spin_write_block<TI, TO>(o, n2, t1, t1, l, ti * PT, tj * PT, s1, s2, as != 0);
        } else {
            spin_write_block<TI, TO>(o, n2, t1, t2, l, ti * PT, tj * PT, s1, s2, as != 0);
            spin_write_block<TI, TO>(o, n2, t2, t1, l, tj * PT, ti * PT, s1, s2, as != 0);
        }
    }
}

// ----------------------------------------------------------------------------
// out[i, 2p+s, 2q+t] = [s==t] h[i,p,q]                 (basis_set.py:768-770)
// ----------------------------------------------------------------------------
template <typename TI, typename TO>
__global__ void kron_eye2_kernel(const TI* __restrict__ h, TO* __restrict__ out, int64_t nmat, int l) {
    const int64_t n2 = 2 * (int64_t)l;
    const int64_t total = nmat * n2 * n2;
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < total;
         i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t mat = i / (n2 * n2), rem = i % (n2 * n2);
        const int P = (int)(rem / n2), Q = (int)(rem % n2);
        TI v = zero_of<TI>();
        if ((P & 1) == (Q & 1)) v = h[(mat * l + (P >> 1)) * l + (Q >> 1)];
        out[i] = widen<TO, TI>(v);
    }
}

// ----------------------------------------------------------------------------
// Two-body S^2 (basis_set.py:745-747, :525-526), complex128, n spin-orbitals:
//   out[p,q,r,s] = sum_i S_i[p,r] S_i[q,s] - as * S_i[p,s] S_i[q,r]
// accumulated in the reference's order i = x, y, z.  One workgroup per (p,q)
// and a chunk of rows r (all of them when there are enough (p,q) pairs to fill the chip); rows p and q of the
// three matrices are staged in LDS.
// ----------------------------------------------------------------------------
__device__ __forceinline__ f64x2 cmul(f64x2 a, f64x2 b) {
    return f64x2{a[0] * b[0] - a[1] * b[1], a[0] * b[1] + a[1] * b[0]};
}

__global__ __launch_bounds__(1024) void spin2_tb_kernel(const f64x2* __restrict__ S, f64x2* __restrict__ out,
                                                        int n, int p_lo, int rchunks, int rows_per_chunk, int cw, int as) {
    extern __shared__ __attribute__((aligned(16))) double smem_raw[];
    f64x2* sp = reinterpret_cast<f64x2*>(smem_raw);   // [3][n] rows p
    f64x2* sq = sp + 3 * n;                           // [3][n] rows q
    const int64_t blk = blockIdx.x;
    const int rc = (int)(blk % rchunks);
    const int64_t pq = blk / rchunks;
    const int q = (int)(pq % n);
    const int64_t pl = pq / n;
    const int p = (int)pl + p_lo;
    for (int i = threadIdx.x; i < 3 * n; i += blockDim.x) {
        const int k = i / n, c = i % n;
        sp[i] = S[((int64_t)k * n + p) * n + c];
        sq[i] = S[((int64_t)k * n + q) * n + c];
    }
    __syncthreads();
    f64x2* o = out + (pl * n + q) * (int64_t)n * n;
    const int r_end = min(n, (rc + 1) * rows_per_chunk);
    // The workgroup is a (rows x cw columns) grid of threads: cw = the columns rounded up to whole waves (at most the
    // workgroup), so a small n does not leave most lanes idle.  A lane keeps its column s for all its rows: S_i[q, s]
    // (and S_i[p, s] for the exchange term) are read from LDS once per column, only the row factors S_i[p, r] /
    // S_i[q, r] (one address per wave: a broadcast) per row.
    const int ts = threadIdx.x % cw, tr = threadIdx.x / cw, rg = blockDim.x / cw;
    if (tr >= rg) return;     // cw does not divide the workgroup: the surplus lanes would repeat rows of row group 0
    for (int s = ts; s < n; s += cw) {
        f64x2 qs[3], ps[3];
#pragma unroll
        for (int k = 0; k < 3; ++k) { qs[k] = sq[k * n + s]; ps[k] = sp[k * n + s]; }
        for (int r = rc * rows_per_chunk + tr; r < r_end; r += rg) {
            f64x2 v = f64x2{0.0, 0.0}, w = f64x2{0.0, 0.0};
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                v = v + cmul(sp[k * n + r], qs[k]);
                if (as) w = w + cmul(ps[k], sq[k * n + r]);
            }
#if QS_SPIN_NT
            stream_store(&o[(int64_t)r * n + s], as ? (v - w) : v);
#else
            o[(int64_t)r * n + s] = as ? (v - w) : v;
#endif
        }
    }
}

// out (cols x rows) = in (rows x cols)^T, small matrices only.
template <typename T>
__global__ void transpose_kernel(const T* __restrict__ in, T* __restrict__ out, int64_t rows, int64_t cols) {
    const int64_t total = rows * cols;
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < total;
         i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t c = i / rows, r = i % rows;   // out index i = c*rows + r
        out[i] = in[r * cols + c];
    }
}

// ----------------------------------------------------------------------------
// Particle-exchange symmetry  t[a,b,r,s] == t[b,a,s,r]  (random_basis.py:52; every physical two-body tensor has it):
// the check of an input tensor and the mirror that completes an (n, n, m, m) tensor computed on `a <= b` only.  Both
// names carry "transpose": they move bytes, and a dispatch record counts products by the names that lack the word.
// ----------------------------------------------------------------------------
__device__ __forceinline__ bool same_bits(double x, double y) { return __double_as_longlong(x) == __double_as_longlong(y); }
__device__ __forceinline__ bool same_bits(f64x2 x, f64x2 y) { return same_bits(x[0], y[0]) && same_bits(x[1], y[1]); }

// (the pair decode, triangle_row, is qs_triangle.h's: the products' triangular batch uses the same one)

// *flag |= 1 iff some u[a,b,c,d] differs BITWISE from u[b,a,d,c] (-0.0 against +0.0 differs, equal NaNs do not).  A
// workgroup takes one pair a <= b and one 32 x 32 tile (ti, tj) of u[a,b] together with tile (tj, ti) of u[b,a]; on the
// diagonal a == b that is the test that u[a,a] is a symmetric matrix.  It looks at the flag first: once a difference
// is known, the rest of the grid costs no memory traffic.  Only the tile of u[b,a] is turned in LDS: a thread compares
// the four elements of u[a,b] that it loaded itself, from its registers.  Nothing here is read twice: the loads are
// non-temporal.  (l = 256 fp64, same call: both tiles through LDS 6.78 ms, this 5.41, with non-temporal loads 5.15 =
// 6.7 TB/s; profiles/exchange_overlap_ab.txt.)
template <typename T>
__global__ __launch_bounds__(256) void exchange_transpose_check_kernel(const T* __restrict__ u, int* flag, int l, int nt) {
    __shared__ T t2[PT][PS];
    if (__atomic_load_n(flag, __ATOMIC_RELAXED)) return;
    const int ntiles = nt * nt;
    const int64_t pair = blockIdx.x / ntiles;
    const int tile = blockIdx.x % ntiles;
    const int ti = tile / nt, tj = tile % nt;
    const int64_t a = triangle_row((uint32_t)pair, (uint32_t)l);
    const int64_t b = a + (pair - (a * l - a * (a - 1) / 2));
    const int64_t ll = (int64_t)l * l;
    const T* uab = u + (a * l + b) * ll;
    const int tx = threadIdx.x & (PT - 1), ty = threadIdx.x / PT;
    T mine[PT / 8];
#pragma unroll
    for (int j = 0; j < PT / 8; ++j) {
        const int r = ti * PT + ty + 8 * j, c = tj * PT + tx;
        mine[j] = (r < l && c < l) ? stream_load(&uab[(int64_t)r * l + c]) : zero_of<T>();
    }
    load_tile<T, true>(t2, u + (b * l + a) * ll, l, tj * PT, ti * PT);
    __syncthreads();
    bool same = true;
#pragma unroll
    for (int j = 0; j < PT / 8; ++j) same = same && same_bits(mine[j], t2[tx][ty + 8 * j]);   // (both zero past the edge)
    if (!same) *flag = 1;
}

// In place on t (n, n, m, m):  t[a,b,r,s] = t[b,a,s,r]  for every pair with a / block > b / block; nothing else is
// written.  A workgroup takes one such pair and one 32 x 32 tile (ti, tj) of t[a,b]: it reads tile (tj, ti) of t[b,a]
// by rows, turns it in LDS and writes whole rows of 32 elements (two 128-byte lines of fp64 where m is a multiple of 16).
// Non-temporal loads as well as stores (l = 256 fp64, same call: block 1 6.25 -> 5.93 ms, block 64 4.57 -> 4.33).
template <typename T>
__global__ __launch_bounds__(256) void exchange_transpose_kernel(T* t, int n, int m, int nt, int block) {
    __shared__ T t1[PT][PS];
    const int ntiles = nt * nt;
    const int64_t pair = blockIdx.x / ntiles;
    const int tile = blockIdx.x % ntiles;
    const int ti = tile / nt, tj = tile % nt;
    // pairs row by row: the rows of block row A = a / block hold A * block pairs each
    const int64_t bb = (int64_t)block * block;
    int64_t A = (int64_t)((1.0 + sqrt(1.0 + 8.0 * (double)pair / (double)bb)) * 0.5);
    if (A < 1) A = 1;
    while (A > 1 && bb * (A * (A - 1) / 2) > pair) --A;
    while (bb * ((A + 1) * A / 2) <= pair) ++A;
    const int64_t rem = pair - bb * (A * (A - 1) / 2), row_len = A * block;
    const int64_t a = A * block + rem / row_len, b = rem % row_len;
    const int64_t mm = (int64_t)m * m;
    load_tile<T, true>(t1, (const T*)t + (b * n + a) * mm, m, tj * PT, ti * PT);
    __syncthreads();
    T* o = t + (a * n + b) * mm;
    const int tx = threadIdx.x & (PT - 1), ty = threadIdx.x / PT;
#pragma unroll
    for (int rr = ty; rr < PT; rr += 8) {
        const int r = ti * PT + rr, c = tj * PT + tx;
        if (r < m && c < m) stream_store(&o[(int64_t)r * m + c], t1[tx][rr]);
    }
}

// In place on t (n, n, m, m):  t[i,j][r,s] = t[j,i][s,r]  for every pair i <= j and every s < r; nothing else is written (the
// fill after the route's column-triangle products, which store the blocks that meet s >= r of EVERY pair).  A workgroup
// takes one pair i <= j and one 32 x 32 tile (ti, tj <= ti) of t[i,j]: it reads tile (tj, ti) of t[j,i] by rows, turns it
// in LDS and writes rows.  A diagonal tile -- and with it the diagonal pair i == j -- stores s < r only: the elements
// s >= r were computed directly and differ from their mirror images in rounding.  Sources (strictly upper) and
// destinations (strictly lower) never overlap; a diagonal tile is read whole before its barrier and written after it.
template <typename T>
__global__ __launch_bounds__(256) void exchange_transpose_lower_kernel(T* t, int n, int m, int nt) {
    __shared__ T t1[PT][PS];
    const uint32_t ntl = (uint32_t)nt * (uint32_t)(nt + 1) / 2u;
    const uint32_t pair = blockIdx.x / ntl, tile = blockIdx.x - pair * ntl;
    const uint32_t i = triangle_row(pair, (uint32_t)n), j = i + (pair - triangle_row_start(i, (uint32_t)n));
    const uint32_t tj = triangle_row(tile, (uint32_t)nt), ti = tj + (tile - triangle_row_start(tj, (uint32_t)nt));      // tj <= ti
    const int64_t mm = (int64_t)m * m;
    load_tile<T, true>(t1, (const T*)t + ((int64_t)j * n + i) * mm, m, (int)tj * PT, (int)ti * PT);
    __syncthreads();
    T* o = t + ((int64_t)i * n + j) * mm;
    const int tx = threadIdx.x & (PT - 1), ty = threadIdx.x / PT;
#pragma unroll
    for (int rr = ty; rr < PT; rr += 8) {
        const int r = (int)ti * PT + rr, c = (int)tj * PT + tx;
        if (r < m && c < r) stream_store(&o[(int64_t)r * m + c], t1[tx][rr]);
    }
}

// ----------------------------------------------------------------------------
// The exchange route's leading indices on pairs (qs_api.hip): seen through its TRAILING indices a tensor with the symmetry
// has u[:, :, c, d] == u[:, :, d, c]^T, so the two leading contractions are a two-sided product of the matrix over (a, b)
// for the pairs d >= c alone -- once the pair matrix l^2 x l^2 is turned, and turned back afterwards.  Two byte movers do
// that.  A tile fixes one index of each pair and turns the other two: on both sides it moves runs of 32 or 64 contiguous
// elements, and the rows of a tile lie a whole matrix (l^2 elements) or more apart.
// ----------------------------------------------------------------------------

// Rows i < n of a triangle in tiles of ts elements: row i has the tiles that reach its side of the diagonal -- `up`: tiles
// i / ts ... nt - 1 (columns j >= i), else tiles 0 ... i / ts (columns j <= i).  All of them, counted (a grid extent):
__host__ __device__ inline int64_t triangle_tiles(int n, bool up, int ts) {
    const int nt = (n + ts - 1) / ts;
    int64_t sum = 0;
    for (int B = 0; B < nt; ++B) sum += (int64_t)(n - B * ts < ts ? n - B * ts : ts) * (up ? nt - B : B + 1);
    return sum;
}

// ... and the idx-th of them, row by row: returns the row, idx becomes the tile's place among the row's own.  (Rows of one
// block of ts have the same count, so the loop runs over blocks; 32-bit arithmetic and one division -- with 64-bit
// divisions in a flat index the way back took 10.8 ms where it now takes 7.5.)
__device__ __forceinline__ int triangle_tiles_row(uint32_t& idx, int n, bool up, int ts) {
    const int nt = (n + ts - 1) / ts;
    int B = 0, cnt;
    for (;; ++B) {
        cnt = up ? nt - B : B + 1;
        const uint32_t span = (uint32_t)(n - B * ts < ts ? n - B * ts : ts) * cnt;
        if (idx < span || B >= nt - 1) break;
        idx -= span;
    }
    const uint32_t r = idx / cnt;
    idx -= r * cnt;
    return B * ts + (int)r;
}

// dst[c,d][a,b] = src[a,b,c,d] for the pairs d >= c; nothing is written at d < c.  Both (l, l, l, l).  A workgroup fixes
// (a, c) and turns one 32 x 32 tile of (b, d): it reads rows b (l^2 apart, d contiguous) and writes rows d (l^2 apart, b
// contiguous).  The grid is three-dimensional: x = the tiles along b; a and the pair (c, tile along d) are y and z, or z
// and y with A_SLOWEST (fp64 is faster with c slowest, 6.6 against 7.1 ms at l = 256, complex128 with a slowest, 12.1
// against 13.4: profiles/exchange_leading_pairs_ab.txt section 1, with the other tiles and walks tried).
template <typename T, bool A_SLOWEST>
__global__ __launch_bounds__(256) void exchange_pair_transpose_kernel(const T* __restrict__ src, T* __restrict__ dst, int l) {
    __shared__ T t[PT][PS];
    const int tb = blockIdx.x, a = A_SLOWEST ? blockIdx.z : blockIdx.y;
    uint32_t idx = A_SLOWEST ? blockIdx.y : blockIdx.z;
    const int c = triangle_tiles_row(idx, l, true, PT), td = c / PT + (int)idx;
    if (a >= l || c >= l) return;
    const int64_t ll = (int64_t)l * l;
    const int tx = threadIdx.x & (PT - 1), ty = threadIdx.x / PT;
    const T* s = src + (a * ll + c) * l;                       // + b l^2 + d
#pragma unroll
    for (int rr = ty; rr < PT; rr += 8) {
        const int b = tb * PT + rr, d = td * PT + tx;
        if (b < l && d < l && d >= c) t[rr][tx] = stream_load(&s[b * ll + d]);
    }
    __syncthreads();
    T* o = dst + (c * ll + a) * l;                             // + d l^2 + b
#pragma unroll
    for (int rr = ty; rr < PT; rr += 8) {
        const int d = td * PT + rr, b = tb * PT + tx;
        if (b < l && d < l && d >= c) stream_store(&o[d * ll + b], t[tx][rr]);
    }
}

// The way back, with the other half filled in: src (l, l, m, m) is stored on the pairs d >= c only; on the pairs q >= p
//   dst[p,q][c,d] = src[c,d][p,q]  where d >= c  (`upper` tiles: fix (p, c), turn (q, d)),
//                 = src[d,c][q,p]  where d <  c  (the others:    fix (q, c), turn (p, d));
// dst (m, m, l, l), nothing is written at q < p and src is never read at d < c.  Either kind reads rows d with the other
// turned index y contiguous (a TD x 32 tile) and writes rows y with d contiguous.  The grid: z = the kind, x = the pair (fixed
// index of the result's pair, tile along y), y = the pair (c, tile along d); either kind has its own triangles, the grid
// takes the larger and the few surplus workgroups leave at once.  TD = 64 for fp64 (512-byte runs of the stores, half the
// workgroups: 8.8 -> 7.5 ms at l = 256), 32 for complex128 (12.1 ms; 64 there: 13.8).
template <typename T, int TD>
__global__ __launch_bounds__(256) void exchange_pair_transpose_back_kernel(const T* __restrict__ src, T* __restrict__ dst, int l,
                                                                           int m) {
    __shared__ T t[TD][PS];
    const bool upper = blockIdx.z == 0;
    // upper: x = p with the tiles of q >= p, c with the tiles of d >= c; else x = q with the tiles of p <= q, and c >= 1 with
    // the tiles of d <= c - 1
    const int lc = upper ? l : l - 1;
    uint32_t ix = blockIdx.x, ic = blockIdx.y;
    if (ix >= (uint32_t)triangle_tiles(m, upper, PT) || ic >= (uint32_t)triangle_tiles(lc, upper, TD)) return;
    const int x = triangle_tiles_row(ix, m, upper, PT);
    int c = triangle_tiles_row(ic, lc, upper, TD);
    if (x >= m || c >= lc) return;
    int tyy = (int)ix, td = (int)ic;            // tiles along y and along d
    if (upper) { tyy += x / PT; td += c / TD; } else { c += 1; }
    const int64_t ll = (int64_t)l * l, mm = (int64_t)m * m;
    const T* s = src + (upper ? ((int64_t)c * l * m + x) * m : ((int64_t)c * m + x) * m);      // + d * srs + y
    T* o = dst + (upper ? ((int64_t)x * m * l + c) * l : ((int64_t)x * l + c) * l);            // + y * drs + d
    const int64_t srs = upper ? mm : l * mm, drs = upper ? ll : m * ll;
#pragma unroll
    for (int rr = threadIdx.x / PT; rr < TD; rr += 256 / PT) {
        const int d = td * TD + rr, tx = threadIdx.x & (PT - 1), y = tyy * PT + tx;
        if (upper ? (y >= x && y < m && d >= c && d < l) : (y <= x && d < c)) t[rr][tx] = stream_load(&s[d * srs + y]);
    }
    __syncthreads();
#pragma unroll
    for (int rr = threadIdx.x / TD; rr < PT; rr += 256 / TD) {
        const int y = tyy * PT + rr, tx = threadIdx.x & (TD - 1), d = td * TD + tx;
        if (upper ? (y >= x && y < m && d >= c && d < l) : (y <= x && d < c)) stream_store(&o[y * drs + d], t[tx][rr]);
    }
}

// ------------------------------------------------------------------ launchers

static inline unsigned stream_grid(int64_t total, int block) {
    const int64_t want = cdiv(total, block);
    return (unsigned)(want < 1 ? 1 : (want > 256 * 32 ? 256 * 32 : want));
}

int transpose_small(int dtype, const void* in, void* out, int64_t rows, int64_t cols, hipStream_t stream) {
    const unsigned grid = stream_grid(rows * cols, 256);
    if (dtype == QS_F64)
        hipLaunchKernelGGL(transpose_kernel<double>, dim3(grid), dim3(256), 0, stream,
                           (const double*)in, (double*)out, rows, cols);
    else
        hipLaunchKernelGGL(transpose_kernel<f64x2>, dim3(grid), dim3(256), 0, stream,
                           (const f64x2*)in, (f64x2*)out, rows, cols);
    return launch_status("transpose_small launch");
}

int antisymmetrize(int dtype, const void* u, void* out, int64_t npq, int64_t l, hipStream_t stream) {
    const int nt = (int)cdiv(l, PT);
    const int64_t npairs = (int64_t)nt * (nt + 1) / 2;
    const int64_t nwg = npq * npairs;
    if (nwg >= (int64_t(1) << 31)) return QS_ERR_BAD_EXTENT;
    if (dtype == QS_F64)
        hipLaunchKernelGGL(antisym_kernel<double>, dim3((unsigned)nwg), dim3(256), 0, stream,
                           (const double*)u, (double*)out, (int)l, nt, (int)npairs);
    else
        hipLaunchKernelGGL(antisym_kernel<f64x2>, dim3((unsigned)nwg), dim3(256), 0, stream,
                           (const f64x2*)u, (f64x2*)out, (int)l, nt, (int)npairs);
    note_dispatch("qs::antisym_kernel<%s>", dtype == QS_F64 ? "double" : "f64x2");
    return launch_status("antisymmetrize launch");
}

// pairs (a, b) of an n x n grid with a / block > b / block
static inline int64_t exchange_lower_pairs(int64_t n, int64_t block) {
    const int64_t full = n / block, rest = n % block;
    return block * block * (full * (full - 1) / 2) + rest * full * block;
}

bool exchange_grids_fit(int64_t L, int64_t M) {
    const int64_t nl = cdiv(L, PT), nm = cdiv(M, PT), top = int64_t(1) << 31, big = L > M ? L : M;
    return L * (L + 1) / 2 * nl * nl < top && big * (big - 1) / 2 * nm * nm < top;
}

int exchange_check(int dtype, const void* u, int64_t l, int* flag, hipStream_t stream) {
    const int nt = (int)cdiv(l, PT);
    const int64_t nwg = l * (l + 1) / 2 * nt * nt;
    if (nwg >= (int64_t(1) << 31)) return QS_ERR_BAD_EXTENT;
    if (dtype == QS_F64)
        hipLaunchKernelGGL(exchange_transpose_check_kernel<double>, dim3((unsigned)nwg), dim3(256), 0, stream,
                           (const double*)u, flag, (int)l, nt);
    else
        hipLaunchKernelGGL(exchange_transpose_check_kernel<f64x2>, dim3((unsigned)nwg), dim3(256), 0, stream,
                           (const f64x2*)u, flag, (int)l, nt);
    note_dispatch("qs::exchange_transpose_check_kernel<%s>", dtype == QS_F64 ? "double" : "f64x2");
    return launch_status("exchange_check launch");
}

int exchange_mirror(int dtype, void* t, int64_t n, int64_t m, int64_t block, hipStream_t stream) {
    const int nt = (int)cdiv(m, PT);
    const int64_t pairs = exchange_lower_pairs(n, block);
    if (pairs == 0) return QS_OK;                          // one block row: nothing lies below it
    const int64_t nwg = pairs * nt * nt;
    if (nwg >= (int64_t(1) << 31)) return QS_ERR_BAD_EXTENT;
    if (dtype == QS_F64)
        hipLaunchKernelGGL(exchange_transpose_kernel<double>, dim3((unsigned)nwg), dim3(256), 0, stream,
                           (double*)t, (int)n, (int)m, nt, (int)block);
    else
        hipLaunchKernelGGL(exchange_transpose_kernel<f64x2>, dim3((unsigned)nwg), dim3(256), 0, stream,
                           (f64x2*)t, (int)n, (int)m, nt, (int)block);
    note_dispatch("qs::exchange_transpose_kernel<%s>", dtype == QS_F64 ? "double" : "f64x2");
    return launch_status("exchange_mirror launch");
}

bool exchange_mirror_lower_fits(int64_t n, int64_t m) {
    const int64_t nt = cdiv(m, PT);
    return n > 0 && m > 0 && n <= 4096 && m <= 4096 && n * (n + 1) / 2 * (nt * (nt + 1) / 2) < (int64_t(1) << 31);
}

int exchange_mirror_lower(int dtype, void* t, int64_t n, int64_t m, hipStream_t stream) {
    if (dtype != QS_F64) return QS_ERR_BAD_DTYPE;
    if (!exchange_mirror_lower_fits(n, m)) return QS_ERR_BAD_EXTENT;
    const int nt = (int)cdiv(m, PT);
    const int64_t nwg = n * (n + 1) / 2 * ((int64_t)nt * (nt + 1) / 2);
    hipLaunchKernelGGL(exchange_transpose_lower_kernel<double>, dim3((unsigned)nwg), dim3(256), 0, stream, (double*)t, (int)n,
                       (int)m, nt);
    note_dispatch("qs::exchange_transpose_lower_kernel<double>");
    return launch_status("exchange_mirror_lower launch");
}

// The pair movers' grids: x, y, z extents (y and z hold at most 65535 workgroups each, a whole grid fewer than 2^31).
static inline int pair_back_td(int dtype) { return dtype == QS_F64 ? 64 : PT; }

struct PairGrid { int64_t x, y, z; bool fits() const { return y <= 65535 && z <= 65535 && x * y * z < (int64_t(1) << 31); } };

static inline PairGrid pair_transpose_grid(int dtype, int64_t l) {
    const int64_t pairs = triangle_tiles((int)l, true, PT);
    return dtype == QS_F64 ? PairGrid{cdiv(l, PT), l, pairs} : PairGrid{cdiv(l, PT), pairs, l};
}

static inline PairGrid pair_transpose_back_grid(int dtype, int64_t l, int64_t m) {
    const int td = pair_back_td(dtype);
    const int64_t xu = triangle_tiles((int)m, true, PT), xl = triangle_tiles((int)m, false, PT);
    const int64_t cu = triangle_tiles((int)l, true, td), cl = triangle_tiles((int)l - 1, false, td);
    return PairGrid{xu > xl ? xu : xl, cu > cl ? cu : cl, 2};
}

bool exchange_pair_grids_fit(int dtype, int64_t L, int64_t M) {
    return L > 0 && M > 0 && L <= 4096 && M <= 4096 && pair_transpose_grid(dtype, L).fits() && pair_transpose_back_grid(dtype, L, M).fits();
}

int exchange_pair_transpose(int dtype, const void* src, void* dst, int64_t l, hipStream_t stream) {
    const PairGrid g = pair_transpose_grid(dtype, l);
    if (l <= 0 || l > 4096 || !g.fits()) return QS_ERR_BAD_EXTENT;
    const dim3 grid((unsigned)g.x, (unsigned)g.y, (unsigned)g.z);
    if (dtype == QS_F64)
        hipLaunchKernelGGL((exchange_pair_transpose_kernel<double, false>), grid, dim3(256), 0, stream,
                           (const double*)src, (double*)dst, (int)l);
    else
        hipLaunchKernelGGL((exchange_pair_transpose_kernel<f64x2, true>), grid, dim3(256), 0, stream,
                           (const f64x2*)src, (f64x2*)dst, (int)l);
    note_dispatch("qs::exchange_pair_transpose_kernel<%s>", dtype == QS_F64 ? "double, false" : "f64x2, true");
    return launch_status("exchange_pair_transpose launch");
}

int exchange_pair_transpose_back(int dtype, const void* src, void* dst, int64_t l, int64_t m, hipStream_t stream) {
    if (l <= 0 || m <= 0 || l > 4096 || m > 4096) return QS_ERR_BAD_EXTENT;
    const PairGrid g = pair_transpose_back_grid(dtype, l, m);
    if (!g.fits()) return QS_ERR_BAD_EXTENT;
    const dim3 grid((unsigned)g.x, (unsigned)g.y, (unsigned)g.z);
    if (dtype == QS_F64)
        hipLaunchKernelGGL((exchange_pair_transpose_back_kernel<double, 64>), grid, dim3(256), 0, stream,
                           (const double*)src, (double*)dst, (int)l, (int)m);
    else
        hipLaunchKernelGGL((exchange_pair_transpose_back_kernel<f64x2, PT>), grid, dim3(256), 0, stream,
                           (const f64x2*)src, (f64x2*)dst, (int)l, (int)m);
    note_dispatch("qs::exchange_pair_transpose_back_kernel<%s>", dtype == QS_F64 ? "double, 64" : "f64x2, 32");
    return launch_status("exchange_pair_transpose_back launch");
}

int spin_expand(int in_dtype, int out_dtype, const void* u, void* out, int64_t l, int64_t nq, int64_t p_lo,
                int64_t p_hi, int as, hipStream_t stream) {
    const int nt = (int)cdiv(l, PT);
    const int64_t npairs = (int64_t)nt * (nt + 1) / 2;
    const int64_t nwg = (p_hi - p_lo) * nq * npairs;
    if (nwg >= (int64_t(1) << 31)) return QS_ERR_BAD_EXTENT;
    const dim3 grid((unsigned)nwg), block(256);
    if (in_dtype == QS_F64 && out_dtype == QS_F64)
        hipLaunchKernelGGL((spin_expand_kernel<double, double>), grid, block, 0, stream,
                           (const double*)u, (double*)out, (int)l, (int)nq, nt, (int)npairs, (int)p_lo, as);
    else if (in_dtype == QS_F64 && out_dtype == QS_C128)
        hipLaunchKernelGGL((spin_expand_kernel<double, f64x2>), grid, block, 0, stream,
                           (const double*)u, (f64x2*)out, (int)l, (int)nq, nt, (int)npairs, (int)p_lo, as);
    else if (in_dtype == QS_C128 && out_dtype == QS_C128)
        hipLaunchKernelGGL((spin_expand_kernel<f64x2, f64x2>), grid, block, 0, stream,
                           (const f64x2*)u, (f64x2*)out, (int)l, (int)nq, nt, (int)npairs, (int)p_lo, as);
    else
        return QS_ERR_BAD_DTYPE;
    note_dispatch("qs::spin_expand_kernel<%s, %s>", in_dtype == QS_F64 ? "double" : "f64x2",
                  out_dtype == QS_F64 ? "double" : "f64x2");
    return launch_status("spin_expand launch");
}

int kron_eye2(int in_dtype, int out_dtype, const void* h, void* out, int64_t nmat, int64_t l,
              hipStream_t stream) {
    const unsigned grid = stream_grid(nmat * 4 * l * l, 256);
    if (in_dtype == QS_F64 && out_dtype == QS_F64)
        hipLaunchKernelGGL((kron_eye2_kernel<double, double>), dim3(grid), dim3(256), 0, stream,
                           (const double*)h, (double*)out, nmat, (int)l);
    else if (in_dtype == QS_F64 && out_dtype == QS_C128)
        hipLaunchKernelGGL((kron_eye2_kernel<double, f64x2>), dim3(grid), dim3(256), 0, stream,
                           (const double*)h, (f64x2*)out, nmat, (int)l);
    else if (in_dtype == QS_C128 && out_dtype == QS_C128)
        hipLaunchKernelGGL((kron_eye2_kernel<f64x2, f64x2>), dim3(grid), dim3(256), 0, stream,
                           (const f64x2*)h, (f64x2*)out, nmat, (int)l);
    else
        return QS_ERR_BAD_DTYPE;
    note_dispatch("qs::kron_eye2_kernel");
    return launch_status("kron_eye2 launch");
}

int spin2_two_body(const void* S, void* out, int64_t n, int64_t p_lo, int64_t p_hi, int as,
                   hipStream_t stream) {
    // one workgroup stages rows p and q of the three matrices (96 n bytes) and writes rows_per_chunk * n elements:
    // whole (p, q) matrices per workgroup unless that leaves the chip short of workgroups (the first version
    // always took 8 rows: 48 KB staged per 64 KB written at n = 512)
    const int64_t npq = (p_hi - p_lo) * n;
    int64_t want = cdiv(2048, npq);
    if (want < 1) want = 1;
    if (want > cdiv(n, 8)) want = cdiv(n, 8);
    const int rows_per_chunk = (int)cdiv(n, want);
    const int rchunks = (int)cdiv(n, rows_per_chunk);
    const int64_t nwg = npq * rchunks;
    if (nwg >= (int64_t(1) << 31)) return QS_ERR_BAD_EXTENT;
    const size_t lds = sizeof(double) * 2 * 6 * n;       // rows p and q of S_x, S_y, S_z: 96 n bytes
    if (lds > 160 * 1024) return QS_ERR_BAD_EXTENT;      // n <= 1706 spin orbitals (LDS of one CU)
    static PerDeviceLds lds_opt_in;                     // beyond 64 KB (n > 682) the kernel opts in, per device
    if (int rc = opt_in_dynamic_lds((const void*)spin2_tb_kernel, lds, lds_opt_in, "hipFuncSetAttribute(spin2_tb)"))
        return rc;
    // beyond 64 KB of LDS one workgroup fits a CU: make it 1024 threads so that the CU still has 16 waves in flight
    const int threads = lds > 64 * 1024 ? 1024 : 256;
    int cw = (int)(cdiv(n, 64) * 64);
    if (cw > threads) cw = threads;
    hipLaunchKernelGGL(spin2_tb_kernel, dim3((unsigned)nwg), dim3(threads), lds, stream,
                       (const f64x2*)S, (f64x2*)out, (int)n, (int)p_lo, rchunks, rows_per_chunk, cw, as);
    note_dispatch("qs::spin2_tb_kernel");
    return launch_status("spin2_two_body launch");
}

}  // namespace qs
