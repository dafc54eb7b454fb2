/*
 * qs_amd.h -- C ABI of the MI355X (gfx950) integral basis-transformation path.
 *
 * The reference (HyQD/quantum-systems v0.2.6) is pure Python and has no FFI:
 * its seam is the injected array module (`np=` / `change_module`,
 * quantum_systems/basis_set.py:32-38, :268-296).  The entry points below are
 * what a binding for that seam calls in place of the NumPy calls on the hot
 * path; each one names the reference call it replaces.  `INTEGRATION.md` shows
 * the ctypes stub a maintainer of the reference would add.
 *
 * Conventions
 *   - every pointer is a DEVICE pointer (hipMalloc / torch CUDA tensor
 *     storage), 8-byte aligned (16 for complex), row-major, contiguous;
 *   - complex128 is interleaved (re, im) doubles, as NumPy / torch store it;
 *   - conjugation is resolved by the caller (`Ct` is passed explicitly);
 *   - `stream` is a hipStream_t passed as void*; all work is enqueued on it
 *     and the call returns without synchronising;
 *   - the library allocates nothing: outputs and workspace are the caller's;
 *   - no process-global mutable state: caches are keyed by device ordinal, the
 *     error / dispatch / tuning records are thread-local; calls are re-entrant
 *     for distinct streams and devices (the current device must be the one
 *     that owns the pointers and the stream);
 *   - return value: QS_OK (0) or a negative QS_ERR_* code, never throws.
 *
 * dtype codes: QS_F64 = real fp64, QS_C128 = complex128.
 */
#ifndef QS_AMD_H
#define QS_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define QS_ABI_VERSION 4

enum {
    QS_OK = 0,
    QS_ERR_BAD_EXTENT = -1,   /* non-positive or overflowing dimension      */
    QS_ERR_NULL_POINTER = -2, /* required pointer is NULL                    */
    QS_ERR_MISALIGNED = -3,   /* pointer not aligned to its element size     */
    QS_ERR_WORKSPACE = -4,    /* workspace smaller than qs_*_workspace says  */
    QS_ERR_HIP = -5,          /* a HIP runtime call or kernel launch failed  */
    QS_ERR_BAD_DTYPE = -6,    /* dtype code not QS_F64 / QS_C128             */
    QS_ERR_ALIAS = -7,        /* output aliases an input where not allowed   */
    QS_ERR_COMM = -8          /* RCCL call failed / librccl not loadable     */
};

enum { QS_F64 = 0, QS_C128 = 1 };

/* ABI version of the loaded library (QS_ABI_VERSION it was built with). */
int qs_abi_version(void);

/* Text for a QS_ERR_* code (static storage). */
const char* qs_error_string(int code);

/* Last HIP error string recorded by this thread's most recent QS_ERR_HIP. */
const char* qs_last_hip_error(void);

/*
 * Row-major (batched) matrix product  out[b] = A[b] . B[b]
 *   A[b] : (m, k), leading dimension lda, batch stride stride_a (0 = shared)
 *   B[b] : (k, n), leading dimension ldb, batch stride stride_b (0 = shared)
 *   out[b]: (m, n), leading dimension ldc, batch stride stride_c
 * Strides and leading dimensions are in ELEMENTS of the dtype.
 * accumulate != 0 computes out[b] += A[b] . B[b] (used to close a contraction
 * whose summed index arrives in several slabs, see qs_transform_two_body_partial).
 * Replaces np.dot / np.tensordot over one index:
 *   transform_spf / transform_bra_spf   basis_set.py:321-327
 *   transform_one_body_elements         basis_set.py:329-334
 * and is the building block of qs_transform_two_body.
 */
int qs_matmul(int dtype, const void* A, const void* B, void* out,
              int64_t m, int64_t n, int64_t k,
              int64_t lda, int64_t ldb, int64_t ldc,
              int64_t batch, int64_t stride_a, int64_t stride_b,
              int64_t stride_c, int accumulate, void* stream);

/*
 * qs_matmul over a TRIANGULAR batch: the entries are the grid_n (grid_n + 1) / 2
 * pairs (i, j >= i) of a grid_n x grid_n grid, in row-major order, and the
 * operands of pair (i, j) sit at its flat index f = i * grid_n + j:
 *   A + f * stride_a,  B + f * stride_b,  out + f * stride_c   (0 = shared).
 * Nothing is written at the flat indices of the pairs j < i, and nothing read
 * there reaches an output (a border tile of the edge forms loads past its own
 * entry, inside the operand, into rows that are never stored).  One launch on
 * exactly the pairs (the d and c contractions of the exchange route below).
 */
int qs_matmul_pairs(int dtype, const void* A, const void* B, void* out,
                    int64_t m, int64_t n, int64_t k,
                    int64_t lda, int64_t ldb, int64_t ldc,
                    int64_t grid_n, int64_t stride_a, int64_t stride_b,
                    int64_t stride_c, int accumulate, void* stream);

/*
 * ... which ALSO stores every entry (i, j > i) transposed at the flat index of
 * (j, i): element (r, c) of the pair's m x m result at
 *   out + (j * grid_n + i) * stride_c + c * ldc + r.
 * Entries (i, i) are stored once.  The transposes come out of the registers
 * that hold the result, so they are its bits.  Requires m == n and
 * accumulate == 0, and a product that the dispatch puts on a kernel with this
 * epilogue -- today float64 on the exact 128 x 128 form: m and n multiples of
 * 128, k a multiple of 16, under the calling thread's tuning keys; anything
 * else is refused with QS_ERR_BAD_EXTENT before a launch (no fallback).  The
 * dispatch record names the launch
 * "qs::gemm_fast_kernel<...>(qs::FastPairsMirrorArgs)".  (An addition: the ABI
 * version stays 4.)
 */
int qs_matmul_pairs_mirrored(int dtype, const void* A, const void* B, void* out,
                             int64_t m, int64_t n, int64_t k,
                             int64_t lda, int64_t ldb, int64_t ldc,
                             int64_t grid_n, int64_t stride_a, int64_t stride_b,
                             int64_t stride_c, int accumulate, void* stream);

/*
 * qs_matmul_pairs whose A entries are square (m == k == lda, at least m * m
 * elements apart) and stored, at ALL grid_n * grid_n flat indices, on their
 * 16 x 16 blocks (G, J >= G) only, with A(i, j) == A(j, i)^T.  For every pair
 * (i, j >= i) the launch reads these blocks and nothing else of A:
 *   of entry (i, j): the blocks (G, J >= G);
 *   of entry (j, i): the blocks (J, G) with J < G, each standing for block
 *                    (G, J) of entry (i, j) transposed.
 * The k order is that of qs_matmul_pairs, so on a complete A whose diagonal
 * blocks are symmetric between (i, j) and (j, i) the result has its bits.
 * float64 on the exact tiled forms only: m a multiple of 64, n of 128,
 * 16-byte aligned operands with even strides, accumulate == 0, under the
 * calling thread's tuning keys; anything else is refused with
 * QS_ERR_BAD_EXTENT before a launch (no fallback).  The dispatch record names
 * the launch "qs::gemm_fast_kernel<false, 4|2, 4, true, false>(qs::FastPairsLowerArgs)".
 * (An addition: the ABI version stays 4.)
 */
int qs_matmul_pairs_lower(int dtype, const void* A, const void* B, void* out,
                          int64_t m, int64_t n, int64_t k,
                          int64_t lda, int64_t ldb, int64_t ldc,
                          int64_t grid_n, int64_t stride_a, int64_t stride_b,
                          int64_t stride_c, int accumulate, void* stream);

/*
 * The product on a COLUMN TRIANGLE: the n = stack * side * side columns of B
 * and out are a stack of row-major side x side matrices (c, d), and only the
 * column blocks that meet d >= c are computed.  A tile's 128 columns are R
 * rows c of S contiguous columns d (S = 16 and R = 8; the tuning key
 * "gemm_upper_s" = 32 gives S = 32 and R = 4), and a tile exists iff its last
 * column >= its first row: 272 of the 512 tiles of a 256 x 256 matrix.
 * Elements with d < c inside such a block are computed and stored (correct
 * values); nothing else of B is read and nothing else of out is written.
 *   out[t] (m x n) = A[t] (m x k) . B[t] (k x n)   on those blocks, t < batch
 * float64 only, on the exact forms of the tiled kernel: k a multiple of 16, m
 * of 64, side of S, accumulate == 0 (the argument is there for the shape of
 * qs_matmul's list; a nonzero value is refused); anything else is refused with
 * QS_ERR_BAD_EXTENT (complex128 included) before a launch -- no fallback.  The
 * dispatch record names the launch
 * "qs::gemm_fast_kernel<false, 4, 4, true, false>(qs::FastUpperArgs)" (m a
 * multiple of 128) or "<false, 2, 4, true, false>".  Every computed element
 * has the bits qs_matmul gives it.  (An addition: the ABI version stays 4.)
 */
int qs_matmul_upper(int dtype, const void* A, const void* B, void* out,
                    int64_t m, int64_t side, int64_t stack, int64_t k,
                    int64_t lda, int64_t ldb, int64_t ldc,
                    int64_t batch, int64_t stride_a, int64_t stride_b,
                    int64_t stride_c, int accumulate, void* stream);

/*
 * Host only: pair number t (0 <= t < n (n + 1) / 2) of that order -> (*i, *j),
 * by the same remap the kernels use.  QS_ERR_BAD_EXTENT for n <= 0 or t out
 * of range.
 */
int qs_triangle_pair(int64_t n, int64_t t, int64_t* i, int64_t* j);

/*
 * Bytes of workspace qs_transform_two_body needs for u:(L,L,L,L) -> (M,M,M,M).
 * Returns a negative QS_ERR_* on bad extents.
 */
int64_t qs_transform_two_body_workspace(int dtype, int64_t L, int64_t M);

/*
 * Four-index transform
 *   out[p,q,r,s] = sum_abcd Ct[p,a] Ct[q,b] u[a,b,c,d] C[c,r] C[d,s]
 * evaluated as the reference does, one index at a time in the order d, c, b, a.
 *   u   : (L,L,L,L)   C : (L,M)   Ct : (M,L)   out : (M,M,M,M)
 * `u` is not modified; `out` must not alias `u` or the workspace.
 * Replaces BasisSet.transform_two_body_elements, basis_set.py:336-350.
 */
int qs_transform_two_body(int dtype, const void* u, const void* C,
                          const void* Ct, void* out, void* work,
                          int64_t work_bytes, int64_t L, int64_t M,
                          void* stream);

/*
 * The same transform for a REAL fp64 tensor against complex128 coefficients
 * (NumPy's promotion at basis_set.py:341-342; the per-step call of a
 * time-dependent solver on a real quantum-dot `u`, system.py:222-225):
 *   u_f64 (L,L,L,L) fp64;  C (L,M), Ct (M,L), out (M,M,M,M) complex128.
 * No complex copy of `u` is made: the d contraction reads the real tensor
 * (8 bytes per element) and runs on the real matrix instruction against C seen
 * as an (L, 2M) real matrix -- half the MFMA work of the promoted product --
 * and the c, b, a contractions are complex.  Workspace:
 * qs_transform_two_body_workspace(QS_C128, L, M).
 */
int qs_transform_two_body_mixed(const void* u_f64, const void* C, const void* Ct,
                                void* out, void* work, int64_t work_bytes,
                                int64_t L, int64_t M, void* stream);

/*
 * The same transform IN PLACE, for a caller that drops the old tensor anyway
 * (BasisSet.change_basis rebinds self.u, basis_set.py:374-377): `u` (L,L,L,L) is
 * overwritten and the result (M,M,M,M), M <= L, is left at the START of its
 * storage.  Peak memory is the tensor plus ONE L^3 M spare buffer instead of
 * tensor + workspace + result: the four contractions ping-pong between the two.
 * Same arithmetic, same order; l = 256 fp64 needs 69 GB instead of 103 GB, and
 * the largest fp64 basis one MI355X holds grows from 320 to ~360 orbitals.
 */
int64_t qs_transform_two_body_inplace_workspace(int dtype, int64_t L, int64_t M);
int qs_transform_two_body_inplace(int dtype, void* u, const void* C,
                                  const void* Ct, void* work, int64_t work_bytes,
                                  int64_t L, int64_t M, void* stream);

/*
 * The transform of a tensor with PARTICLE-EXCHANGE SYMMETRY,
 *   u[a,b,c,d] == u[b,a,d,c]  bit for bit
 * (random_basis.py:52; every physical two-body tensor has it).  Both leading
 * indices meet Ct and both trailing ones C, so every intermediate that treats
 * the members of a pair alike keeps the symmetry: the d and c contractions run
 * on the pairs b >= a only, the last product on q >= the block of p, and a
 * byte-moving mirror writes the other half -- about 2.9 products' worth of
 * matrix work instead of 4.  The symmetry has no conjugation in it and Ct may
 * be any matrix.  (No ABI version change: these are additions.)  Where the
 * tuning key "exchange_order" (below) says so, the leading indices are
 * contracted first instead: a on all of u, the b product on q >= the block of
 * p, d and c on the pairs q >= p -- the same matrix work, and one mirror, of
 * the result, where the other order has one of an intermediate as well.
 *
 *   qs_two_body_exchange_symmetric: 1 if u (L,L,L,L) has the symmetry, 0 if
 *     not, negative QS_ERR_* on error.  Bit patterns are compared: -0.0 against
 *     +0.0 is "not symmetric", equal NaNs are symmetric.  `scratch`: 4 bytes
 *     of device memory.  THIS CALL BLOCKS: it launches the check on `stream`,
 *     copies the verdict back and synchronises the stream -- the only blocking
 *     call of the transform path.  A non-symmetric tensor costs microseconds
 *     (the grid stops reading once a difference is known), a symmetric one
 *     one pass over u.  On a capturing stream it launches nothing and
 *     returns 0.  The verdict is not cached anywhere.
 *   qs_transform_two_body_exchange / qs_transform_two_body_inplace_exchange:
 *     arguments, workspace, aliasing rules and asynchrony of
 *     qs_transform_two_body / qs_transform_two_body_inplace.  PRECONDITION: u
 *     has the symmetry (otherwise the result is that of the symmetrised half
 *     that was read, not an error).  Results agree with the plain entries to
 *     rounding, not bit for bit (the a contraction runs before the b one).
 *   qs_transform_two_body_exchange_wanted: 1 where this route is the faster
 *     one for (dtype, L, M) under the calling thread's tuning keys, else 0;
 *     never for min(L, M) <= 128.
 *   qs_exchange_mirror: in place on t (n,n,m,m),
 *     t[a,b,r,s] = t[b,a,s,r] for every pair with a / block > b / block
 *     (block = 1: the lower triangle a > b); nothing else is written.
 *   qs_transform_two_body_exchange_leading_pairs: 1 where the exchange entries
 *     would contract the leading indices of (dtype, L, M) on pairs under the
 *     calling thread's tuning keys ("exchange_order", "exchange_leading"),
 *     else 0.  Launches nothing.
 *   qs_exchange_pair_transpose / qs_exchange_pair_transpose_back: the two byte
 *     movers of "exchange_leading" = 2 (below), exact copies of bits.  The
 *     first, both tensors (L,L,L,L): dst[c,d,a,b] = src[a,b,c,d] for the pairs
 *     d >= c; nothing is written at d < c.  The second, src (L,L,M,M) stored on
 *     the pairs d >= c only (never read at d < c), dst (M,M,L,L):
 *     dst[p,q,c,d] = src[c,d,p,q] where d >= c, src[d,c,q,p] where d < c, for
 *     the pairs q >= p; nothing is written at q < p.  L, M <= 4096 and a grid
 *     below 2^31 workgroups (else QS_ERR_BAD_EXTENT); src and dst must not
 *     overlap (QS_ERR_ALIAS).
 *   qs_transform_two_body_exchange_leading_upper: 1 where the exchange entries
 *     would contract the leading indices of (dtype, L, M) as two
 *     qs_matmul_upper products and one qs_exchange_mirror_lower under the
 *     calling thread's tuning keys ("exchange_order", "exchange_upper",
 *     "exchange_leading"), else 0; qs_transform_two_body_exchange_leading_pairs
 *     answers 0 wherever this answers 1.  Launches nothing.
 *   qs_transform_two_body_exchange_lower_d: 1 where that form would drop its
 *     qs_exchange_mirror_lower and run the d contraction as one
 *     qs_matmul_pairs_lower instead ("exchange_lower", and the keys above),
 *     else 0.  Launches nothing.
 *   qs_exchange_mirror_lower: in place on t (n,n,m,m), float64,
 *     t[i,j][r,s] = t[j,i][s,r] for every pair i <= j (the diagonal pairs
 *     included) and every s < r; nothing else is written.  The fill after the
 *     two products of "exchange_upper".
 */
int qs_two_body_exchange_symmetric(int dtype, const void* u, int64_t L,
                                   void* scratch, void* stream);
int qs_transform_two_body_exchange(int dtype, const void* u, const void* C,
                                   const void* Ct, void* out, void* work,
                                   int64_t work_bytes, int64_t L, int64_t M,
                                   void* stream);
int qs_transform_two_body_inplace_exchange(int dtype, void* u, const void* C,
                                           const void* Ct, void* work,
                                           int64_t work_bytes, int64_t L,
                                           int64_t M, void* stream);
int qs_transform_two_body_exchange_wanted(int dtype, int64_t L, int64_t M);
int qs_exchange_mirror(int dtype, void* t, int64_t n, int64_t m, int64_t block,
                       void* stream);
int qs_transform_two_body_exchange_leading_pairs(int dtype, int64_t L, int64_t M);
int qs_transform_two_body_exchange_leading_upper(int dtype, int64_t L, int64_t M);
int qs_transform_two_body_exchange_lower_d(int dtype, int64_t L, int64_t M);
int qs_exchange_mirror_lower(int dtype, void* t, int64_t n, int64_t m,
                             void* stream);
int qs_exchange_pair_transpose(int dtype, const void* src, void* dst, int64_t L,
                               void* stream);
int qs_exchange_pair_transpose_back(int dtype, const void* src, void* dst,
                                    int64_t L, int64_t M, void* stream);

/*
 * Same transform restricted to rows [a_lo, a_hi) of the leading index of `u`
 * for the contractions over d, c, b only:
 *   v[a,q,r,s] = sum_bcd Ct[q,b] u[a,b,c,d] C[c,r] C[d,s],  a in [a_lo,a_hi)
 *   u_slab : (a_hi-a_lo, L, L, L)     v_slab : (a_hi-a_lo, M, M, M)
 * The slab-local half of the sharded transform; the contraction
 * over `a` is a plain qs_matmul on the exchanged slabs.
 */
int64_t qs_transform_two_body_partial_workspace(int dtype, int64_t L, int64_t M,
                                                int64_t rows);
int qs_transform_two_body_partial(int dtype, const void* u_slab, const void* C,
                                  const void* Ct, void* v_slab, void* work,
                                  int64_t work_bytes, int64_t L, int64_t M,
                                  int64_t rows, void* stream);

/*
 * One-body transform of a stack of matrices:  out[i] = Ct . (h[i] . C)
 *   h : (nmat, L, L)   out : (nmat, M, M)   work : nmat*L*M elements
 * Replaces BasisSet.transform_one_body_elements, basis_set.py:329-334, as
 * applied to h, s, position[i], momentum[i] (:358-406).
 */
int qs_transform_one_body(int dtype, const void* h, const void* C,
                          const void* Ct, void* out, void* work,
                          int64_t work_bytes, int64_t nmat, int64_t L,
                          int64_t M, void* stream);

/*
 * Anti-symmetrisation  out[p,q,r,s] = u[p,q,r,s] - u[p,q,s,r]
 *   u, out : (npq, l, l) with npq = number of leading (p,q) pairs handled
 *            (l*l for a full tensor, fewer for a p-slab).
 * `out` may equal `u` (in place).  Exact (one subtraction per element).
 * Replaces BasisSet.anti_symmetrize_u, basis_set.py:776-778.
 */
int qs_antisymmetrize(int dtype, const void* u, void* out, int64_t npq,
                      int64_t l, void* stream);

/*
 * Spin doubling of the two-body tensor, optionally fused with the
 * anti-symmetrisation and the cast to complex128, for spatial rows
 * p in [p_lo, p_hi):
 *   out[2p+s1, 2q+s2, 2r+s3, 2s+s4] =
 *        d(s1,s3) d(s2,s4) u[p,q,r,s]  - antisym * d(s1,s4) d(s2,s3) u[p,q,s,r]
 *   u   : (l,l,l,l) of in_dtype (full tensor, indexed by absolute p)
 *   out : (2*(p_hi-p_lo), 2l, 2l, 2l) of out_dtype (slab, first row = 2*p_lo)
 * in_dtype QS_F64 may be combined with out_dtype QS_C128 (imaginary part 0).
 * Replaces add_spin_two_body (basis_set.py:772-774) + anti_symmetrize_u
 * (:776-778) + cast_to_complex (:298-319) inside
 * change_to_general_orbital_basis (:530-636).
 */
int qs_spin_expand_two_body(int in_dtype, int out_dtype, const void* u,
                            void* out, int64_t l, int64_t p_lo, int64_t p_hi,
                            int antisymmetrize, void* stream);

/*
 * The same expansion for a BLOCK of the tensor, the form the sharded layouts
 * use (no rank holds the whole tensor):
 *   u   : (np, nq, l, l)  = u[p0:p0+np, q0:q0+nq, :, :], contiguous
 *   out : (2 np, 2 nq, 2l, 2l) = out[2 p0 : 2(p0+np), 2 q0 : 2(q0+nq), :, :]
 * np = rows of a leading-index slab with nq = l, or np = l with nq = the rows
 * of a second-index slab.  Slab-local: output element (2p+s1, 2q+s2, ., .)
 * needs input matrix (p, q) only.
 */
int qs_spin_expand_two_body_block(int in_dtype, int out_dtype, const void* u,
                                  void* out, int64_t l, int64_t np, int64_t nq,
                                  int antisymmetrize, void* stream);

/*
 * kron(h, I2) for a stack of matrices: out[i, 2p+s, 2q+t] = d(s,t) h[i,p,q]
 *   h : (nmat, l, l) in_dtype     out : (nmat, 2l, 2l) out_dtype
 * Replaces BasisSet.add_spin_one_body, basis_set.py:768-770.
 */
int qs_add_spin_one_body(int in_dtype, int out_dtype, const void* h, void* out,
                         int64_t nmat, int64_t l, void* stream);

/*
 * Two-body part of S^2:
 *   out[p,q,r,s] = sum_i S_i[p,r] S_i[q,s]  - antisym * S_i[p,s] S_i[q,r]
 *   S : (3, n, n) complex128 (spin_x, spin_y, spin_z), out : rows
 *   p in [p_lo, p_hi) of the (n,n,n,n) complex128 tensor.
 * Replaces the einsum("pr,qs->pqrs") accumulation of
 * setup_spin_squared_operator, basis_set.py:745-747 (+ :525-526).
 */
int qs_spin_squared_two_body(const void* S, void* out, int64_t n, int64_t p_lo,
                             int64_t p_hi, int antisymmetrize, void* stream);

/*
 * Coulomb matrix elements of the two-dimensional harmonic oscillator (quantum
 * dot) in the Fock-Darwin basis, omega = 1:
 *   out[p - p_lo, q, r, s] = <pq|u|rs>,  p in [p_lo, p_hi),  out : fp64
 * orbitals ordered by shell as two_dim_helper.py:111-166 (index p <-> (n, m)).
 * Replaces _get_coulomb_elements, quantum_dots/two_dim/two_dim_helper.py:250-268
 * and coulomb_ho, quantum_dots/two_dim/coulomb_elements.py:6-92 (the input
 * generator of TwoDimensionalHarmonicOscillator, two_dim_ho.py:84-95).
 */
int qs_tdho_coulomb_elements(void* out, int64_t l, int64_t p_lo, int64_t p_hi,
                             void* stream);

/*
 * The same elements for an explicit orbital table: nm_table is a device array
 * of 2*l int32, n of every orbital followed by m of every orbital; max_shell =
 * max(2 n + |m| + 1) over the table (the caller knows it; the log-factorial
 * tables cover max_shell <= 30).  Replaces get_coulomb_elements_B,
 * two_dim_helper.py:284-301 (orbitals ordered by their energy in a magnetic
 * field, TwoDimHarmonicOscB, two_dim_ho.py:213-276).
 */
int qs_tdho_coulomb_elements_nm(void* out, const void* nm_table, int64_t l,
                                int64_t max_shell, int64_t p_lo, int64_t p_hi,
                                void* stream);

/*
 * ---- several GPUs of one node: one process per GPU, RCCL over xGMI ------------
 * (the reference itself knows one device only.)
 *
 * qs_comm_unique_id: 128 bytes that identify a communicator; ONE rank calls it,
 *   the host distributes the bytes to the other ranks by its own means (MPI
 *   broadcast, a file, a socket) -- exactly ncclGetUniqueId's contract.
 * qs_comm_init: collective over the `world` ranks; binds the communicator to
 *   the calling thread's current device and creates the stream the exchange
 *   runs on.  The handle is the only persistent object the library owns.
 * qs_comm_destroy: frees it.  qs_last_comm_error: text of the calling thread's
 *   most recent QS_ERR_COMM.
 * RCCL is loaded at run time (librccl.so.1; the copy already in the process
 * when there is one): single-GPU users have no link-time dependency on it.
 * (Development / test hook: the environment variable QS_AMD_RCCL_LIB names a
 * library to load instead -- the test suite's file-based stand-in, which lets
 * several ranks share one GPU.)
 */
#define QS_UNIQUE_ID_BYTES 128
int qs_comm_unique_id(void* id /* QS_UNIQUE_ID_BYTES */);
int qs_comm_init(void** comm, int rank, int world, const void* unique_id);
int qs_comm_destroy(void* comm);
/* Tear down without waiting for outstanding operations (ncclCommAbort): the
 * only thing left to do after a sharded call returned an error in the middle
 * of its exchange (the handle then refuses further work: peers may be blocked
 * in a group this rank never completed) or when a peer died. */
int qs_comm_abort(void* comm);
int qs_comm_rank(void* comm);
int qs_comm_world(void* comm);
const char* qs_last_comm_error(void);
/* Per-handle options (every rank of the communicator must choose the same):
 *   "rows_coalesce" = 1: qs_transform_two_body_sharded_rows exchanges ONE
 *     message per peer and step -- the peer's block of the send buffer as it
 *     is; the received block goes through a staging area at the end of the
 *     workspace and is put in place by one strided copy on the communicator's
 *     stream -- instead of one message per peer and result row that lands in
 *     place (0, the default).  Same results bit for bit; trades
 *     jl (world - 1) chunk_rows M^2 elements of workspace and one extra pass
 *     over the received rows for (world - 1) instead of jl (world - 1)
 *     messages per step and direction.
 * Unknown key: QS_ERR_BAD_EXTENT. */
int qs_comm_set_option(void* comm, const char* key, int64_t value);

/*
 * STATUS of the sharded entry points below: EXPERIMENTAL.  On REAL RCCL they
 * have run with ONE rank only (the development boxes hold one GPU).  Their
 * multi-rank branches are executed by tests/test_gpu_mock_rccl_ranks.py: 2-5
 * rank processes on one GPU, every ncclSend / ncclRecv the library posts
 * carried by a file-based stand-in for librccl (tests/cabi/mock_rccl.cpp: same
 * pairing and size rules, no asynchrony), results bit-identical to the
 * single-GPU transform, and by tests/test_gpu_async_transport.py: the ranks as
 * THREADS of one process over a stream-ordered, asynchronous stand-in
 * (tests/cabi/mock_rccl_async.cpp: ncclGroupEnd returns before anything has
 * moved, every transfer is a device copy behind events of both sides, with an
 * optional delay), which fails -- and is tested to fail -- when any one of
 * the stream waits between the caller's stream and the communicator's stream
 * is left out; in addition worlds of 1..8 ranks are covered by CPU
 * replays of the exchange plans (qs_sharded_exchange_plan,
 * qs_sharded_rows_exchange_plan) and by the same algorithms driven through
 * torch.distributed in the Python layer.  Unrun until an 8-GPU node: RCCL's own
 * transport and the overlap of the two streams.
 *
 * Four-index transform of a tensor sharded over the ranks of `comm`:
 *   u_bslab   : u[:, b_lo:b_hi, :, :]  (L, bl, L, L), this rank's share of the
 *               SECOND index; balanced split: the first L % world ranks hold
 *               L / world + 1 rows (same rule for the result)
 *   out_pslab : out[p_lo:p_hi]  (pc, M, M, M), this rank's share of the LEADING
 *               index of the result
 *   C (L, M), Ct (M, L) replicated on every rank.
 * d, c and a are contracted on the slab, ONE exchange re-shards
 * [p, b_loc] -> [p_loc, b] -- (world-1)/world^2 of the tensor leaves every rank,
 * as grouped ncclSend / ncclRecv pairs so that every peer's xGMI link carries
 * its share at once -- and the contraction over b closes on the received rows.
 * The exchange is issued in `nchunks` pieces (1..16; <= 0 selects 4) on the
 * communicator's stream and overlaps the products on `stream`; on return,
 * `stream` is ordered behind all of it.  Replaces transform_two_body_elements
 * (basis_set.py:336-350) for a tensor that one device does not hold;
 * collective: every rank of `comm` must call it with the same L, M, nchunks.
 */
int64_t qs_transform_two_body_sharded_workspace(int dtype, int64_t L, int64_t M,
                                                int world, int rank);
int qs_transform_two_body_sharded(void* comm, int dtype, const void* u_bslab,
                                  const void* C, const void* Ct, void* out_pslab,
                                  void* work, int64_t work_bytes, int64_t L,
                                  int64_t M, int nchunks, void* stream);

/*
 * The exchange plan of qs_transform_two_body_sharded for one rank, as numbers
 * (pure index arithmetic: no GPU, no RCCL).  Test hook: the CPU suite replays
 * the plans of all ranks of a world with NumPy and checks that every row ends
 * up where the closing product reads it.
 *   header  : {b_lo, bl, p_lo, pc, row_x, row_r, nchunks}
 *   ct_rows : M entries, the row of Ct multiplied in slot i of X
 *   chunks  : nchunks x {first slot, slots, first result row (relative), result rows}
 *   table   : one row {chunk, peer, kind, x_off, r_off, count, rows} per
 *             operation, kind 0 send / 1 receive / 2 own rows (X -> R)
 * Returns the number of operations (<= table_rows) or a negative QS_ERR_*.
 */
int qs_sharded_exchange_plan(int64_t L, int64_t M, int world, int rank,
                             int nchunks, int64_t* header, int64_t* ct_rows,
                             int64_t* chunks, int64_t* table, int64_t table_rows);

/*
 * The memory-lean sharded transform: rows of ONE leading index in, rows of the
 * OTHER one out, everything else O(chunk_rows * l^3).  Replaces
 * transform_two_body_elements (basis_set.py:336-350) for the per-step call on
 * a resident sharded `u` (system.py:222-225) and inside change_basis
 * (basis_set.py:374-382) when two slabs are all a GPU can hold (l = 512
 * complex128 on 8 GPUs: 128 GiB in + 128 GiB out per rank).
 *   rows       : (il, L, L, L) of `in_dtype` -- rows[i][j] = u[i_lo + i, j]
 *                for a leading-index sharding, u[j, i_lo + i] for a
 *                second-index sharding (the transform is symmetric under
 *                swapping its two leading index pairs, so one routine serves
 *                both); `in_starts` (world + 1 offsets, 0 ... L) gives every
 *                rank's first row, NULL = the balanced split.  in_dtype
 *                QS_F64 with dtype QS_C128 is the mixed product above.
 *   out_buffer : qs_transform_two_body_sharded_rows_out_bytes(); on return its
 *                first jl * M^3 elements are out[j'_loc][i'][r][s], this
 *                rank's rows j' (balanced split of M) of the other
 *                transformed leading index.  The rest of the buffer held the
 *                received rows: the closing contraction runs row by row
 *                inside it, no second slab.
 *   chunk_rows : input rows per exchange step (<= 0: qs_sharded_rows_default_chunk,
 *                at least four steps within a fixed scratch budget).  Per step
 *                d, c and the contraction over the whole leading index run on
 *                `stream`; the grouped ncclSend / ncclRecv of the step (one
 *                contiguous message per peer and result row, landing in
 *                place) run on the communicator's stream under the next
 *                step's products.
 * Collective: every rank passes the same L, M, chunk_rows, in_starts.
 */
int64_t qs_sharded_rows_default_chunk(int dtype, int64_t L, int64_t M, int world,
                                      const int64_t* in_starts);
int64_t qs_transform_two_body_sharded_rows_out_bytes(int dtype, int64_t L, int64_t M,
                                                     int world, int rank);
int64_t qs_transform_two_body_sharded_rows_workspace(int dtype, int64_t L, int64_t M,
                                                     int64_t chunk_rows);
/* The same for THIS handle: adds the staging area when the handle's option
 * "rows_coalesce" is set (this is the size the call checks work_bytes against). */
int64_t qs_comm_rows_workspace(void* comm, int dtype, int64_t L, int64_t M,
                               int64_t chunk_rows);
int qs_transform_two_body_sharded_rows(void* comm, int in_dtype, int dtype,
                                       const void* rows, const int64_t* in_starts,
                                       const void* C, const void* Ct,
                                       void* out_buffer, int64_t out_bytes,
                                       void* work, int64_t work_bytes, int64_t L,
                                       int64_t M, int64_t chunk_rows, void* stream);
/* Its exchange plan for one rank as numbers (test hook, no GPU, no RCCL):
 *   header : {i_start, il, jl, il_max, r0, out_elems, chunk_rows, nsteps}
 *   table  : {step, peer, kind, w_off, buf_off, count, rows} per operation,
 *            kind 0 send (offset into the step's send block W[j'][i][(r,s)]),
 *            1 receive (offset into out_buffer), 2 own rows (W -> out_buffer,
 *            `rows` pieces of `count` elements, pitches n*M*M and L*M*M).
 * Returns the number of operations (<= table_rows) or a negative QS_ERR_*. */
int qs_sharded_rows_exchange_plan(int64_t L, int64_t M, int world, int rank,
                                  const int64_t* in_starts, int64_t chunk_rows,
                                  int64_t* header, int64_t* table, int64_t table_rows);
/* ... of the coalesced exchange ("rows_coalesce"): kind 0 send (one per peer:
 * the peer's whole block of W), 3 receive into the staging area (buf_off =
 * offset into it), 4 staging -> out_buffer behind the group (w_off = offset
 * into the staging area, `rows` pieces of `count` elements, pitches count and
 * L*M*M), 2 own rows as above. */
int qs_sharded_rows_exchange_plan_coalesced(int64_t L, int64_t M, int world, int rank,
                                            const int64_t* in_starts, int64_t chunk_rows,
                                            int64_t* header, int64_t* table,
                                            int64_t table_rows);

/*
 * Which kernels the calling thread's most recent compute entry point launched,
 * as the names rocprofv3 prints for them, ';'-separated, repeated launches of
 * one instantiation folded to "name xN" (static thread-local storage; empty
 * before the first call).  bench.py puts this string into its `roofline.kernel`
 * field so that a bench line names the kernel that actually ran.
 */
const char* qs_last_dispatch(void);

/*
 * Auxiliary entry points (no reference counterpart).  NOT part of the product
 * path: tuning runs, tests and bench probes only.
 *   qs_tuning_set / qs_tuning_reset: override a kernel choice FOR THE CALLING
 *     THREAD (thread-local state: the library has no process-global mutable
 *     state; every thread starts from the automatic policy and
 *     qs_tuning_reset() returns the calling thread to it).  Keys
 *     "gemm_f64_cfg", "gemm_c128_cfg" (tile shape of the general
 *     kernel, 0 = automatic), "gemm_pipe" (1 = rotated K-loop schedule, 0 = plain),
 *     "gemm_fast" (0 = general kernel only, 1 = automatic, 2 = exact form of
 *     the VALU-free kernel only, 3 = its edge form wherever it is legal), "gemm_fast_shape" (edge-form tile
 *     shape 1..4, 0 = automatic), "gemm_fast_persist"
 *     (0 one workgroup per tile, 1 automatic, 2 always persistent, >= 3 tiles
 *     per workgroup),
 *     "gemm_skinny" (0 = never use the streaming short-and-wide kernel),
 *     "gemm_stream" (0 = never use the small-coefficient streaming kernel,
 *     2 = never split the rows of A over two waves), "slab_pair" (0 = never fuse
 *     the d and c contractions of a small-basis transform into one pass, 2 = one
 *     wave per slab always), "sandwich" (the two fused passes of a small-basis
 *     transform on the 4-wide fp64 matrix instruction: 0 = off, 1 = both,
 *     2 = the (d, c) pass only, 3 = the (b, a) pass only; 4 / 5 / 6 = both /
 *     (d, c) only / (b, a) only wherever the kernel is legal, not only where it
 *     measures faster), "sandwich_mode"
 *     (work split of those passes: -1 automatic, 0 one item quad per workgroup,
 *     1 four adjacent quads per workgroup, 3 the same with a barrier per step),
 *     "sandwich_t2" (the intermediate between those passes stored transposed,
 *     (r, s, a, b), so that the second pass fetches slabs too: -1 automatic,
 *     0 never, 1 always), "sandwich_v2" (the balanced form of those passes:
 *     -1 automatic, 0 never, 1 wherever it exists, 2 also odd quad counts on
 *     the next even instantiation), "sandwich_tail" (0 = never split the item
 *     quads of a partly filled last round over all workgroups), "small4"
 *     (the whole-quad kernel of up to 32 orbitals: 0 never, 1 automatic,
 *     2 wherever it exists), "quad4s" (the streamed fp64 kernel of 5-64
 *     orbitals: 0 never, 1 automatic, 2 wherever it exists), "pair4c" (the
 *     streamed complex128 / real-tensor-complex-coefficients kernel of 5-64
 *     orbitals: 0 never, 1 automatic, 2 wherever it exists), "gemm_fit"
 *     (fitted tile shapes of the general kernel: 0 never, 1 automatic, 2 always),
 *     "gemm_pick" (0 = tile shape by padded area only), "gemm_strip" (the strip
 *     kernels, which cover the small extent of a product with one tile to the
 *     next multiple of 16: 0 never, 1 by estimated time, 2 wherever they
 *     exist), "gemm_strip_w" (tuning runs: their relative rate in percent,
 *     0 = built-in weights), "gemm_strip_wide" (their 256-wide form: 0 =
 *     automatic, where the tile list fills the chip a few times over, 1 = never,
 *     2 = wherever it exists, fp64 up to 10 blocks of 16; any other value is
 *     refused with QS_ERR_BAD_EXTENT), "gemm_strip_wgs" (the most workgroups of
 *     a strip launch: 0 = one per CU, 1 ... 4096 = at most that many, each
 *     walking more tiles; any other value is refused with QS_ERR_BAD_EXTENT;
 *     the result does not depend on either key),
 *     "gemm_stream_wgs" (the most workgroups of a launch of the
 *     small-coefficient streaming product: 0 = as many as stay resident,
 *     1 ... 4096 = at most that many, each wave walking more column blocks;
 *     any other value is refused with QS_ERR_BAD_EXTENT; the result does not
 *     depend on it),
 *     "gemm_fast_unaligned" (0 = 8-byte global items at
 *     odd strides as in rounds 1-3, 1 = 16-byte items at any 8-byte-aligned
 *     address), "comm_drop_wait" (TEST HOOK of the sharded entry points: a bit
 *     mask of stream waits between the caller's stream and the communicator's
 *     to leave out -- the negative control of the asynchronous stand-in
 *     transport, tests/test_gpu_async_transport.py; never set it elsewhere),
 *     "lead_rows_max" (qs_transform_two_body_blocks: the most leading rows M0
 *     whose step a takes the streaming kernel of qs_lead_contract, 0 ... 32;
 *     a value outside that range is refused with QS_ERR_BAD_EXTENT),
 *     "pair_contract_g" (qs_pair_contract, qs_pair_contract_antisym and
 *     qs_pair_contract_exchange: vectors per load of U, 0 = the shipped group size of the dtype pair, 1, 2, 4 or 8
 *     for tuning runs),
 *     "det_ci_g" (qs_det_ci_sigma: vectors per walk of a determinant's
 *     excitations, 0 = shipped, 1, 2, 4 or 8 for tuning runs),
 *     "string_ci_bytes" (qs_string_ci_group: the byte budget of the D and G
 *     panels of one qs_string_ci_sigma call, 0 = the caller's shipped value;
 *     a negative value is refused with QS_ERR_BAD_EXTENT),
 *     "triples_bytes" (qs_triples_energy_budget: the byte budget of the blocks
 *     of one pass of the triples correction, 0 = the caller's shipped value;
 *     a negative value is refused with QS_ERR_BAD_EXTENT),
 *     "exchange" (qs_transform_two_body_exchange_wanted: 0 = never, 1 = where
 *     the exchange route measured faster, 2 = wherever it exists, any size),
 *     "exchange_block" / "exchange_block_d" (rows per block of that route's
 *     closing product and mirror / of its d contraction, 0 = automatic),
 *     "exchange_pairs" (1 = that route's c contraction, and its d contraction
 *     where that pads no more, as one qs_matmul_pairs launch; 0 = one launch
 *     per row / per block of rows, the same bits),
 *     "exchange_order" (that route's order of the contractions: 0 = d and c
 *     on the pairs b >= a of u, a mirror, a, the closing blocks, a mirror;
 *     2 = a, the closing blocks, d and c on the pairs q >= p of the result's
 *     grid, one mirror; 1, the default = 2 where M >= L and L is at least the
 *     smallest size measured to gain, never below the route's own thresholds,
 *     else 0.  The two orders agree to rounding, not bit for bit; a value
 *     outside 0 ... 2 is refused with QS_ERR_BAD_EXTENT),
 *     "exchange_leading" (how order 2 contracts the leading indices: 0 = a as
 *     one product and the closing blocks; 2 = on pairs: u's trailing indices
 *     have the symmetry too, u[:,:,c,d] == u[:,:,d,c]^T, so the pair matrix is
 *     turned (qs_exchange_pair_transpose), b and a run as two products over
 *     the pairs d >= c of u's grid, and qs_exchange_pair_transpose_back turns
 *     the result and fills in the other half -- 1.0 instead of 1.625 products'
 *     worth of matrix work, plus two passes over half a tensor.  Its
 *     intermediates need M >= L: for M < L, and where a mover's grid would
 *     not fit, 2 gives the very launches of 0.  1, the default = 2 from the
 *     smallest size measured to gain, never below the route's own
 *     thresholds, else 0.  b runs before a: 0 and 2 agree to rounding, not
 *     bit for bit; outside 0 ... 2: QS_ERR_BAD_EXTENT),
 *     "exchange_upper" (order 2's leading indices with the triangle on the
 *     COLUMNS of the products instead of on their batch: b and a as two
 *     qs_matmul_upper products on the column blocks d >= c of u's trailing
 *     indices, for all leading indices, then qs_exchange_mirror_lower fills
 *     the triangles d < c of the pairs q >= p -- 1.06 products' worth of
 *     matrix work and one pass over a quarter of a tensor, no pair movers;
 *     also for M < L and in place.  float64 only.  0 = never; 2 = wherever
 *     qs_matmul_upper takes both products (L a multiple of 16, M of 64);
 *     1, the default = 2 where M >= L from the smallest size measured to gain
 *     (192 orbitals, the route's own threshold), and only while
 *     "exchange_leading" is at its own default: an explicit 0 or 2 there keeps
 *     exactly those launches.  Agrees with the other forms to rounding;
 *     outside 0 ... 2: QS_ERR_BAD_EXTENT),
 *     "exchange_lower" (that column-triangle form WITHOUT its fill: the d
 *     launch over the pairs q >= p, the fill's one reader, runs as
 *     qs_matmul_pairs_lower and takes each 16 x 16 block below the block
 *     diagonal from the mirror pair, where the second product stored it; the
 *     blocks below the diagonal of the intermediate are then never written,
 *     and in place they hold stale input that nothing reads.  float64 only.
 *     0 = never; 2 = wherever "exchange_upper" runs and qs_matmul_pairs_lower
 *     takes that launch (L a multiple of 64, M of 128), elsewhere the launches
 *     with the fill; 1, the default = 2 from the smallest size measured to
 *     gain (256 orbitals), and only while "exchange_upper" is at its own
 *     default: an explicit 2 there keeps exactly its launches, the fill
 *     included.  Agrees with the filled form to rounding (its bits except on
 *     the diagonal blocks, whose lower elements no longer come from their
 *     mirror images); outside 0 ... 2: QS_ERR_BAD_EXTENT),
 *     "gemm_upper_s" (the segment length S of qs_matmul_upper's tiles: 16 or
 *     32, 0 = the shipped choice, 16; anything else: QS_ERR_BAD_EXTENT).
 *   qs_probe_mfma_f64: register-resident fp64 MFMA loop, `blocks` workgroups
 *     of 4 waves, each wave issuing iters*8 v_mfma_f64_16x16x4_f64
 *     (flops = blocks*4*iters*8*2048); `sink` is a device scratch of
 *     8 + 16*blocks bytes: after the dummy first word, per block the deltas of
 *     the shader clock and of the 100 MHz counter around the loop (their ratio
 *     x 100 MHz is the clock the chip holds under pure MFMA load).
 *   qs_probe_stream_copy: 16-byte-per-lane device copy (moves 2*bytes).
 * bench.py uses the probes to print measured ceilings beside datasheet ones.
 */
int qs_tuning_set(const char* key, int64_t value);
int qs_tuning_reset(void);

/*
 * Mean-field (Fock) contraction of the two-body tensor with a one-body density,
 * both sums from ONE read of `u`:
 *   W[p,q] = cj * sum_{r,s} u[p,r,q,s] D[s,r]  +  ck * sum_{r,s} u[p,r,s,q] D[s,r]
 *   u_slab : (P, R, L, L) contiguous -- rows p_lo ... p_lo+P of the leading index
 *            and r_lo ... r_lo+R of the second (the whole tensor, u[lo:hi] and
 *            u[:, lo:hi] made contiguous are all this one call); with R < L the
 *            result is the partial sum over the slab's r;
 *   D      : (L, L) row-major, D[s, r];   W : (P, L).
 * dtype pairs (u, D): (F64, F64) -> W fp64; (C128, C128) -> W complex128;
 * (F64, C128) -> W complex128 with no complex copy of `u`; (C128, F64) is
 * QS_ERR_BAD_DTYPE.  1 <= L <= 1024, 1 <= P <= L, 1 <= R, r_lo >= 0, r_lo + R <= L.
 * cj == 0 / ck == 0 skip that sum's arithmetic.  RHF: cj = 1, ck = -1/2 with the
 * spin-summed density; anti-symmetrised spin orbitals: cj = 1, ck = 0.
 * Replaces np.einsum("prqs,sr->pq") / ("prsq,sr->pq") on the whole tensor (the
 * reference names the step: change_to_hf_basis, general_orbital_system.py:161-169).
 * Deterministic (no floating-point atomics): the r range is cut into chunks of
 *   Rc = min(ceil(R / min(ceil(4096 / L), R)), max(1, floor(2048 / (Le * dw))))
 * consecutive r, Le = L rounded up to even, dw = 1 for an fp64 D and 2 for a
 * complex one; each (p, chunk) sum goes to the workspace and a second launch adds
 * the chunks in ascending order.  The split depends on (L, R, dtypes) only: row p
 * of a slab call is bit-identical to row p of the full call.
 * Workspace: P * L * ceil(R / Rc) elements of W's dtype (bytes per row times P);
 * nothing else is allocated or written.  `W` must not overlap `u_slab`, `D` or
 * the workspace.
 */
int64_t qs_mean_field_workspace(int u_dtype, int d_dtype, int64_t L, int64_t P, int64_t R);
int qs_mean_field(int u_dtype, int d_dtype, const void* u_slab, const void* D, void* W,
                  int64_t L, int64_t P, int64_t R, int64_t r_lo, double cj, double ck,
                  void* workspace, int64_t workspace_bytes, void* stream);
/* The launch geometry qs_mean_field uses for (dtypes, L, P, R), as numbers (pure
 * index arithmetic from the functions the entry itself calls: no GPU, no HIP
 * call).  Test hook: the suite derives the geometry classes its cases must
 * cover from it.  Writes 7 values to `out` (n_out >= 7):
 *   {Rc, nchunk, ct_log, ncb, nrb, lds_bytes, grid}
 * Rc consecutive r per work unit, nchunk = ceil(R / Rc) units per row; CT =
 * 1 << ct_log column threads of one 16-byte item (cpi = 2 real columns, or 1
 * complex element of u), RT = 256 / CT row threads of 8 rows: a tile is RB =
 * 8 RT rows by CT * cpi columns, a slab ncb x nrb tiles, a tile row WPR =
 * max(1, CT / 64) waves; lds_bytes = 8 * aw * (Rc * Le + nrb * RB + ncb * CT *
 * cpi + RB * WPR + 256 * cpi) dynamic LDS, aw = 1 for an fp64 D and 2 for a
 * complex one; grid = P * nchunk workgroups.  All but `grid` depend on (dtypes,
 * L, R) only.  Returns 0 or what qs_mean_field_workspace refuses (dtype pair,
 * extents; QS_ERR_BAD_EXTENT for n_out < 7, QS_ERR_NULL_POINTER for out == 0). */
int qs_mean_field_plan(int u_dtype, int d_dtype, int64_t L, int64_t P, int64_t R,
                       int64_t* out, int n_out);

/*
 * The same contraction for a BATCH of densities from one read of `u` per group
 * of G of them (csrc/qs_mean_field_batch.hip):
 *   W_k[p,q] = cj[k] * sum_{r,s} u[p,r,q,s] D_k[s,r] + ck[k] * sum_{r,s} u[p,r,s,q] D_k[s,r]
 *   u_slab : (P, R, L, L) as for qs_mean_field;  D : (ND, L, L);  W : (ND, P, L);
 *   cj, ck : HOST arrays of ND weights (read before the call returns).
 * dtype pairs, extents and r_lo as qs_mean_field; 1 <= ND <= 65536.  A zero
 * weight leaves its sum out of W_k.  ceil(ND / G) streaming launches and one
 * closing launch.  G is a property of the dtype pair (fp64 8; complex128 4;
 * real u with complex D 4), halved for the L at which the group's share of the
 * 64 KB of LDS -- one column of every density plus the unit's sums -- no longer
 * fits (qs_mean_field_batch_plan reports it).
 * Deterministic, and independent of the batch: the r range is cut into chunks of
 *   Rc = the largest rc <= ceil(R / min(ceil(4096 / L), R)) with
 *        (rc * Le + nrb * RB + ncb * CT * cpi) * G * aw <= 8192   (rc >= 1)
 * consecutive r (Le, aw, cpi, CT, RB, ncb, nrb: see qs_mean_field_batch_plan), a
 * function of (L, R, dtypes) only -- not of ND, of k, or of whether a group is
 * partial.  W_k has the same bits whether D_k is sent alone or anywhere in a
 * batch of any size, and row p of a slab call has the bits of row p of the full
 * call.  (Equality of bits with qs_mean_field is not promised.)
 * Workspace: ND * P * L * ceil(R / Rc) elements of W's dtype; nothing else is
 * allocated or written.  `W` must not overlap `u_slab`, `D` or the workspace.
 * Errors as qs_mean_field, checked in the same order before any HIP call;
 * ND < 1 is QS_ERR_BAD_EXTENT, a null weight array QS_ERR_NULL_POINTER.
 */
int64_t qs_mean_field_batch_workspace(int u_dtype, int d_dtype, int64_t L, int64_t P, int64_t R,
                                      int64_t ND);
int qs_mean_field_batch(int u_dtype, int d_dtype, const void* u_slab, const void* D, void* W,
                        int64_t L, int64_t P, int64_t R, int64_t r_lo, int64_t ND,
                        const double* cj, const double* ck, void* workspace,
                        int64_t workspace_bytes, void* stream);
/* The launch geometry qs_mean_field_batch uses, as numbers (host only, no HIP
 * call; test hook).  Writes 9 values to `out` (n_out >= 9):
 *   {G, passes, Rc, nchunk, ct_log, ncb, nrb, lds_bytes, grid}
 * G densities per load of u, passes = ceil(ND / G) streaming launches; CT =
 * 1 << ct_log column threads of one 16-byte item (cpi = 2 real columns or 1
 * complex element of u), RT = 256 / CT row threads of 4 rows: a tile is RB =
 * 4 RT rows by CT * cpi columns, a slab ncb x nrb tiles; lds_bytes = 8 * aw * G *
 * (Rc * Le + nrb * RB + ncb * CT * cpi) dynamic LDS of a full group, Le = L
 * rounded up to even, aw = 1 for an fp64 D and 2 for a complex one; grid =
 * P * nchunk workgroups per launch.  All but `passes` and `grid` depend on
 * (dtypes, L, R) only.  Returns 0 or what qs_mean_field_batch_workspace refuses
 * (QS_ERR_BAD_EXTENT for n_out < 9, QS_ERR_NULL_POINTER for out == 0). */
int qs_mean_field_batch_plan(int u_dtype, int d_dtype, int64_t L, int64_t P, int64_t R,
                             int64_t ND, int64_t* out, int n_out);

/*
 * Leading-index contraction with a few rows (csrc/qs_lead_contract.hip):
 *   T[i, x] = sum_a A[i, a] * B[a, x]      A (m, k) lda;  B (k, n) ldb;  T (m, n) ldt
 * for 1 <= m <= 32, any k >= 1 and any n >= 1 (odd included), row-major, leading
 * dimensions in elements (lda >= k, ldb >= n, ldt >= n).  dtype pairs (A, B):
 * (F64, F64) -> T fp64; (C128, C128) -> T complex128; (C128, F64) -> T
 * complex128 with B read as stored; a complex B with a real A is
 * QS_ERR_BAD_DTYPE.  One read of B, no workspace.  Every T[i, x] is ONE fused
 * multiply-add chain over ascending a: row i of an m-row call has the bits of
 * the 1-row call on that row, and column x depends neither on n, ldb nor on the
 * launch geometry.  Nothing outside B's (k - 1) * ldb + n elements is read.
 * `T` must not overlap `A` or `B`.
 */
int qs_lead_contract(int a_dtype, int b_dtype, const void* A, const void* B, void* T,
                     int64_t m, int64_t n, int64_t k, int64_t lda, int64_t ldb, int64_t ldt,
                     void* stream);

/*
 * Four-index transform with ONE coefficient matrix PER INDEX, to a block:
 *   out[p,q,r,s] = sum_abcd Ct0[p,a] Ct1[q,b] u[a,b,c,d] C2[c,r] C3[d,s]
 *   u (L,L,L,L);  Ct0 (M0,L), Ct1 (M1,L): bra rows;  C2 (L,M2), C3 (L,M3): ket
 *   columns;  out (M0,M1,M2,M3); all contiguous.
 * Contraction order a, b, d, c -- the LEADING index first, so every step works
 * on a tensor already shrunk by the blocks in front of it: put the small blocks
 * (the occupied orbitals of <ij|ab>) first; for a Hermitian u, <ab|ij> is the
 * conjugate of <ij|ab>.  Step a is qs_lead_contract (one read of u) when
 * M0 <= the tuning key "lead_rows_max" (0 ... 32, default 8), otherwise one
 * tiled product; b, d and c are batched products of the general dispatch.
 * dtype pairs (u, C) as qs_mean_field: (F64, F64); (C128, C128); (F64, C128) ->
 * complex128 out with u read as stored; (C128, F64) is QS_ERR_BAD_DTYPE.
 * 1 <= L <= 4096, 1 <= Mi <= L.
 * Workspace, in elements of the result dtype (Le = rounded up to even):
 *   Le(L * (M0 + M2)) + M0 * L^3 + M0 * M1 * L^2
 * = scratch for C2 transposed and the split rows of Ct0, the intermediate of
 * step a, and that of step b; the intermediate of step d (M0 * M1 * L * M3
 * elements) reuses the place of step a's, which it fits since M1 * M3 <= L^2.
 * `out` must not overlap any operand or the workspace, nor the workspace `u`.
 */
int64_t qs_transform_two_body_blocks_workspace(int u_dtype, int c_dtype, int64_t L,
                                               int64_t M0, int64_t M1, int64_t M2, int64_t M3);
int qs_transform_two_body_blocks(int u_dtype, int c_dtype, const void* u, const void* Ct0,
                                 const void* Ct1, const void* C2, const void* C3, void* out,
                                 void* work, int64_t work_bytes, int64_t L, int64_t M0,
                                 int64_t M1, int64_t M2, int64_t M3, void* stream);
/*
 * Contraction with a few vectors over the TRAILING index, one read of the matrix
 * per group of G vectors (csrc/qs_pair_contract.hip):
 *   S[k, x] = sum_y U[x * ldu + y] * T[k * Y + y]      (no conjugation)
 *   U : X rows of Y elements, row-major, ldu >= Y (elements);  T : (K, Y);  S : (K, X).
 * With U = u viewed as (l^2, l^2) this is S[k,p,q] = sum_rs u[p,q,r,s] T[k,r,s]:
 * the u-dependent part of the sigma vector of a two-particle full CI, and the
 * particle-particle ladder of coupled-cluster doubles on the untransformed tensor.
 * Replaces np.einsum("pqrs,krs->kpq") / np.tensordot(u, T, ((2, 3), (0, 1))).
 * dtype pairs (U, T): (F64, F64) -> S fp64; (C128, C128) -> S complex128;
 * (F64, C128) -> S complex128 with U read as stored (two real accumulations per
 * element, no complex copy of U); (C128, F64) is QS_ERR_BAD_DTYPE.
 * 1 <= X <= 2^32, 1 <= Y <= ldu <= 2^24 (odd Y and odd ldu included), 1 <= K <= 65536.
 * ceil(K / G) streaming launches and nothing else: a wave of 64 lanes walks along
 * four rows in steps of 64 16-byte items and closes each row sum once, so y is
 * never split and the workspace is 0 bytes (`work` may be NULL; the query stays in
 * the ABI for a geometry that would split y).  G is a property of the dtype pair
 * (fp64 8; complex128 8; real U with complex T 4), the tuning key
 * "pair_contract_g" (0 = shipped, 1, 2, 4, 8; anything else QS_ERR_BAD_EXTENT)
 * overrides it for the calling thread.  A partial last group runs on the smallest
 * instantiation that holds it.
 * Promises (tests/test_gpu_pair_contract.py):
 *   1. S[k] has the same bits alone and at any position in a batch of any K (and
 *      under any "pair_contract_g");
 *   2. row x has the same bits whatever X, whatever ldu and wherever the slab
 *      starts (8- or 16-byte-aligned base, rows cut out of a larger tensor): the
 *      lanes' shares of a row and the order of every sum depend on Y and the
 *      dtype pair only;
 *   3. repeating a call gives the same bits (no floating-point atomics);
 *   4. a non-finite value in row x of U reaches S[:, x] only, one in T[k] reaches
 *      S[k] only, and nothing outside U[0 : (X - 1) * ldu + Y) is read: the bytes
 *      between rows (ldu > Y) are fetched with the rows' items only where an item
 *      straddles a row's end, and then dropped by a select.
 * Errors, checked in this order before any HIP call: dtype pair, extents
 * (ldu < Y included), null U / T / S, misaligned pointer (element size), S
 * overlapping U or T (QS_ERR_ALIAS), work_elems below the query (negative).
 */
int64_t qs_pair_contract_workspace(int u_dtype, int t_dtype, int64_t X, int64_t Y, int64_t K);
int qs_pair_contract(int u_dtype, int t_dtype, const void* U, const void* T, void* S,
                     int64_t X, int64_t Y, int64_t K, int64_t ldu,
                     void* work, int64_t work_elems, void* stream);
/*
 * Pair contraction of an anti-symmetrised tensor with amplitudes anti-symmetric in
 * their pair, from the quarter of the tensor the two symmetries do not repeat
 * (csrc/qs_pair_contract_antisym.hip):
 *   S[k,p,q] = 2 * sum_{r<s} U[p,q,r,s] * T[k,r,s]   for p < q      (no conjugation)
 *   S[k,q,p] = -S[k,p,q],   S[k,p,p] = +0
 *   U : (l, l, l, l), consecutive (p, q) rows ldu >= l^2 elements apart;
 *   T : (K, l, l);  S : (K, l, l), written in full.
 * For U[p,q,r,s] = -U[q,p,r,s] = -U[p,q,s,r] and T[k] = -T[k]^T this is
 * np.einsum("pqrs,krs->kpq", U, T) from a quarter of the bytes: the particle-particle
 * ladder of coupled-cluster doubles on the untransformed tensor, the sigma vector of
 * two particles in spin orbitals.  The symmetries are taken on trust, not checked.
 * dtype pairs (U, T): (F64, F64) -> S fp64; (C128, C128) -> S complex128; every other
 * pair is QS_ERR_BAD_DTYPE (a real U against complex T is the fp64 form on the real
 * and the imaginary parts as 2 K amplitudes, which is exact).
 * 2 <= l <= 4096, l^2 <= ldu <= 2^24, 1 <= K <= 65536.  ceil(K / G) launches and nothing
 * else, workspace 0 bytes (`work` may be NULL); G = 8 in both forms, the tuning key
 * "pair_contract_g" overrides it as it does for qs_pair_contract.
 * Promises (tests/test_gpu_pair_contract_antisym.py):
 *   1. only U[p,q,r,s] with p < q and r < s and T[k,r,s] with r < s are read;
 *   2. S[k,q,p] is the negation of the very value stored at S[k,p,q];
 *   3. S[k] has the same bits alone and at any position in a batch of any K (and
 *      under any "pair_contract_g"): the order of every sum depends on l only;
 *   4. a non-finite value in a read element of row (p, q) of U reaches S[:, p, q] and
 *      S[:, q, p] only, one in T[k] reaches S[k] only.
 * Errors, checked in this order before any HIP call: dtype pair, extents (l < 2,
 * K < 1, ldu < l^2 included), null U / T / S, misaligned pointer (element size), S
 * overlapping U or T (QS_ERR_ALIAS), work_elems below the query (negative).
 */
int64_t qs_pair_contract_antisym_workspace(int u_dtype, int t_dtype, int64_t l, int64_t K);
int qs_pair_contract_antisym(int u_dtype, int t_dtype, const void* U, const void* T, void* S,
                             int64_t l, int64_t K, int64_t ldu,
                             void* work, int64_t work_elems, void* stream);
/*
 * Pair contraction of a tensor with particle-exchange symmetry with ANY amplitudes,
 * from the half of the tensor the symmetry does not repeat
 * (csrc/qs_pair_contract_exchange.hip):
 *   S[k,p,q] = sum_rs U[p,q,r,s] * T[k,r,s]   for all p, q      (no conjugation)
 *   U : (l, l, l, l), consecutive (p, q) rows ldu >= l^2 elements apart;
 *   T : (K, l, l);  S : (K, l, l), written in full.
 * For U[p,q,r,s] = U[q,p,s,r] (the two-body integrals of spatial orbitals: what
 * qs_two_body_exchange_symmetric checks) this is np.einsum("pqrs,krs->kpq", U, T)
 * from half of the bytes and half of the products: with a = U[p,q,r,s],
 * b = U[q,p,r,s] for p <= q, r <= s,
 *   S+-[p,q] = sum_{r<=s} w_rs (a +- b) (T[k,r,s] +- T[k,s,r]),  w_rs = 1/2 if r = s else 1
 *   S[k,p,q] = (S+ + S-) / 2,   S[k,q,p] = (S+ - S-) / 2.
 * The particle-particle ladder of closed-shell coupled-cluster doubles on the
 * untransformed tensor.  The symmetry is taken on trust, not checked.
 * dtype pairs (U, T): (F64, F64) -> S fp64; (C128, C128) -> S complex128; every other
 * pair is QS_ERR_BAD_DTYPE (a real U against complex T is the fp64 form on the real
 * and the imaginary parts as 2 K amplitudes, which is exact).
 * 1 <= l <= 4096, l^2 <= ldu <= 2^24, 1 <= K <= 65536.  ceil(K / G) launches and nothing
 * else, workspace 0 bytes (`work` may be NULL); G = 8 in both forms, the tuning key
 * "pair_contract_g" overrides it as it does for qs_pair_contract.
 * Promises (tests/test_gpu_pair_contract_exchange.py):
 *   1. only U[p,q,r,s] with r <= s is read; all of T[k] is read;
 *   2. S[k] has the same bits alone, at any position in a batch of any K, under any
 *      "pair_contract_g" and on repetition: the order of every sum depends on l only;
 *   3. if T[k] equals its transpose bit for bit, S[k,q,p] and S[k,p,q] have the same
 *      bits; if T[k] = -T[k]^T, they differ in the sign bit only;
 *   4. a non-finite value in a read element of row (p, q) of U reaches S[:, p, q] and
 *      S[:, q, p] only, one in T[k] reaches S[k] only.
 * Errors, checked in this order before any HIP call: dtype pair, extents (l < 1,
 * K < 1, ldu < l^2 included), null U / T / S, misaligned pointer (element size), S
 * overlapping U or T (QS_ERR_ALIAS), work_elems below the query (negative).
 */
int64_t qs_pair_contract_exchange_workspace(int u_dtype, int t_dtype, int64_t l, int64_t K);
int qs_pair_contract_exchange(int u_dtype, int t_dtype, const void* U, const void* T, void* S,
                              int64_t l, int64_t K, int64_t ldu,
                              void* work, int64_t work_elems, void* stream);
/*
 * Direct configuration interaction on Slater determinants (csrc/qs_det_ci.hip):
 *   H = sum_pq ht[p,q] a+_p a_q + 1/4 sum_pqrs ut[p,q,r,s] a+_p a+_q a_s a_r
 *   ht : (m, m) Hermitian;  ut : (m, m, m, m), ut[p,q,r,s] = <pq|rs> - <pq|sr>.
 * A determinant is a 64-bit occupation mask over 1 <= m <= 63 orthonormal spin
 * orbitals (bit p = orbital p occupied); the space is data: `dets` holds dim
 * ascending, duplicate-free masks of exactly N bits, none at or above m (the
 * full space, a spin sector, an excitation-truncated space, any subset).  A
 * connection whose target is not in `dets` contributes nothing: the matrix of a
 * subset is the projection of the full one.  The caller vouches for the list (a
 * bit at or above m is masked off before it indexes anything; an unsorted list
 * gives wrong numbers, never an access outside the arguments).
 *   qs_det_ci_diagonal : D[I] = <I|H|I>, dim doubles (real in both forms).
 *   qs_det_ci_sigma    : sigma[k * dim + I] = sum_J <I|H|J> c[J * ldc + k],
 *       k < K.  c is stored with the K values of one determinant adjacent
 *       (ldc >= K elements between determinants), sigma as K rows of dim.  D is
 *       the output of qs_det_ci_diagonal for the same ht, ut and dets.
 *       ceil(K / G) launches and nothing else: the thread that owns I walks its
 *       single and double excitations once per group of G vectors, looks each
 *       target up by binary search and feeds G running sums.  G is 8 in both
 *       forms; the tuning key "det_ci_g" (0 = shipped, 1, 2, 4, 8; anything
 *       else QS_ERR_BAD_EXTENT) overrides it for the calling thread.  A partial
 *       last group runs on the smallest instantiation that holds it.  The
 *       workspace is 0 bytes (`work` may be NULL).
 *   qs_det_ci_density1 : rho[q * m + p] = sum_IJ conj(c[I]) <I|a+_p a_q|J> c[J]
 *       for ONE vector c[dim]: one workgroup per (p, q), a fixed-order sum.
 *   qs_det_ci_transition_density1 :
 *       rho[q * m + p] = sum_IJ conj(bra[I]) <I|a+_p a_q|J> ket[J]
 *       for two vectors bra[dim], ket[dim] of one dtype: the same kernel, and
 *       with bra == ket (the same pointer is allowed) the bits of
 *       qs_det_ci_density1.
 *   qs_det_ci_density2 :
 *       gamma2[((p*m + q)*m + r)*m + s]
 *           = sum_IJ conj(bra[I]) <I|a+_p a+_q a_s a_r|J> ket[J],
 *       m^4 elements, every one written by the call: the output is zeroed on
 *       the stream (elements with p = q or r = s; everything at N = 1), then
 *       one workgroup per unique (p < q, r < s), C(m,2)^2 of them, strides over
 *       dets, closes its sum in a fixed order and writes the four copies
 *       gamma2[pqrs] = -gamma2[qprs] = -gamma2[pqsr] = gamma2[qpsr] (exact
 *       anti-symmetry, no atomics, repeatable bits).  With this index order
 *       <bra|H|ket> = sum_pq ht[p,q] rho[q,p]
 *                     + 1/4 sum_pqrs ut[p,q,r,s] gamma2[p,q,r,s].
 *       A target outside `dets` contributes nothing: a subset gives the
 *       densities of the projected problem.
 * dtype pairs (ht and ut, c): (F64, F64) and (C128, C128); any other pair is
 * QS_ERR_BAD_DTYPE.  The diagonal takes the dtype of ht / ut, the densities that
 * of c or of bra and ket (rho and gamma2 have it too).
 * Promises (tests/test_gpu_det_ci.py):
 *   1. sigma[k] has the same bits alone, at any position in a batch of any K and
 *      under any "det_ci_g"; repeating a call gives the same bits (no atomics,
 *      every product an explicit fma, a sum order fixed by I and dets);
 *   2. nothing outside sigma[0 : K * dim), D[0 : dim), rho[0 : m * m) is written,
 *      whatever dim is relative to the workgroup of 64 determinants.
 * Errors, checked in this order before any HIP call: dtype pair, extents (m
 * outside 1 ... 63, N outside 1 ... m, dim < 1 or > 2^31 - 1, K < 1, ldc < K),
 * null pointer, misaligned pointer (element size; 8 for dets and D), an output
 * overlapping an input (QS_ERR_ALIAS; rho and gamma2 against dets, bra and ket),
 * work_elems below the query (negative).
 */
int64_t qs_det_ci_workspace(int h_dtype, int c_dtype, int64_t m, int64_t N, int64_t dim, int64_t K);
int qs_det_ci_diagonal(int h_dtype, const void* ht, const void* ut, const int64_t* dets, double* D,
                       int64_t m, int64_t N, int64_t dim, void* stream);
int qs_det_ci_sigma(int h_dtype, int c_dtype, const void* ht, const void* ut, const int64_t* dets,
                    const double* D, const void* c, void* sigma, int64_t m, int64_t N, int64_t dim,
                    int64_t K, int64_t ldc, void* work, int64_t work_elems, void* stream);
int qs_det_ci_density1(int c_dtype, const int64_t* dets, const void* c, void* rho,
                       int64_t m, int64_t N, int64_t dim, void* stream);
int qs_det_ci_transition_density1(int c_dtype, const int64_t* dets, const void* bra, const void* ket,
                                  void* rho, int64_t m, int64_t N, int64_t dim, void* stream);
int qs_det_ci_density2(int c_dtype, const int64_t* dets, const void* bra, const void* ket,
                       void* gamma2, int64_t m, int64_t N, int64_t dim, void* stream);
/*
 * Spin-free configuration interaction on alpha and beta occupation strings
 * (Knowles-Handy; csrc/qs_string_ci.hip), for SPATIAL orbitals:
 *   H = sum_pr k[p,r] E_pr + sum_(pr),(qs) W[(pr),(qs)] E_pr E_qs,
 *   E_pq = sum_spin a+_p,spin a_q,spin,
 *   k[p,r] = ht[p,r] - 1/2 sum_q ut[p,q,q,r],
 *   W[(pr),(qs)] = 1/2 ut[p,q,r,s]       (m^2 x m^2, row p*m + r, column q*m + s)
 * with ht (m, m) and ut (m, m, m, m) = <pq|rs>, NOT anti-symmetrised.  A state
 * is c[Ia * nb + Ib] over a list of na alpha and a list of nb beta strings:
 * ascending, duplicate-free 64-bit masks over 1 <= m <= 63 spatial orbitals with
 * Na and Nb bits; the determinant is all alpha creators first, ascending within
 * each spin.  The lists are data: a replacement whose target string is missing
 * contributes nothing.
 *   qs_string_ci_table : T[K * m*m + p*m + q] (int32) of one list of n strings:
 *       +-(index of J + 1) where <K|E_pq|J> = +-1 -- J = K - p + q, p in K, q not
 *       in K or q = p, sign (-1)^(bits of K strictly between p and q) --, 0 where
 *       the replacement is empty or J is not in the list.  One table per spin;
 *       equal lists may share one (ta == tb is allowed below).
 *   qs_string_ci_diagonal : D[Ia * nb + Ib] = <I|H|I>, na * nb doubles, from ht
 *       and ut (real parts), n_p = n_p,alpha + n_p,beta:
 *       sum_p n_p ht[p,p] + 1/2 sum_pq n_p n_q ut[p,q,p,q]
 *                         - 1/2 sum_pq (n_pa n_qa + n_pb n_qb) ut[p,q,q,p].
 *   qs_string_ci_sigma : sigma[k, Ia, Ib] = (H c_k)[Ia, Ib] for the K vectors of
 *       c, (K, na, nb) contiguous in and out, in three steps without atomics:
 *         expand : D[(qs), k, :] = E_qs c_k              (m^2 x K na nb, work)
 *         product: G = W . D                             (the dispatcher of qs_matmul)
 *         fold   : sigma_k = sum_pr E_pr (G[(pr), k, :] + k[p,r] c_k)
 *       The fold's sum has a fixed order (pr ascending, alpha before beta, explicit
 *       fmas): repeating a call gives the same bits.  Bit-equality of sigma_k
 *       between DIFFERENT K (alone, in a batch, in another group) is NOT promised:
 *       the product dispatcher chooses its kernel by the extents.
 *   qs_string_ci_workspace : bytes of `work` for K vectors,
 *         2 * ceil16(m^2 * K * na * nb * sizeof(element of c)),
 *       D then G.  qs_string_ci_density1 needs D only, for one vector: the query
 *       with K = 1 is sufficient for it (half of it is what it checks).
 *   qs_string_ci_group : the number of vectors, 1 ... K, to send per
 *       qs_string_ci_sigma call so that its workspace stays within budget_bytes
 *       (the calling thread's tuning key "string_ci_bytes" when that is set; 2 GiB
 *       when both are 0) and its product within 2^31 - 1 columns; at least 1.
 *       A positive tuning key takes precedence over budget_bytes: it is the
 *       override of a tuning run, not a default.
 *   qs_string_ci_sigma_rows : the same sigma in passes over alpha rows of the
 *       INTERMEDIATE, for vectors whose D and G do not fit a byte budget.  A pass
 *       owns the alpha rows r0 <= Ka < r1, R = r1 - r0:
 *         expand : D_p[(qs), k, Ka - r0, Kb] = (E_qs c_k)[Ka, Kb]   (m^2 x K R nb)
 *         product: G_p = W . D_p
 *         fold   : sigma_k[Ia, Ib] (+)= the terms of the fold above whose source
 *                  row (Ta[Ia,pr] for alpha, Ia for beta) lies in the pass
 *       c stays whole; the passes follow one another on the stream and add into
 *       sigma, the first one from 0: sigma need not be initialised, every element
 *       is written.  No atomics; the order of one element's sum is pass ascending,
 *       pr ascending, alpha before beta: repeating a call gives the same bits, and
 *       a call of one pass gives the bits of qs_string_ci_sigma.  budget_bytes as
 *       in qs_string_ci_group (tuning key, else the argument, else 2 GiB);
 *       budget_bytes < 0 is QS_ERR_BAD_EXTENT.  work holds plan[3] bytes.
 *   qs_string_ci_sigma_plan : plan[0 ... 3] = alpha rows per pass, passes, columns
 *       of one (full) pass's product, workspace bytes.  rows is the largest count
 *       with 2 * ceil16(m^2 * K * rows * nb * sizeof(element of c)) <= budget and
 *       K rows nb (twice that for (F64, C128)) <= 2^31 - 1, at least 1; then
 *       passes = ceil(na / rows) and rows = ceil(na / passes), so that the passes
 *       are of equal length where that costs no extra pass.  The workspace is
 *       2 * ceil16(m^2 * K * rows * nb * sizeof(element of c)) of the final rows.
 *   qs_string_ci_sigma_sym : sigma of vectors of definite parity under the exchange
 *       of the two spins, c_k[Ia, Ib] = parity * c_k[Ib, Ia] (parity = +-1), for
 *       na = nb = n strings and ONE table t for both spins.  In this determinant
 *       convention an eigenstate of spin S has parity (-1)^S.  Every row of D, G
 *       and X = G + k c then has the same parity in (Ka, Kb), and only the columns
 *       Kb <= Ka are formed: packed row Ka at off(Ka) = Ka (Ka + 1) / 2.  Always in
 *       passes over packed rows r0 <= Ka < r1, L = off(r1) - off(r0):
 *         expand : D_p[(qs), k, off(Ka) - off(r0) + Kb] = (E_qs c_k)[Ka, Kb]
 *         product: G_p = W . D_p                          (m^2 x K L, the dispatcher)
 *         fold   : S_k[Ia, Ib] (+)= the stored terms of the fold whose source row
 *                  lies in the pass, a diagonal element of X weighted 1/2
 *         close  : sigma_k = S_k + parity * S_k^T, in place, after the last pass
 *       c and sigma are full (K, n, n).  sigma need not be initialised.  The
 *       result has the parity bit for bit: sigma[a,b] == parity * sigma[b,a], the
 *       diagonal +0.0 for parity = -1; repeating a call gives the same bits.  The
 *       precondition on c is NOT checked: for another c the result is
 *       deterministic and unspecified.  budget_bytes as in qs_string_ci_sigma_rows;
 *       parity other than +-1 or budget_bytes < 0 is QS_ERR_BAD_EXTENT.  work
 *       holds plan[3] bytes, D_p then G_p.
 *   qs_string_ci_sigma_sym_plan : plan[0 ... 3] = passes, the largest packed length
 *       L, the columns of the largest product (K L, twice that for (F64, C128)),
 *       workspace bytes 2 * ceil16(m^2 * K * L * sizeof(element of c)).  The
 *       boundaries are greedy from b_0 = 0: b_i+1 is the largest r <= n with
 *       2 * ceil16(m^2 * K * (off(r) - off(b_i)) * sizeof(element)) <= budget, at
 *       least b_i + 1.  bounds may be null; otherwise it receives the passes + 1
 *       boundaries, and bounds_len < passes + 1 is QS_ERR_BAD_EXTENT.
 *   qs_string_ci_density1 : rho[q * m + p] = <bra| E_pq |ket>
 *       = sum_K conj(bra[K]) (E_pq ket)[K], spin-summed, one expand of ket and one
 *       fixed-order sum per (p, q); bra == ket (the same pointer is allowed) is a
 *       state's density.
 *   qs_string_ci_density2 : the spin-summed two-body density
 *         gamma[((p*m + q)*m + r)*m + s] = sum_spins <bra| a+_p a+_q a_s a_r |ket>
 *                                        = X[(pr),(qs)] - delta_qr <bra| E_ps |ket>,
 *         X[(pr),(qs)] = <bra| E_pr E_qs |ket>
 *                      = sum_K conj((E_rp bra)[K]) (E_qs ket)[K],
 *       and rho[q * m + p] = <bra| E_pq |ket> from the same pass; fp64 and
 *       complex128, bra == ket (the same pointer is allowed) is a state.  X is a
 *       Gram product of two expanded panels over the determinants, in passes over
 *       alpha rows so that both panels fit a byte budget: the tuning key
 *       "string_ci_bytes" when it is positive, else budget_bytes, else 2 GiB; at
 *       least one alpha row per pass.  A pass is ONE batched product over T slices
 *       of kc determinants (split-k) that adds into T partial results; a closing
 *       kernel sums them in ascending t.  No atomics: a repeated call gives the
 *       same bits; another budget agrees to rounding.  With the plain ut
 *       <bra|H|ket> = sum ht[p,q] rho[q,p] + 1/2 sum ut[p,q,r,s] gamma[p,q,r,s].
 *   qs_string_ci_density2_plan : plan[0 ... 4] = alpha rows per pass, passes,
 *       slices T, slice length kc, workspace bytes; T kc >= rows nb > (T - 1) kc.
 *   qs_string_ci_density2_workspace : bytes of `work` under that budget,
 *         T (m^2 + 1) m^2 e + (2 m^2 + 1) T kc e,   e = sizeof(element of c):
 *       the partial results, the bra panel (m^2 + 1 rows: conj(bra) is the last)
 *       and the ket panel.  The budget bounds the panels (or is the panels of one
 *       alpha row when it is smaller); the partial results come on top and stay
 *       below an eighth of the panels wherever T > 1.
 *   qs_string_ci_density2_spin : the spin-resolved densities of the same pair,
 *       with E^s_pq = a+_ps a_qs on the strings of one spin (s, t = alpha, beta):
 *         gamma_st[((p*m + q)*m + r)*m + s] = <bra| a+_ps a+_qt a_st a_rs |ket>
 *                       = X^st[(pr),(qs)] - delta_st delta_qr <bra| E^s_ps |ket>,
 *         X^st[(pr),(qs)] = sum_K conj((E^s_rp bra)[K]) (E^t_qs ket)[K],
 *         rho_s[q * m + p] = <bra| E^s_pq |ket>
 *       for st = aa, ab, bb; the beta-alpha block is gamma_ab[q,p,s,r] and is never
 *       formed.  gamma_aa + gamma_bb + gamma_ab + gamma_ba and rho_a + rho_b are the
 *       results of qs_string_ci_density2, and with the plain ut  <bra|H|ket> =
 *       sum ht[p,q] (rho_a + rho_b)[q,p]
 *       + 1/2 sum ut[p,q,r,s] (gamma_aa + gamma_bb + 2 gamma_ab)[p,q,r,s].
 *       Passes, budget, slices and close as in qs_string_ci_density2, on panels
 *       that keep the two replacements apart: with h = m^2 (fp64: rounded up to
 *       even, the pad column zero) the ket panel is (K, 2 h) = E^a_qs ket | E^b_qs
 *       ket, the bra panel (2 m^2 + 1, K) = conj(E^a_pq bra); conj(bra);
 *       conj(E^b_pq bra).  Per pass two batched products over the T slices: rows
 *       0 ... m^2 against all columns into part1[t] (m^2 + 1, 2 h), and the beta
 *       rows against the beta columns into part2[t] (m^2, h).  Na = 0 or Nb = 0
 *       (the list [0], a table of zeros) gives zero blocks.  No atomics: a repeated
 *       call gives the same bits; another budget agrees to rounding.
 *   qs_string_ci_density2_spin_plan : plan[0 ... 4] = alpha rows per pass, passes,
 *       slices T, slice length kc, workspace bytes; T kc >= rows nb > (T - 1) kc.
 *   qs_string_ci_density2_spin_workspace : bytes of `work` under that budget,
 *         T ((m^2 + 1) 2 h + m^2 h) e + (2 m^2 + 1 + 2 h) T kc e:
 *       part1, part2, the bra panel and the ket panel.  The budget bounds the
 *       panels (or is the panels of one alpha row when it is smaller); the partial
 *       results stay below an eighth of the panels wherever T > 1.
 *   qs_string_ci_spin_squared : out[k] = S^2 c[k] for c (K, na, nb),
 *         S^2 = S_z (S_z + 1) + N_beta - sum_pq E^alpha_qp E^beta_pq,
 *         S_z = (Na - Nb) / 2,
 *       one gather through both tables per (p, q) in a fixed order; no workspace.
 *       On a truncated list a missing target contributes nothing: like H, S^2 is
 *       then the operator of the truncated formulation.
 *   qs_string_ci_one_body : d one-body operators on K vectors, no workspace and no
 *       intermediate:
 *         out[x, k, Ia, Ib] = sum_pq ( A_up[x,p,q]   sgn c_k[Ta[Ia,pq], Ib]
 *                                    + A_down[x,p,q] sgn c_k[Ia, Tb[Ib,pq]] )
 *       for A_up, A_down (d, m, m) row-major, c (K, na, nb) and out (d, K, na, nb).
 *       A_down == NULL means A_down = A_up: the spin-free sum_pq A[p,q] E_pq.  One
 *       gather through the tables per (p, q) serves a group of up to 4 operators;
 *       the order of one element's sum is pq ascending, alpha before beta, every
 *       term an fma: a repeated call gives the same bits.  dtype pairs (A; c) as
 *       for sigma.  d < 1, d K na nb elements past int64 bytes, or a grid
 *       ceil(d / 4) K na ceil(nb / threads) past 2^31 - 1 is QS_ERR_BAD_EXTENT;
 *       out may share no byte with c, A_up, A_down or a table (QS_ERR_ALIAS).
 *   qs_string_ci_ladder_table : the ladder table L (n_t, m) int32 between two
 *       ascending, duplicate-free lists of ONE spin,
 *         L[J, p] = +-(index in source of target[J] ^ bit p, plus 1),
 *       sign (-1)^(bits of target[J] below p), the sign of a_p and of a+_p on a
 *       string; 0 where that mask is not in source.  With source one particle
 *       richer than target it is the table of annihilation (out of source, into
 *       target), with source one particle poorer that of creation.  Errors in this
 *       order: m outside 1 ... 63 or a list length refused as above, null
 *       pointer, alignment, table sharing a byte with a list.
 *   qs_string_ci_ladder : d combinations of ladder operators of one spin on K
 *       vectors, sum_p phi[x,p] a_p or sum_p phi[x,p] a+_p as the table says:
 *         spin 0: out[x,k,Ja,Jb] = sum_p phi[x,p] sgn(L[Ja,p]) c_k[|L[Ja,p]| - 1, Jb]
 *         spin 1: out[x,k,Ja,Jb] = (-1)^n_alpha
 *                                  sum_p phi[x,p] sgn(L[Jb,p]) c_k[Ja, |L[Jb,p]| - 1]
 *       for phi (d, m) (not conjugated), c (K, na_s, nb_s) on the source lists and
 *       out (d, K, na_t, nb_t) on the target lists, (na_t, nb_t) = (n_t, nb_s) for
 *       spin 0 and (na_s, n_t) for spin 1; the determinant is all alpha creators
 *       first, so a beta ladder passes n_alpha alpha particles.  No workspace, no
 *       intermediate; p ascending, every term one fma, zero coefficients skipped:
 *       a repeated call, a vector alone or in a batch and an operator alone or in
 *       a group give the same bits.  dtype pairs (phi; c) as for sigma.  Errors in
 *       this order: dtype pair; extents (those of sigma on the source and on the
 *       target lists, d < 1, spin not 0 or 1, n_alpha outside 0 ... m, the bytes
 *       of out past int64, a grid ceil(d / 4) K na_t ceil(nb_t / threads) past
 *       2^31 - 1); null pointer; alignment; out sharing a byte with c, phi or L.
 * dtype pairs (ht, ut, k, W; c): (F64, F64), (C128, C128) and (F64, C128), which
 * runs the product in fp64 on the re / im pairs of D as 2 K na nb columns (no
 * complex copy of W); (C128, F64) is QS_ERR_BAD_DTYPE.
 * Errors, checked in this order before any HIP call: dtype (pair), extents (m
 * outside 1 ... 63, Na or Nb outside 0 ... m, a list of < 1 or >= 2^31 - 1
 * strings, K < 1, more than 2^31 - 1 columns K na nb -- 2 K na nb for (F64,
 * C128) -- in one call), null pointer, misaligned pointer (element size; 8 for
 * strings and D, 4 for tables, 16 for work), work_bytes too small
 * (QS_ERR_WORKSPACE), an output overlapping an input or the workspace, or the
 * workspace overlapping an input (QS_ERR_ALIAS).  A table entry that points past its list is read as 0.
 */
int qs_string_ci_table(const int64_t* strings, int64_t n, int64_t m, int64_t N, int32_t* table, void* stream);
int qs_string_ci_diagonal(int h_dtype, const void* ht, const void* ut, const int64_t* sa, int64_t na, int64_t Na,
                          const int64_t* sb, int64_t nb, int64_t Nb, int64_t m, double* D, void* stream);
int64_t qs_string_ci_workspace(int h_dtype, int c_dtype, int64_t m, int64_t na, int64_t nb, int64_t K);
int64_t qs_string_ci_group(int h_dtype, int c_dtype, int64_t m, int64_t na, int64_t nb, int64_t K, int64_t budget_bytes);
int qs_string_ci_sigma(int h_dtype, int c_dtype, const void* k, const void* W, const int32_t* ta, const int32_t* tb,
                       int64_t m, int64_t na, int64_t nb, const void* c, int64_t K, void* sigma,
                       void* work, int64_t work_bytes, void* stream);
int qs_string_ci_sigma_plan(int h_dtype, int c_dtype, int64_t m, int64_t na, int64_t nb, int64_t K, int64_t budget_bytes,
                            int64_t* plan);
int qs_string_ci_sigma_rows(int h_dtype, int c_dtype, const void* k, const void* W, const int32_t* ta, const int32_t* tb,
                            int64_t m, int64_t na, int64_t nb, const void* c, int64_t K, void* sigma,
                            void* work, int64_t work_bytes, int64_t budget_bytes, void* stream);
int qs_string_ci_sigma_sym_plan(int h_dtype, int c_dtype, int64_t m, int64_t n, int64_t K, int64_t budget_bytes,
                                int64_t* plan, int64_t* bounds, int64_t bounds_len);
int qs_string_ci_sigma_sym(int h_dtype, int c_dtype, const void* k, const void* W, const int32_t* t, int64_t m, int64_t n,
                           int64_t parity, const void* c, int64_t K, void* sigma, void* work, int64_t work_bytes,
                           int64_t budget_bytes, void* stream);
int qs_string_ci_density1(int c_dtype, const int32_t* ta, const int32_t* tb, int64_t m, int64_t na, int64_t nb,
                          const void* bra, const void* ket, void* rho, void* work, int64_t work_bytes, void* stream);
int64_t qs_string_ci_density2_workspace(int c_dtype, int64_t m, int64_t na, int64_t nb, int64_t budget_bytes);
int qs_string_ci_density2_plan(int c_dtype, int64_t m, int64_t na, int64_t nb, int64_t budget_bytes, int64_t* plan);
int qs_string_ci_density2(int c_dtype, const int32_t* ta, const int32_t* tb, int64_t m, int64_t na, int64_t nb,
                          const void* bra, const void* ket, void* gamma, void* rho, void* work, int64_t work_bytes,
                          int64_t budget_bytes, void* stream);
int64_t qs_string_ci_density2_spin_workspace(int c_dtype, int64_t m, int64_t na, int64_t nb, int64_t budget_bytes);
int qs_string_ci_density2_spin_plan(int c_dtype, int64_t m, int64_t na, int64_t nb, int64_t budget_bytes, int64_t* plan);
int qs_string_ci_density2_spin(int c_dtype, const int32_t* ta, const int32_t* tb, int64_t m, int64_t na, int64_t nb,
                               const void* bra, const void* ket, void* gamma_aa, void* gamma_ab, void* gamma_bb, void* rho_a,
                               void* rho_b, void* work, int64_t work_bytes, int64_t budget_bytes, void* stream);
int qs_string_ci_spin_squared(int c_dtype, const int32_t* ta, const int32_t* tb, int64_t m, int64_t na, int64_t nb,
                              int64_t Na, int64_t Nb, const void* c, int64_t K, void* out, void* stream);
int qs_string_ci_one_body(int h_dtype, int c_dtype, const void* A_up, const void* A_down, int64_t d, const int32_t* ta,
                          const int32_t* tb, int64_t m, int64_t na, int64_t nb, const void* c, int64_t K, void* out,
                          void* stream);
int qs_string_ci_ladder_table(const int64_t* target, int64_t n_t, const int64_t* source, int64_t n_s, int64_t m, int32_t* table,
                              void* stream);
int qs_string_ci_ladder(int h_dtype, int c_dtype, const void* phi, int64_t d, int64_t spin, const int32_t* table, int64_t m,
                        int64_t n_alpha, int64_t na_s, int64_t nb_s, int64_t n_t, const void* c, int64_t K, void* out,
                        void* stream);
/*
 * Pivoted Cholesky decomposition of the two-body tensor (csrc/qs_cholesky.hip).
 * With G[(r,p),(q,s)] = u[p,q,r,s], an m^2 x m^2 matrix (flat index first * m +
 * second) that is Hermitian positive semidefinite for a positive interaction and a
 * plain, NOT anti-symmetrised u (m, m, m, m), the vectors L_x (m x m) satisfy
 *   u[p,q,r,s] = sum_x conj(L_x[r,p]) L_x[q,s]  + R,   0 <= R[(i),(i)] <= tau:
 * the residual R is positive semidefinite, so every element of it is bounded by
 * its largest diagonal element.  For the Coulomb tensor of a quantum dot the rank
 * is about 4 m, not m^2.  u is read in place (the pivot column of (q*, s*) is the
 * conjugated row u[s*, r, q*, p], contiguous in p); no m^4 copy is made.
 * Left-looking, one vector per step:
 *   piv = argmax d (the LOWEST flat index on ties);  stop when d[piv] <= tau or
 *   the capacity is reached;
 *   L_j[i] = (u[s*, r, q*, p] - sum_{x<j} L_x[i] conj(L_x[piv])) / sqrt(d[piv]),
 *   i = r m + p;   d[i] -= |L_j[i]|^2;   d[piv] = 0 exactly.
 * Hermiticity of G is the caller's contract and is not checked; an indefinite
 * tensor shows as a negative residual diagonal (extremes[1]).
 *   vectors  : (capacity, m, m) of dtype, device; rows 0 ... rank - 1 are L_x
 *   rank     : HOST pointer, in and out.  In: the vectors already in the buffer
 *              (0 = a fresh run, which fills diag from u).  Out: the vectors
 *              there now.  A call with rank > 0 CONTINUES the run that left
 *              vectors, diag and pivots: a caller whose run ended on the capacity
 *              copies the rows into a larger buffer and calls again.  Every sum
 *              has a fixed order that depends on neither the capacity nor the
 *              interruption: a resumed run, a fresh run and a repeated run give
 *              the same bits.
 *   diag     : m^2 doubles, device: the residual diagonal d[(r,p)], in and out
 *   pivots   : capacity int64, device: the flat index (q*, s*) of every step
 *   extremes : HOST pointer, 2 doubles out: the largest and the smallest residual
 *              diagonal at exit (largest <= tau: converged; smallest < 0 beyond
 *              rounding: G is not positive semidefinite).  A NaN anywhere on
 *              the residual diagonal ends the run at the next pivot: *rank is
 *              the number of steps completed and extremes[0] is NaN -- a
 *              caller must not read "not > tau" as converged
 *   work     : qs_cholesky_two_body_workspace bytes, device, 16-byte aligned
 * Two plain launches per step, in stream order (no grid-wide barrier, no spin
 * wait): the pivot, the rank and a stop flag stay in device memory and every
 * launch after the stop returns at once.  THIS CALL BLOCKS: it enqueues
 * qs_cholesky_two_body_block() steps at a time and reads the state back once
 * after each such block (hipMemcpyAsync + hipStreamSynchronize on `stream`); on
 * a capturing stream it launches nothing and returns QS_ERR_HIP.
 * Errors, checked in this order before any HIP call: dtype; extents (m < 1,
 * m^2 > 2^31 - 1, capacity < 1 or its bytes past int64, tau < 0 or NaN); null
 * pointer; *rank < 0 or > capacity (QS_ERR_BAD_EXTENT); misaligned pointer
 * (element size for u and vectors, 8 for rank, diag, pivots and extremes, 16 for
 * work); work_bytes below the query (QS_ERR_WORKSPACE).  (Additions: the ABI
 * version stays 4.)
 */
int64_t qs_cholesky_two_body_workspace(int dtype, int64_t m, int64_t capacity);
int64_t qs_cholesky_two_body_block(void);
int qs_cholesky_two_body(int dtype, const void* u, int64_t m, double tau, void* vectors, int64_t capacity,
                         int64_t* rank, double* diag, int64_t* pivots, double* extremes, void* work,
                         int64_t work_bytes, void* stream);
/*
 * Coulomb elements of the two-dimensional harmonic oscillator by exact quadrature
 * (csrc/qs_tdho_quadrature.hip): the tensor of
 * qs_tdho_coulomb_elements / _nm, omega = 1, from a form with no cancellation,
 *   out[p - p_lo, q, r, s] = sum_{g < R} (F_pr[g] * F_qs[g]) * wt_g   where m_p + m_q == m_r + m_s,
 *                            +0.0                                      elsewhere,
 * one fma chain over ascending g.  F_pr[g] is the form factor of the orbital pair
 * at node k_g: a signed product of two orthonormal Laguerre functions of k_g^2 / 4.
 * R = max_shell nodes (the positive half of the 2R-point Gauss-Hermite rule) make
 * the sum exact: the integrand is exp(-k^2 / 2) times an even polynomial of degree
 * <= 4 (R - 1).  Measured against 80-digit values up to 22 shells: DESIGN 3.19.
 *   out       : (p_hi - p_lo, l, l, l) fp64, device, 8-byte aligned
 *   nm_table  : device array of 2 l int32 (n of every orbital, then m of every
 *               orbital) with max_shell = max(2 n + |m| + 1) over it, or NULL:
 *               the shell order of qs_tdho_coulomb_elements, and max_shell is
 *               ignored and derived from l
 *   workspace : qs_tdho_coulomb_quadrature_workspace bytes, device, 16-byte
 *               aligned: F (l, l, max_shell) and the orbitals grouped by m.  The
 *               query takes max_shell <= 0 for the shell order.
 * Limits: 1 <= l <= 2048, 1 <= max_shell <= 32 (shell order: l <= 528), else
 * QS_ERR_BAD_EXTENT.  A table that exceeds its max_shell gives wrong numbers for
 * the orbitals that do, and is never read or written out of bounds.
 * Promises:
 *   - the bits of an element depend on neither p_lo / p_hi nor repetition;
 *   - u[p,q,r,s], u[q,p,s,r] and u[r,s,p,q] have identical bits (F[p][r] and
 *     F[r][p] are one number, and the product above commutes), so
 *     qs_two_body_exchange_symmetric says yes;
 *   - an element that does not conserve m is +0.0, sign bit included.
 * Three launches in stream order (the index of m groups, F, the assembly: one store
 * per element, no atomics); asynchronous.  Errors, in this order, before any HIP
 * call: null out / workspace (and bytes of the query); extents (l, the slab,
 * max_shell); misaligned pointer (8 out, 4 nm_table, 16 workspace);
 * workspace_bytes below the query (QS_ERR_WORKSPACE).
 *
 * qs_tdho_quadrature_nodes: HOST arrays k_out, w_out of max_shell doubles receive
 * the nodes k_g = sqrt(2) t_g, ascending, and the weights wt_g = sqrt(2) w_g
 * exp(t_g^2) of that rule (t_g, w_g: the positive half of Gauss-Hermite with
 * 2 max_shell points).  Plain host code, no HIP call.  (Additions: the ABI version
 * stays 4.)
 */
int qs_tdho_quadrature_nodes(int64_t max_shell, double* k_out, double* w_out);
int qs_tdho_coulomb_quadrature_workspace(int64_t l, int64_t max_shell, int64_t* bytes);
int qs_tdho_coulomb_quadrature(void* out, const void* nm_table, int64_t l, int64_t max_shell, int64_t p_lo,
                               int64_t p_hi, void* workspace, int64_t workspace_bytes, void* stream);
/*
 * The same tensor as vectors, without building it (csrc/qs_tdho_quadrature.hip,
 * DESIGN 3.22): the m-conservation delta splits by the transfer mu = m_s - m_q, so
 *   u[p,q,r,s] = sum_x L_x[r,p] L_x[q,s],     x = j R + g,  mu_j = j - (m_max - m_min),
 *   out[x - x_lo][q][s] = fl(sqrt(wt_g)) * F_qs[g]   where m_s - m_q == mu_j,
 *                         +0.0                        elsewhere,
 * with R = max_shell, g ascending as in qs_tdho_quadrature_nodes and j = 0 ...
 * 2 (m_max - m_min): rank = R (2 (m_max - m_min) + 1) vectors, R (4 R - 3) for
 * full shells.  L_x is real, so M_x = L_x^T = L_x^H in u = sum_x M_x (x) L_x.
 *   out       : (x_hi - x_lo, l, l) fp64, device, 8-byte aligned
 *   nm_table, max_shell, workspace: as for qs_tdho_coulomb_quadrature;
 *               qs_tdho_coulomb_vectors_workspace is the same number of bytes
 *   x_lo, x_hi: the vectors to write, 0 <= x_lo < x_hi <= rank.  Under a table,
 *               which lives on the device, x_hi is checked against the most its
 *               max_shell allows, max_shell (4 max_shell - 3); vectors past the
 *               table's own rank are all +0.0.
 * qs_tdho_coulomb_vectors_rank: the rank of a table given as a HOST array of
 * 2 l int32 (same layout), or of the shell order (NULL); plain host code.  A table
 * whose m spread exceeds 2 (max_shell - 1) is QS_ERR_BAD_EXTENT.
 * Limits and the order of the argument errors are those of
 * qs_tdho_coulomb_quadrature, the slab x_lo:x_hi among the extents.
 * Promises:
 *   - the bits of an element depend on neither x_lo / x_hi nor repetition;
 *   - out[(j, g)][q][s] and out[(N - 1 - j, g)][s][q], N = 2 (m_max - m_min) + 1,
 *     have identical bits (F[q][s] and F[s][q] are one number);
 *   - an element outside its band is +0.0, sign bit included;
 *   - every element of out is stored exactly once (16-byte stores, one 8-byte
 *     store where a vector starts or ends on an odd double), nothing else is.
 * Three launches in stream order (index, F, the store kernel; no atomics, 64-bit
 * offsets); asynchronous.  (Additions: the ABI version stays 4.)
 */
int qs_tdho_coulomb_vectors_workspace(int64_t l, int64_t max_shell, int64_t* bytes);
int qs_tdho_coulomb_vectors_rank(const void* nm_table_host, int64_t l, int64_t max_shell, int64_t* rank);
int qs_tdho_coulomb_vectors(void* out, const void* nm_table, int64_t l, int64_t max_shell, int64_t x_lo,
                            int64_t x_hi, void* workspace, int64_t workspace_bytes, void* stream);
/*
 * Closed-shell perturbative triples: the energy of occupied triples from their
 * blocks (csrc/qs_triples.hip).  Triple x owns six blocks of X, each
 * (v, v, v) row-major of dtype: X_0 ... X_5 = X_ijk, X_ikj, X_jik, X_jki, X_kij,
 * X_kji at the block indices slots[x][0 ... 5] (equal occupied indices share
 * blocks: equal entries are allowed and read once).  With
 *   W[a,b,c] = X_0[a,b,c] + X_1[a,c,b] + X_2[b,a,c] + X_3[b,c,a] + X_4[c,a,b] + X_5[c,b,a]
 *   Z[a,b,c] = (4 W[abc] + W[bca] + W[cab] - 2 W[acb] - 2 W[cba] - 2 W[bac]) / 3
 *   e[x]     = sum_abc Re(conj(W[abc]) Z[abc]) / (eo3[x] - ev[a] - ev[b] - ev[c])
 * without the weight of the triple.  W and Z are never stored; every element of
 * the six blocks is read once.
 *   X      : (nblocks, v, v, v) of dtype, device
 *   slots  : (n, 6) int32, device, every entry in 0 ... nblocks - 1; a triple
 *            with an entry outside that range reads nothing and gets e = NaN
 *   eo3    : n doubles, device: e_i + e_j + e_k of the triple
 *   ev     : v doubles, device: the virtual orbital energies
 *   e      : n doubles, device, out
 *   work   : qs_triples_energy_workspace bytes, device, 8-byte aligned: one
 *            partial per (triple, set of three tiles)
 * Two launches in stream order, no atomics, asynchronous: a workgroup per triple
 * and unordered set of three tiles of edge qs_triples_energy_tile(dtype) along
 * a, b, c adds its elements in a fixed order; a closing launch adds the partials
 * of a triple in an order fixed by v alone.  e[x] has the same bits on every
 * run, and the same alone as anywhere in a batch.
 * Limits: 1 <= v <= 4096, n >= 1, n times the tile sets of one triple below 2^31,
 * 1 <= nblocks < 2^31 with the bytes of X inside int64, else QS_ERR_BAD_EXTENT.
 * Errors, in this order, before any HIP call: dtype; extents; null pointer;
 * misaligned pointer (element size X, 4 slots, 8 the others); work_bytes below
 * the query (QS_ERR_WORKSPACE); e sharing a byte with an input or the workspace,
 * or the workspace with X (QS_ERR_ALIAS).
 *
 * qs_triples_energy_budget: the byte budget in force on the calling thread --
 * the tuning key "triples_bytes" where it is positive, else budget_bytes
 * (negative: QS_ERR_BAD_EXTENT).  Plain host code.  (Additions: the ABI version
 * stays 4.)
 */
int64_t qs_triples_energy_tile(int dtype);
int64_t qs_triples_energy_budget(int64_t budget_bytes);
int64_t qs_triples_energy_workspace(int dtype, int64_t v, int64_t n);
int qs_triples_energy(int dtype, const void* X, int64_t nblocks, const int32_t* slots, const double* eo3, const double* ev,
                      int64_t v, int64_t n, double* e, void* work, int64_t work_bytes, void* stream);
/*
 * The same with the singles term of (T) beside it.  Block beta of
 * triple x has a partner Y_beta[p,q,r] = A[sa][p] G[sg][q,r], an outer product
 * that is never stored, with (sa, sg) = sslots[x][beta]; V' is made from the
 * Y_beta as W from the X_beta, and
 *   e[x]  = as qs_triples_energy (the connected part)
 *   es[x] = sum_abc Re(conj(V'[abc]) Z[abc]) / (eo3[x] - ev[a] - ev[b] - ev[c])
 *   A      : (na, v) of dtype, device
 *   G      : (ng, v, v) of dtype, device
 *   sslots : (n, 6, 2) int32, device: (sa, sg) per slot, in 0 ... na - 1 and
 *            0 ... ng - 1; a triple with an entry of slots or sslots out of
 *            range reads nothing and gets e = es = NaN
 *   e, es  : n doubles each, device, out
 *   work   : qs_triples_energy_singles_workspace bytes (two partials per triple
 *            and set of tiles), device, 8-byte aligned
 * Three launches in stream order (the work units, one close per output), no
 * atomics, asynchronous; the bits of e[x] and es[x] depend on the triple's own
 * inputs alone.  Limits and errors as qs_triples_energy, with 1 <= na, ng < 2^31,
 * A and G aligned to the element size, sslots to 4; QS_ERR_ALIAS where e, es or
 * the workspace share a byte with an input or with one another.  (Additions:
 * the ABI version stays 4.)
 */
int64_t qs_triples_energy_singles_workspace(int dtype, int64_t v, int64_t n);
int qs_triples_energy_singles(int dtype, const void* X, int64_t nblocks, const int32_t* slots, const double* eo3,
                              const double* ev, const void* A, int64_t na, const void* G, int64_t ng, const int32_t* sslots,
                              int64_t v, int64_t n, double* e, double* es, void* work, int64_t work_bytes, void* stream);
int qs_probe_mfma_f64(void* sink, int64_t blocks, int64_t iters, void* stream);
int qs_probe_stream_copy(const void* src, void* dst, int64_t bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* QS_AMD_H */
