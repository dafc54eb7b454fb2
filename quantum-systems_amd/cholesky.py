"""Cholesky vectors of the two-body tensor: decompose once, then transform and consume the vectors instead of ``u``.

With ``G[(r,p),(q,s)] = u[p,q,r,s]`` -- Hermitian positive semidefinite for a positive interaction and a plain, not
anti-symmetrised ``u`` -- a pivoted Cholesky decomposition ``G = V V^H`` gives, with ``L_x = conj(V_x)`` as (m, m)
matrices and ``M_x = L_x^H``,

    u[p,q,r,s] = sum_x M_x[p,r] L_x[q,s]                     (to the threshold of the decomposition)

For the Coulomb tensor of a two-dimensional quantum dot with R closed shells the rank is (2R - 1) 2R / 2, about 4 l
instead of l^2, exact to rounding: l^4 elements become about 4 l^3.

    chol = cholesky.decompose(system, tol=1e-9 * float(abs(system.u).max()))
    chol.rank, chol.converged, chol.residual
    W = chol.mean_field(rho, cj=1.0, ck=-0.5)                # a Fock build: a few products on the vectors
    g = chol.transform(C).block(o, o, v, v)                  # <ij|ab> in another basis, O(rank l^3)
    hf = HartreeFock(system, two_body=chol)

The decomposition is ``kernels.cholesky_two_body`` (``qs_cholesky_two_body``); everything after it is the product
dispatcher (``kernels.gemm_raw``) and ``kernels.transform_one_body`` on stacks of m x m matrices.

Hermiticity of ``G`` -- ``u[p,q,r,s] == conj(u[r,s,p,q])`` -- is the caller's contract and is NOT checked: the
decomposition reads one triangle's worth of columns and would silently decompose the Hermitian matrix they imply.
"""

import math

import torch

from . import kernels
from .basis_set import _stage, refuse_vectors_only
from .sharded_module import is_sharded


def _plain(arr):
    return _stage(arr).as_subclass(torch.Tensor)


def _index_range(x, m):
    """``(start, stop)`` of a slice or range of step 1 inside ``0 ... m``."""
    if isinstance(x, slice):
        x = range(*x.indices(m))
    if not isinstance(x, range) or x.step != 1 or not 0 <= x.start < x.stop <= m:
        raise ValueError(f"block() takes non-empty slices or ranges of step 1 inside 0 ... {m}, got {x!r}")
    return x.start, x.stop


def decompose(u_or_system, tol, max_rank=None):
    """Pivoted Cholesky vectors of a two-body tensor ``u`` (m, m, m, m) or of a system's ``u``, to the threshold
    ``tol`` (absolute: every element of ``u - reconstruct()`` is bounded by the largest residual diagonal, which is
    ``<= tol`` when the run converged).  Returns a ``CholeskyTwoBody``.

    The vector buffer starts at ``8 m`` vectors (clipped to ``m^2`` and ``max_rank``); where a run ends on the capacity
    and ``max_rank`` allows more, the buffer is doubled and the run resumed -- with the bits of an uninterrupted run.
    With ``max_rank`` reached first the result has ``converged == False`` and exactly ``max_rank`` vectors.

    Raises ``ValueError`` for a system whose ``u`` is anti-symmetrised, and where the smallest residual diagonal is
    below ``-tol``: the matrix is not positive semidefinite (an anti-symmetrised tensor, the negative of an
    interaction, or an otherwise indefinite one), and where a residual extreme is not finite: a NaN on the residual
    diagonal ends the kernel's run with a NaN as its largest element, which is an error here, never "converged".
    Hermiticity of ``G[(r,p),(q,s)] = u[p,q,r,s]`` is the caller's
    contract and is not checked."""
    u = u_or_system
    if hasattr(u_or_system, "_basis_set"):
        refuse_vectors_only(u_or_system, "cholesky.decompose")
        if u_or_system._basis_set._anti_symmetrized_u:
            raise ValueError(
                "the system's u is anti-symmetrised: its matrix G[(r,p),(q,s)] is indefinite and has no Cholesky "
                "vectors -- decompose the plain <pq|rs>")
        u = u_or_system.u
    if is_sharded(u):
        raise NotImplementedError("decompose does not take a sharded u")
    with torch._C.DisableTorchFunctionSubclass():
        u = _plain(u)
        if u.dim() != 4 or len(set(u.shape)) != 1:
            raise ValueError(f"u must be (m, m, m, m), got {tuple(u.shape)}")
        m = u.shape[0]
        limit = m * m if max_rank is None else min(int(max_rank), m * m)
        if limit < 1:
            raise ValueError("max_rank must be at least 1")
        cap = min(8 * m, limit)
        state = None
        while True:
            L, _, (dmax, dmin), state = kernels.cholesky_two_body(u, tol, max_rank=cap, state=state)
            converged = dmax <= tol
            if not (math.isfinite(dmax) and math.isfinite(dmin)):
                raise ValueError(
                    f"non-finite residual diagonal after {state.rank} vectors (largest {dmax}, smallest {dmin}): u holds a "
                    "NaN or an infinity, or the run produced one")
            if converged or state.rank < cap or cap >= limit:
                break
            cap = min(2 * cap, limit)
        if dmin < -tol:
            raise ValueError(
                f"the smallest residual diagonal is {dmin:.3e}, below -tol = {-tol:.3e}: G[(r,p),(q,s)] = u[p,q,r,s] is "
                "not positive semidefinite (an anti-symmetrised or otherwise indefinite tensor has no Cholesky vectors)")
        if state.rank < state.capacity:
            L = L.clone()
        return CholeskyTwoBody(L, None, tol=tol, residual=(dmax, dmin), converged=converged)


class CholeskyTwoBody:
    """The two-body tensor as vectors: ``u[p,q,r,s] = sum_x M[x,p,r] L[x,q,s]``.

    ``L`` (rank, m, m) device tensor; ``M`` (rank, m, m) or ``None`` for ``M_x = L_x^H`` (which holds in every basis
    reached by ``C~ = C^H``); ``rank``; ``tol`` and ``residual = (largest, smallest)`` residual diagonal of the
    decomposition; ``converged``: largest ``<= tol``."""

    def __init__(self, L, M=None, tol=0.0, residual=(0.0, 0.0), converged=True):
        with torch._C.DisableTorchFunctionSubclass():
            self.L = _plain(L).contiguous()
            self.M = None if M is None else _plain(M).contiguous()
        if self.L.dim() != 3 or self.L.shape[1] != self.L.shape[2] or (self.M is not None and self.M.shape != self.L.shape):
            raise ValueError("L (and M) must be (rank, m, m)")
        self.tol, self.residual, self.converged = tol, tuple(residual), bool(converged)
        self._Mc = self.M

    @property
    def rank(self):
        return self.L.shape[0]

    @property
    def m(self):
        return self.L.shape[1]

    def _bra(self):
        """``M`` materialised: (rank, m, m)."""
        if self._Mc is None:
            self._Mc = self.L.conj().transpose(1, 2).resolve_conj().contiguous()
        return self._Mc

    def transform(self, C, C_tilde=None):
        """The vectors in the basis ``C`` (l, m'), rectangular included: ``L'_x = C~ L_x C``, ``M'_x = C~ M_x C`` --
        ``kernels.transform_one_body`` on the stack, O(rank l^3) -- so that ``reconstruct()`` of the result is
        ``transform_two_body(u, C, C~)``.  With ``C~ = C^H`` (the default) ``M' = L'^H`` stays implicit; a ``C_tilde``
        that is given and is not ``C^H`` (a bi-orthogonal pair) keeps ``M`` as a stack of its own.  Returns a new
        object."""
        with torch._C.DisableTorchFunctionSubclass():
            C = _plain(C)
            if C_tilde is not None:
                C_tilde = _plain(C_tilde)
                if C_tilde.shape == (C.shape[1], C.shape[0]) and torch.equal(C_tilde, kernels.default_bra(C).to(C_tilde.dtype)):
                    C_tilde = None
            L = kernels.transform_one_body(self.L, C, C_tilde)
            M = None
            if C_tilde is not None or self.M is not None:
                M = kernels.transform_one_body(self._bra(), C, C_tilde)
        return CholeskyTwoBody(L, M, tol=self.tol, residual=self.residual, converged=self.converged)

    def reconstruct(self, out=None):
        """``u[p,q,r,s] = sum_x M[x,p,r] L[x,q,s]`` (m, m, m, m), written in that index order without a permuted
        copy: for every ``p`` one batched product over ``q``, ``out[p,q] (r x s) = M[:,p,:]^T . L[:,q,:]``."""
        with torch._C.DisableTorchFunctionSubclass():
            m, r, dt = self.m, self.rank, self.L.dtype
            if out is None:
                out = torch.empty((m, m, m, m), dtype=dt, device=self.L.device)
            else:
                kernels._check_out(out, (m, m, m, m), dt, "reconstruct")
            if r == 0:
                return out.zero_()
            Mt = self._bra().permute(1, 2, 0).contiguous()              # [p, r, x]
            for p in range(m):
                # A = Mt[p] (m x rank);  B_q = L[:, q, :] (rank x m, ldb = m^2, batch stride m);  C_q = out[p, q]
                kernels.gemm_raw(dt, Mt, self.L, out, m, m, r, r, m * m, m, batch=m, sa=0, sb=m, sc=m * m,
                                 a_off=p * m * r, c_off=p * m * m * m)
        return out

    def block(self, P, Q, R, S):
        """``u[P, Q, R, S]`` for four slices or ranges (step 1), from the sliced vectors in ONE product:
        ``(M[:, P, R] as (|P||R|, rank)) . (L[:, Q, S] as (rank, |Q||S|))``, then the small block is put in the
        project's index order."""
        with torch._C.DisableTorchFunctionSubclass():
            m = self.m
            (p0, p1), (q0, q1), (r0, r1), (s0, s1) = (_index_range(x, m) for x in (P, Q, R, S))
            shape = (p1 - p0, r1 - r0, q1 - q0, s1 - s0)
            if self.rank == 0:
                return torch.zeros(shape, dtype=self.L.dtype, device=self.L.device).permute(0, 2, 1, 3).contiguous()
            A = self._bra()[:, p0:p1, r0:r1].permute(1, 2, 0).reshape(shape[0] * shape[1], self.rank)
            B = self.L[:, q0:q1, s0:s1].reshape(self.rank, shape[2] * shape[3])
            return kernels.matmul(A, B).reshape(shape).permute(0, 2, 1, 3).contiguous()

    def transform_blocks(self, bras, kets):
        """``out[pqrs] = Ct0[pa] Ct1[qb] u[abcd] C2[cr] C3[ds]`` with ``bras = (Ct0, Ct1)`` (rows, (M, m)) and ``kets =
        (C2, C3)`` (columns, (m, M)) -- ``BasisSet.transform_two_body_blocks`` on the vectors: the two stacks of
        rectangular one-body transforms ``Ct0 M_x C2`` and ``Ct1 L_x C3`` (bra first: the small side of ``<ij|ab>``
        shrinks the stack), then one product over ``x``, put in the project's index order."""
        with torch._C.DisableTorchFunctionSubclass():
            (Ct0, Ct1), (C2, C3) = ((_plain(c) for c in bras), (_plain(c) for c in kets))
            m, r = self.m, self.rank
            if not (Ct0.dim() == Ct1.dim() == C2.dim() == C3.dim() == 2
                    and Ct0.shape[1] == Ct1.shape[1] == C2.shape[0] == C3.shape[0] == m):
                raise ValueError(f"bras must be (M, {m}) and kets ({m}, M)")
            dt = kernels.result_dtype(self.L, Ct0, Ct1, C2, C3)
            shape = (Ct0.shape[0], C2.shape[1], Ct1.shape[0], C3.shape[1])
            if r == 0:
                return torch.zeros(shape, dtype=dt, device=self.L.device).permute(0, 2, 1, 3).contiguous()

            def stack(V, Ct, C):
                half = kernels.matmul(Ct.to(dt), V.to(dt))                                  # (rank, M, m)
                return kernels.matmul(half.reshape(r * Ct.shape[0], m), C.to(dt))          # (rank M, M')

            A = stack(self._bra(), Ct0, C2).reshape(r, shape[0] * shape[1]).transpose(0, 1).contiguous()
            B = stack(self.L, Ct1, C3).reshape(r, shape[2] * shape[3])
            return kernels.matmul(A, B).reshape(shape).permute(0, 2, 1, 3).contiguous()

    def mean_field(self, D, cj=1.0, ck=0.0):
        """``W = cj sum_x M_x tr(L_x D) + ck sum_x M_x D L_x`` -- ``kernels.mean_field(u, D, cj, ck)`` on the vectors,
        ``D`` (m, m) real or complex.  The Coulomb term is two matrix-vector products; the exchange term two products:
        ``Y[p,(x,s)] = (M_x (ck D))[p,s]`` written straight into that layout (the batch stride and ``ldc`` of the
        product), then ``Y (m x rank m) . L (rank m x m)`` with the sum over ``x`` inside the inner dimension."""
        with torch._C.DisableTorchFunctionSubclass():
            D = _plain(D)
            m, r = self.m, self.rank
            if tuple(D.shape) != (m, m):
                raise ValueError(f"D must be ({m}, {m}), got {tuple(D.shape)}")
            dt = kernels.result_dtype(self.L, D)
            D = kernels._dev(D, dt)
            L, M = kernels._dev(self.L, dt), kernels._dev(self._bra(), dt)
            W = torch.zeros((m, m), dtype=dt, device=L.device)
            if r == 0:
                return W
            wrote = False
            if cj != 0.0:
                Dt = (cj * D).transpose(0, 1).contiguous()                          # [(r,s)] -> cj D[s,r]
                t = torch.empty(r, dtype=dt, device=L.device)
                kernels.gemm_raw(dt, L, Dt, t, r, 1, m * m, m * m, 1, 1)           # t_x = cj tr(L_x D)
                kernels.gemm_raw(dt, t, M, W, 1, m * m, r, r, m * m, m * m)        # W = sum_x t_x M_x
                wrote = True
            if ck != 0.0:
                Dk = (ck * D).contiguous()
                Y = torch.empty((m, r, m), dtype=dt, device=L.device)
                kernels.gemm_raw(dt, M, Dk, Y, m, m, m, m, m, r * m, batch=r, sa=m * m, sb=0, sc=m)
                kernels.gemm_raw(dt, Y, L, W, m, m, r * m, r * m, m, m, accumulate=wrote)
            return W
