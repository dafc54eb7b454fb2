"""One batched product as flat host buffers with NaN around the operands and a sentinel around C: the ``Case`` shared by
tests/test_gpu_strip_forms.py and tests/test_gpu_stream_forms.py (imports nothing from the package but the kernels module
a test hands to ``run``).

Bound (derived as tests/_blocks_ref.py and tests/test_gpu_fast_walk.py, not tuned): an inner product of length k in any
order has relative error gamma_(k+1) on its absolute-value sum, one more rounding for the conversion at the end:
|C - exact| <= gamma_(k+2) |A| |B| element-wise, times 2 sqrt 2 for complex products; ``exact`` is the numpy.longdouble
(clongdouble) product of the same strided views."""

import numpy as np
import torch
from numpy.lib.stride_tricks import as_strided

from _blocks_ref import gamma

SENTINEL = -7777.25


def cdiv(a, b):
    return -(-a // b)


def odd_layout(cx, m, n, k):
    """(lda, ldb, ldc, gap of sb, gap of sc, element offset of every base): fp64 all odd, complex128 padded."""
    if cx:
        return k + 1, n + 2, n + 3, 1, 1, 1
    lda, ldb, ldc = k + 1 + k % 2, n + 1 + n % 2, n + 3 - n % 2
    return lda, ldb, ldc, 1 + (k + 1) * ldb % 2, 1 + (m + 1) * ldc % 2, 1


def even_layout(cx, m, n, k):
    """16-byte bases and even strides, still padded."""
    return k + 2 - k % 2, n + 2 - n % 2, n + 4 - n % 2, 2, 2, 0


class Case:
    """One product C[t] = A B[t] (A shared) as flat host buffers: C[t] at offs + t sc with m + 1 rows of ldc, B[t] at
    offs + t sb with k + 1 rows of ldb, A at offs with m rows of lda and eight elements of slack.  NaN around the
    operands, the sentinel around (and, unless ``accumulate``, in) C; the long-double product of the strided views.

    ``per_entry_a``: an A per batch entry, C[t] = A[t] B[t], A[t] at offs + t sa with sa = m lda + 3 (NaN between them).
    ``reference=False`` leaves the long-double product and the bound out (a case that is only launched)."""

    def __init__(self, cx, m, n, k, batch, layout, seed, offs=None, accumulate=False, per_entry_a=False, reference=True):
        self.cx, self.m, self.n, self.k, self.batch = cx, m, n, k, batch
        self.lda, self.ldb, self.ldc, gap_b, gap_c, off = layout
        self.offs = offs if offs is not None else (off, off, off)
        self.sb, self.sc = (k + 1) * self.ldb + gap_b, (m + 1) * self.ldc + gap_c
        self.sa = m * self.lda + 3 if per_entry_a else 0
        self.accumulate = accumulate
        dt = np.complex128 if cx else np.float64
        rng = np.random.default_rng(seed)

        def rnd(*shape):
            x = rng.standard_normal(shape)
            return x + 1j * rng.standard_normal(shape) if cx else x

        oa, ob, oc = self.offs
        es = dt().itemsize
        if per_entry_a:
            self.A = np.full(oa + batch * self.sa + 8, np.nan, dtype=dt)
            a = as_strided(self.A[oa:], (batch, m, k), (self.sa * es, self.lda * es, es))
            a[...] = rnd(batch, m, k)
        else:
            self.A = np.full(oa + m * self.lda + 8, np.nan, dtype=dt)
            a = as_strided(self.A[oa:], (m, k), (self.lda * es, es))
            a[...] = rnd(m, k)
        self.B = np.full(ob + batch * self.sb, np.nan, dtype=dt)
        b = as_strided(self.B[ob:], (batch, k, n), (self.sb * es, self.ldb * es, es))
        b[...] = rnd(batch, k, n)
        self.C0 = np.full(oc + batch * self.sc, SENTINEL, dtype=dt)
        self.stored = np.zeros(self.C0.size, dtype=bool)
        as_strided(self.stored[oc:], (batch, m, n), (self.sc, self.ldc, 1))[...] = True
        self.c0 = rnd(batch, m, n) if accumulate else None
        if accumulate:
            self.view(self.C0)[...] = self.c0
        self.dt = torch.complex128 if cx else torch.float64
        self.dA, self.dB, self.dC0 = (torch.from_numpy(x).cuda() for x in (self.A, self.B, self.C0))
        if not reference:
            self.prod = self.bound = None
            return
        ld = np.clongdouble if cx else np.longdouble
        self.prod = np.matmul(a.astype(ld), b.astype(ld))                  # (batch, m, n), a shared A broadcast
        bound = gamma(k + 2) * np.matmul(np.abs(a), np.abs(b))
        if accumulate:
            self.prod = self.prod + self.c0
            bound = bound + gamma(k + 2) * np.abs(self.c0)
        self.bound = bound * (2.0 * np.sqrt(2.0) if cx else 1.0)

    def view(self, flat):
        es = flat.dtype.itemsize
        return as_strided(flat[self.offs[2]:], (self.batch, self.m, self.n), (self.sc * es, self.ldc * es, es))

    def run(self, K, **kw):
        out = self.dC0.clone()
        K.gemm_raw(self.dt, self.dA, self.dB, out, self.m, self.n, self.k, self.lda, self.ldb, self.ldc, self.batch,
                   self.sa if self.batch > 1 else 0, self.sb if self.batch > 1 else 0, self.sc if self.batch > 1 else 0,
                   self.accumulate, a_off=self.offs[0], b_off=self.offs[1], c_off=self.offs[2], **kw)
        return out

    def ratio(self, out, entries=None):
        """Largest error / bound of the stored elements (of the batch entries ``entries``: all); asserts that nothing
        else was written and that no NaN was stored."""
        got = out.cpu().numpy()
        stored = self.stored
        if entries is not None:
            stored = np.zeros_like(self.stored)
            as_strided(stored[self.offs[2]:], (self.batch, self.m, self.n), (self.sc, self.ldc, 1))[entries] = True
        assert np.array_equal(got[~stored], self.C0[~stored]), "a sentinel around C was overwritten"
        c = self.view(got)
        sel = slice(None) if entries is None else entries
        assert not np.isnan(c[sel].real).any() and not np.isnan(c[sel].imag).any(), "a NaN reached a stored element"
        return float((np.abs(c[sel] - self.prod[sel]) / self.bound[sel]).max())
