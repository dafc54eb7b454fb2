"""Typed Python front of the C ABI: torch tensors in, torch tensors out.

PyTorch is used here for what it is good at on ROCm -- owning device memory
and the current HIP stream.  Every function hands raw device pointers to
``libqs_amd.so``; none of them computes anything with torch ops, and none has a
CPU path: a tensor that is not on a ``cuda`` device is an error.
"""

import ctypes

import torch

from . import _lib
from ._lib import QS_C128, QS_F64, check
from .partition import SlabPartition

_F64 = torch.float64
_C128 = torch.complex128


def dtype_code(dtype):
    if dtype == _F64:
        return QS_F64
    if dtype == _C128:
        return QS_C128
    raise TypeError(f"only float64 and complex128 are supported, got {dtype}")


def _stream():
    """Raw handle of the current device's current stream (``torch.cuda.current_stream().cuda_stream`` without the
    Python object around it: the wrappers below are on the path of every small-basis transform)."""
    return torch._C._cuda_getCurrentRawStream(torch._C._cuda_getDevice())


def _plain(fn):
    """The wrapped function sees device arrays as plain tensors: every tensor method called on a ``torch.Tensor``
    subclass (``DeviceArray``) otherwise goes through ``__torch_function__`` and re-wraps its result -- ~100 of those
    per ``change_basis`` cost more than the kernels of a 55-orbital transform.  Results come back as plain tensors
    (the callers wrap what they hand out)."""
    import functools

    @functools.wraps(fn)
    def inner(*args, **kwargs):
        with torch._C.DisableTorchFunctionSubclass():
            return fn(*args, **kwargs)

    return inner


# Measurement hook (bench.py): when this is a list, every compute call appends the kernels it
# launched (qs_last_dispatch), so a bench line can name what actually ran.  None = off.
dispatch_log = None


def _ran(code, what):
    code = check(code, what)
    if dispatch_log is not None:
        dispatch_log.append(_lib.load().qs_last_dispatch().decode())
    return code


def _dev(t, dtype=None):
    """Contiguous, conjugation-resolved device tensor of the wanted dtype."""
    if not isinstance(t, torch.Tensor):
        raise TypeError("expected a torch.Tensor")
    if not t.is_cuda:
        raise RuntimeError(
            "the transform path runs on the GPU only: move the array to the "
            "device module first (change_module)"
        )
    if dtype is not None and t.dtype != dtype:
        t = t.to(dtype)
    if t.is_conj():
        t = t.resolve_conj()
    return t if t.is_contiguous() else t.contiguous()


class _on_device_of:
    """Launch context: makes the device that owns the operands current (the C ABI
    launches on the current device, and ``_stream()`` is that device's current
    stream) and refuses operands that live on different devices."""

    def __init__(self, *tensors):
        dev = None
        for t in tensors:
            if t is None:
                continue
            if dev is None:
                dev = t.device
            elif t.device != dev:
                devs = {x.device for x in tensors if x is not None}
                raise ValueError(f"operands live on different devices: {sorted(str(d) for d in devs)}")
        if dev is None:
            raise ValueError("operands live on different devices: []")
        self.device = dev
        self._guard = None

    def __enter__(self):
        if self.device.index != torch._C._cuda_getDevice():
            self._guard = torch.cuda.device(self.device)
            self._guard.__enter__()
        return self

    def __exit__(self, *exc):
        if self._guard is not None:
            self._guard.__exit__(*exc)
        return False


def _check_out(out, shape, dt, what):
    """A caller-supplied output buffer goes to the kernels as a raw pointer: it
    must be exactly what the kernel will write (dtype, shape, contiguous, on the GPU)."""
    if not isinstance(out, torch.Tensor) or not out.is_cuda:
        raise ValueError(f"{what}: `out` must be a device tensor")
    if out.dtype != dt or tuple(out.shape) != tuple(shape) or not out.is_contiguous():
        raise ValueError(
            f"{what}: `out` must be a contiguous {dt} tensor of shape {tuple(shape)}, got "
            f"{out.dtype} {tuple(out.shape)}{'' if out.is_contiguous() else ' (non-contiguous)'}"
        )
    return out


def result_dtype(*tensors):
    """NumPy-style promotion restricted to {float64, complex128}."""
    out = _F64
    for t in tensors:
        if not isinstance(t, torch.Tensor):
            raise TypeError(f"expected a torch.Tensor, got {type(t).__name__}")
        if t.dtype in (torch.complex64, _C128):
            out = _C128
        elif t.dtype not in (_F64, torch.float32, torch.int64, torch.int32):
            raise TypeError(f"unsupported dtype {t.dtype}")
    return out


@_plain
def default_bra(C):
    """``C.conj().T`` materialised (basis_set.py:331-332, 338-339)."""
    if not isinstance(C, torch.Tensor):
        raise TypeError(f"expected a torch.Tensor, got {type(C).__name__}")
    return C.conj().transpose(0, 1).resolve_conj().contiguous()


class Workspace:
    """Grow-only device scratch shared by the transforms of one process, ONE BUFFER PER DEVICE (a process that drives
    several GPUs -- the one-process-eight-devices style -- would otherwise free and re-allocate the scratch of the
    other device on every call).

    The C ABI never allocates; this keeps the buffers alive between calls so a time loop calling the transform every step
    does not hit the allocator.  Calls that share a device's buffer are meant to be issued on ONE stream per device (stream
    order keeps them apart); concurrent streams of one device should call the C ABI with their own workspaces, or use one
    ``TransformPlan`` each."""

    def __init__(self):
        self._bufs = {}

    def get(self, nbytes, device):
        key = (device.type, device.index if device.index is not None else torch.cuda.current_device())
        buf = self._bufs.get(key)
        if buf is None or buf.numel() < nbytes:
            self._bufs[key] = None  # release before growing
            buf = torch.empty(int(nbytes), dtype=torch.uint8, device=device)
            self._bufs[key] = buf
        return buf

    def release(self, device=None):
        """Drop the scratch of one device (or of all of them)."""
        if device is None:
            self._bufs.clear()
        else:
            device = torch.device(device)
            self._bufs.pop((device.type, device.index if device.index is not None else torch.cuda.current_device()), None)


workspace = Workspace()


def _work(nbytes, device):
    """``(pointer, size)`` of ``nbytes`` of the shared scratch of ``device``; ``(None, 0)`` for a call that needs none."""
    if not nbytes:
        return None, 0
    work = workspace.get(nbytes, device)
    return work.data_ptr(), work.numel()


# A/B switch for measurements (bench.py --dtype mixed, tests): False restores the route of rounds 1-2 for a real u against
# complex coefficients -- a complex copy of the whole tensor, then the complex transform.
mixed_real_u = True


@_plain
def gemm_raw(dt, A, B, out, m, n, k, lda, ldb, ldc, batch=1, sa=0, sb=0, sc=0,
             accumulate=False, a_off=0, b_off=0, c_off=0, pairs=None, mirror=False, lower=False):
    """Thin call of ``qs_matmul`` on tensors already prepared by the caller
    (contiguous storage, matching dtype); offsets and strides in elements.

    ``pairs=n``: ``qs_matmul_pairs`` -- the batch is the upper triangle of an n x n grid (``batch`` is not used), the
    operands of pair (i, j >= i) at ``(i * n + j)`` strides; with ``mirror=True`` ``qs_matmul_pairs_mirrored``, which also
    stores pair (i, j > i) transposed at (j, i) and raises ``ValueError`` where no kernel can; with ``lower=True``
    ``qs_matmul_pairs_lower``, which takes the 16 x 16 blocks below the block diagonal of the square ``A`` entry of pair
    (i, j) from the mirror entry (j, i) and raises ``ValueError`` where no kernel can."""
    lib = _lib.load()
    es = 16 if dt == _C128 else 8
    if (mirror or lower) and pairs is None:
        raise ValueError("mirror=True and lower=True need pairs=n")
    if mirror and lower:
        raise ValueError("mirror=True and lower=True are two different launches")
    fn, name, count = ((lib.qs_matmul, "qs_matmul", batch) if pairs is None else
                       (lib.qs_matmul_pairs_mirrored, "qs_matmul_pairs_mirrored", pairs) if mirror else
                       (lib.qs_matmul_pairs_lower, "qs_matmul_pairs_lower", pairs) if lower else
                       (lib.qs_matmul_pairs, "qs_matmul_pairs", pairs))
    with _on_device_of(A, B, out):
        _ran(
            fn(
                dtype_code(dt), A.data_ptr() + a_off * es, B.data_ptr() + b_off * es,
                out.data_ptr() + c_off * es, m, n, k, lda, ldb, ldc, count, sa, sb, sc,
                1 if accumulate else 0, _stream(),
            ),
            name,
        )
    return out


@_plain
def matmul_upper(dt, A, B, out, m, side, stack, k, lda, ldb, ldc, batch=1, sa=0, sb=0, sc=0, accumulate=False,
                 a_off=0, b_off=0, c_off=0):
    """Thin call of ``qs_matmul_upper`` on tensors already prepared by the caller, offsets and strides in elements: the
    product on the column blocks that meet ``d >= c`` of a stack of row-major ``side x side`` matrices ``(c, d)``
    (``n = stack * side * side`` columns).  float64 on the exact tiled forms only; raises ``ValueError`` where no kernel
    can.  Returns ``out``."""
    lib = _lib.load()
    es = 16 if dt == _C128 else 8
    with _on_device_of(A, B, out):
        _ran(
            lib.qs_matmul_upper(
                dtype_code(dt), A.data_ptr() + a_off * es, B.data_ptr() + b_off * es, out.data_ptr() + c_off * es,
                m, side, stack, k, lda, ldb, ldc, batch, sa, sb, sc, 1 if accumulate else 0, _stream(),
            ),
            "qs_matmul_upper",
        )
    return out


@_plain
def matmul(A, B, out=None, accumulate=False):
    """Row-major ``A @ B`` for 2-D operands (or a shared 2-D ``A`` against a
    batch ``B`` of shape (batch, k, n)); ``accumulate`` adds into ``out``."""
    dt = result_dtype(A, B)
    A = _dev(A, dt)
    B = _dev(B, dt)
    if A.dim() != 2:
        raise ValueError("A must be 2-D")
    m, k = A.shape
    if B.dim() == 2:
        batch, (kb, n) = 1, B.shape
        oshape = (m, n)
    elif B.dim() == 3:
        batch, kb, n = B.shape
        oshape = (batch, m, n)
    else:
        raise ValueError("B must be 2-D or 3-D")
    if kb != k:
        raise ValueError(f"inner dimensions differ: {k} vs {kb}")
    if out is None:
        if accumulate:
            raise ValueError("accumulate needs an output buffer")
        out = torch.empty(oshape, dtype=dt, device=A.device)
    elif (not isinstance(out, torch.Tensor) or not out.is_cuda or out.dtype != dt
          or out.numel() != batch * m * n or not out.is_contiguous()):
        raise ValueError("bad output buffer")
    return gemm_raw(dt, A, B, out, m, n, k, k, n, n, batch, 0, k * n, m * n, accumulate)


def _takes_exchange_route(lib, code, u, L, M, work, exchange):
    """Does this transform take the route for a tensor with particle-exchange symmetry, ``u[a,b,c,d] == u[b,a,d,c]``
    (qs_amd.h)?  Only where the library's policy wants it for the size (``qs_transform_two_body_exchange_wanted``, which
    honours the tuning keys) and the check kernel finds the symmetry bit for bit -- the check is the ONE blocking call of
    the path: it synchronises the current stream, and on a capturing stream it answers "no" without launching.  Nothing
    is remembered between calls (a tensor written through a raw pointer would keep a stale verdict)."""
    if exchange is False or not lib.qs_transform_two_body_exchange_wanted(code, L, M):
        return False
    return _ran(lib.qs_two_body_exchange_symmetric(code, u.data_ptr(), L, work.data_ptr(), _stream()),
                "qs_two_body_exchange_symmetric") == 1


@_plain
def transform_two_body(u, C, C_tilde=None, out=None, exchange=None):
    """out[pqrs] = Ct[pa] Ct[qb] u[abcd] C[cr] C[ds]  (basis_set.py:336-350).

    ``exchange=None``: a tensor with particle-exchange symmetry takes the route that skips the half the symmetry
    repeats, where that is faster (``_takes_exchange_route``); ``exchange=False``: the four full products always."""
    lib = _lib.load()
    if C_tilde is None:
        C_tilde = default_bra(C)
    dt = result_dtype(u, C, C_tilde)
    # a real fp64 tensor against complex coefficients (NumPy's promotion, basis_set.py:341-342; the time-propagation
    # call on a real quantum-dot u) stays real: the d contraction reads it as it is (qs_transform_two_body_mixed)
    mixed = dt == _C128 and isinstance(u, torch.Tensor) and u.dtype == _F64 and mixed_real_u
    u = _dev(u, _F64 if mixed else dt)
    C = _dev(C, dt)
    Ct = _dev(C_tilde, dt)
    L, M = C.shape
    if tuple(u.shape) != (L, L, L, L):
        raise ValueError(f"u has shape {tuple(u.shape)}, C is {tuple(C.shape)}")
    if tuple(Ct.shape) != (M, L):
        raise ValueError(f"C_tilde has shape {tuple(Ct.shape)}, expected {(M, L)}")
    code = dtype_code(dt)
    nbytes = check(lib.qs_transform_two_body_workspace(code, L, M), "workspace query")
    if out is None:
        out = torch.empty((M, M, M, M), dtype=dt, device=u.device)
    else:
        _check_out(out, (M, M, M, M), dt, "transform_two_body")
    with _on_device_of(u, C, Ct, out):
        work = workspace.get(nbytes, u.device)
        if mixed:
            _ran(
                lib.qs_transform_two_body_mixed(
                    u.data_ptr(), C.data_ptr(), Ct.data_ptr(), out.data_ptr(),
                    work.data_ptr(), work.numel(), L, M, _stream(),
                ),
                "qs_transform_two_body_mixed",
            )
        else:
            route = "qs_transform_two_body" + ("_exchange" if _takes_exchange_route(lib, code, u, L, M, work, exchange) else "")
            _ran(
                getattr(lib, route)(
                    code, u.data_ptr(), C.data_ptr(), Ct.data_ptr(), out.data_ptr(),
                    work.data_ptr(), work.numel(), L, M, _stream(),
                ),
                route,
            )
    return out


@_plain
def transform_two_body_(u, C, C_tilde=None, exchange=None):
    """The transform IN PLACE: ``u`` (L,L,L,L; float64 / complex128, contiguous, owning its storage) is overwritten
    and the result (M,M,M,M), M <= L, is returned as a view of the start of its storage.  One L^3 M spare buffer
    instead of workspace + result (qs_transform_two_body_inplace): for callers that drop the old tensor.
    ``exchange``: as in ``transform_two_body``."""
    lib = _lib.load()
    if C_tilde is None:
        C_tilde = default_bra(C)
    dt = result_dtype(u, C, C_tilde)
    if not isinstance(u, torch.Tensor) or not u.is_cuda or u.dtype != dt or not u.is_contiguous():
        raise ValueError("the in-place transform needs a contiguous device tensor that already has the result dtype")
    C, Ct = _dev(C, dt), _dev(C_tilde, dt)
    L, M = C.shape
    if tuple(u.shape) != (L, L, L, L) or tuple(Ct.shape) != (M, L) or M > L:
        raise ValueError(f"u {tuple(u.shape)}, C {tuple(C.shape)}, C_tilde {tuple(Ct.shape)}: need u (L,L,L,L) and M <= L")
    code = dtype_code(dt)
    nbytes = check(lib.qs_transform_two_body_inplace_workspace(code, L, M), "workspace query")
    with _on_device_of(u, C, Ct):
        work = workspace.get(nbytes, u.device)
        route = "qs_transform_two_body_inplace" + ("_exchange" if _takes_exchange_route(lib, code, u, L, M, work, exchange) else "")
        _ran(
            getattr(lib, route)(code, u.data_ptr(), C.data_ptr(), Ct.data_ptr(), work.data_ptr(), work.numel(), L, M, _stream()),
            route,
        )
    # (the tensor itself when the size does not change: no view object keeps a second handle on the storage, so
    # the next change_basis can reuse it again)
    return u if M == L else u.reshape(-1)[: M**4].reshape(M, M, M, M)


class TransformPlan:
    """The four-index transform of a RESIDENT ``u`` captured once as a HIP graph,
    for loops that transform every step with new coefficients (the
    time-propagation pattern of BASELINE.json configs[4]: ``C(t)`` changes, ``u``
    stays).  At small l a transform is a handful of 10 us kernels and the host
    side of each call (argument checks, ctypes, allocator) costs as much as the
    GPU work; a graph replay is one launch.

        plan = TransformPlan(u, C)          # u (L,L,L,L), C (L,M), C_tilde optional
        for step in ...:
            plan.C.copy_(C_t)               # update the static coefficient buffers in place
            plan.C_tilde.copy_(Ct_t)
            out = plan.replay()             # valid until the next replay

    The captured launches are exactly those of ``transform_two_body(..., exchange=False)``
    (``qs_transform_two_body`` on the capture stream); buffers, workspace and the
    output are owned by the plan.  The plan stays on the four full products: the
    exchange-symmetry check reads its verdict back, which a capture cannot do
    (``qs_two_body_exchange_symmetric`` and ``qs_transform_two_body_exchange`` are
    separate calls so that a plan could run the check once, before capturing)."""

    def __init__(self, u, C, C_tilde=None):
        lib = _lib.load()
        if C_tilde is None:
            C_tilde = default_bra(C)
        dt = result_dtype(u, C, C_tilde)
        self.u = _dev(u, dt)
        self.C = _dev(C, dt).clone()
        self.C_tilde = _dev(C_tilde, dt).clone()
        L, M = self.C.shape
        if tuple(self.u.shape) != (L, L, L, L) or tuple(self.C_tilde.shape) != (M, L):
            raise ValueError("operand shapes do not match C")
        code = dtype_code(dt)
        nbytes = check(lib.qs_transform_two_body_workspace(code, L, M), "workspace query")
        self.out = torch.empty((M, M, M, M), dtype=dt, device=self.u.device)
        self._work = torch.empty(int(nbytes), dtype=torch.uint8, device=self.u.device)

        def launch():
            _ran(
                lib.qs_transform_two_body(
                    code, self.u.data_ptr(), self.C.data_ptr(), self.C_tilde.data_ptr(),
                    self.out.data_ptr(), self._work.data_ptr(), self._work.numel(), L, M, _stream(),
                ),
                "qs_transform_two_body",
            )

        if self.u.device.index != torch.cuda.current_device():
            raise ValueError("TransformPlan: make the device that owns `u` current first (torch.cuda.device)")

        # one eager run on a side stream (first-launch set-up: function attributes, device
        # properties), then the capture
        side = torch.cuda.Stream(device=self.u.device)
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            launch()
        torch.cuda.current_stream().wait_stream(side)
        self.graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(self.graph):
            launch()

    def replay(self):
        self.graph.replay()
        return self.out


@_plain
def two_body_exchange_symmetric(u):
    """Does ``u`` (l,l,l,l; float64 / complex128 on the device) have particle-exchange symmetry,
    ``u[a,b,c,d] == u[b,a,d,c]``, bit for bit?  Blocks (``qs_two_body_exchange_symmetric``); False on a capturing stream."""
    lib = _lib.load()
    u = _dev(u)
    code = dtype_code(u.dtype)
    l = u.shape[0] if u.dim() == 4 else 0
    if tuple(u.shape) != (l, l, l, l):
        raise ValueError(f"u has shape {tuple(u.shape)}, expected (l, l, l, l)")
    with _on_device_of(u):
        work = workspace.get(16, u.device)
        return _ran(lib.qs_two_body_exchange_symmetric(code, u.data_ptr(), l, work.data_ptr(), _stream()),
                    "qs_two_body_exchange_symmetric") == 1


@_plain
def exchange_mirror_(t, block=1):
    """In place on ``t`` (n,n,m,m), contiguous: ``t[a,b,r,s] = t[b,a,s,r]`` wherever ``a // block > b // block``
    (``qs_exchange_mirror``); returns ``t``."""
    lib = _lib.load()
    if not isinstance(t, torch.Tensor) or not t.is_cuda or not t.is_contiguous() or t.dim() != 4 \
            or t.shape[0] != t.shape[1] or t.shape[2] != t.shape[3]:
        raise ValueError("exchange_mirror_ needs a contiguous device tensor of shape (n, n, m, m)")
    with _on_device_of(t):
        _ran(lib.qs_exchange_mirror(dtype_code(t.dtype), t.data_ptr(), t.shape[0], t.shape[2], int(block), _stream()),
             "qs_exchange_mirror")
    return t


@_plain
def exchange_mirror_lower_(t):
    """In place on ``t`` (n,n,m,m), contiguous float64: ``t[i,j,r,s] = t[j,i,s,r]`` for every pair ``i <= j`` and every
    ``s < r`` (``qs_exchange_mirror_lower``: the fill of ``exchange_upper``); returns ``t``."""
    lib = _lib.load()
    if not isinstance(t, torch.Tensor) or not t.is_cuda or not t.is_contiguous() or t.dim() != 4 \
            or t.shape[0] != t.shape[1] or t.shape[2] != t.shape[3]:
        raise ValueError("exchange_mirror_lower_ needs a contiguous device tensor of shape (n, n, m, m)")
    with _on_device_of(t):
        _ran(lib.qs_exchange_mirror_lower(dtype_code(t.dtype), t.data_ptr(), t.shape[0], t.shape[2], _stream()),
             "qs_exchange_mirror_lower")
    return t


def _pair_operands(name, src, dst, src_shape, dst_shape):
    for t, shape in ((src, src_shape), (dst, dst_shape)):
        if not isinstance(t, torch.Tensor) or not t.is_cuda or not t.is_contiguous() or tuple(t.shape) != shape \
                or t.dtype != src.dtype:
            raise ValueError(f"{name} needs contiguous device tensors of one dtype, shapes {src_shape} and {dst_shape}")


@_plain
def exchange_pair_transpose(src, dst):
    """``dst[c,d,a,b] = src[a,b,c,d]`` for the pairs ``d >= c``, both (l,l,l,l); the rest of ``dst`` is left as it is
    (``qs_exchange_pair_transpose``: the way in of ``exchange_leading=2``); returns ``dst``."""
    lib = _lib.load()
    l = src.shape[0] if isinstance(src, torch.Tensor) and src.dim() == 4 else 0
    _pair_operands("exchange_pair_transpose", src, dst, (l, l, l, l), (l, l, l, l))
    with _on_device_of(src, dst):
        _ran(lib.qs_exchange_pair_transpose(dtype_code(src.dtype), src.data_ptr(), dst.data_ptr(), l, _stream()),
             "qs_exchange_pair_transpose")
    return dst


@_plain
def exchange_pair_transpose_back(src, dst):
    """The way back: ``src`` (l,l,m,m), read on the pairs ``d >= c`` only, to ``dst`` (m,m,l,l) on the pairs ``q >= p``:
    ``dst[p,q,c,d] = src[c,d,p,q]`` where ``d >= c``, ``src[d,c,q,p]`` where ``d < c``; the rest of ``dst`` is left as it
    is (``qs_exchange_pair_transpose_back``); returns ``dst``."""
    lib = _lib.load()
    l, m = (src.shape[0], src.shape[2]) if isinstance(src, torch.Tensor) and src.dim() == 4 else (0, 0)
    _pair_operands("exchange_pair_transpose_back", src, dst, (l, l, m, m), (m, m, l, l))
    with _on_device_of(src, dst):
        _ran(lib.qs_exchange_pair_transpose_back(dtype_code(src.dtype), src.data_ptr(), dst.data_ptr(), l, m, _stream()),
             "qs_exchange_pair_transpose_back")
    return dst


@_plain
def transform_two_body_partial(u_slab, C, C_tilde=None, out=None):
    """Contractions over d, c, b of a leading-index slab:
    v[a,q,r,s] = Ct[qb] u[a,b,c,d] C[cr] C[ds] for the rows of the slab."""
    lib = _lib.load()
    if C_tilde is None:
        C_tilde = default_bra(C)
    dt = result_dtype(u_slab, C, C_tilde)
    u_slab = _dev(u_slab, dt)
    C = _dev(C, dt)
    Ct = _dev(C_tilde, dt)
    L, M = C.shape
    rows = u_slab.shape[0]
    if tuple(u_slab.shape[1:]) != (L, L, L):
        raise ValueError("slab shape does not match C")
    code = dtype_code(dt)
    nbytes = check(
        lib.qs_transform_two_body_partial_workspace(code, L, M, rows), "workspace query"
    )
    if out is None:
        out = torch.empty((rows, M, M, M), dtype=dt, device=u_slab.device)
    else:
        _check_out(out, (rows, M, M, M), dt, "transform_two_body_partial")
    with _on_device_of(u_slab, C, Ct, out):
        work = workspace.get(nbytes, u_slab.device)
        _ran(
            lib.qs_transform_two_body_partial(
                code, u_slab.data_ptr(), C.data_ptr(), Ct.data_ptr(), out.data_ptr(),
                work.data_ptr(), work.numel(), L, M, rows, _stream(),
            ),
            "qs_transform_two_body_partial",
        )
    return out


@_plain
def transform_one_body(h, C, C_tilde=None):
    """``Ct @ (h @ C)`` for one (L,L) matrix or a stack (n,L,L)
    (basis_set.py:329-334)."""
    lib = _lib.load()
    if C_tilde is None:
        C_tilde = default_bra(C)
    dt = result_dtype(h, C, C_tilde)
    h = _dev(h, dt)
    C = _dev(C, dt)
    Ct = _dev(C_tilde, dt)
    L, M = C.shape
    single = h.dim() == 2
    hs = h.reshape(-1, L, L) if not single else h.reshape(1, L, L)
    if tuple(hs.shape[1:]) != (L, L) or tuple(Ct.shape) != (M, L):
        raise ValueError("operand shapes do not match C")
    nmat = hs.shape[0]
    out = torch.empty((nmat, M, M), dtype=dt, device=h.device)
    es = 16 if dt == _C128 else 8
    with _on_device_of(hs, C, Ct):
        work = workspace.get(nmat * L * M * es, h.device)
        _ran(
            lib.qs_transform_one_body(
                dtype_code(dt), hs.data_ptr(), C.data_ptr(), Ct.data_ptr(), out.data_ptr(),
                work.data_ptr(), work.numel(), nmat, L, M, _stream(),
            ),
            "qs_transform_one_body",
        )
    return out[0] if single else out.reshape(*h.shape[:-2], M, M)


@_plain
def antisymmetrize(u, out=None):
    """``u - u.transpose(0,1,3,2)`` (basis_set.py:776-778); pass ``out=u`` for
    the in-place form."""
    lib = _lib.load()
    dt = result_dtype(u)
    src = _dev(u, dt)
    l = src.shape[-1]
    if src.dim() < 2 or src.shape[-2] != l:
        raise ValueError("last two axes must be square")
    npq = src.numel() // (l * l)
    in_place = out is u
    if out is None:
        out = torch.empty_like(src)
    elif in_place:
        out = src          # the kernel's tile-pair scheme is safe in place
    else:
        _check_out(out, src.shape, dt, "antisymmetrize")
    with _on_device_of(src, out):
        _ran(
            lib.qs_antisymmetrize(dtype_code(dt), src.data_ptr(), out.data_ptr(), npq, l, _stream()),
            "qs_antisymmetrize",
        )
    if in_place and src is not u:
        u.copy_(src)       # `u` was a view / other dtype: write the result back into it
        return u
    return out


@_plain
def spin_expand_two_body(u, antisymmetrize=False, out_dtype=None, p_lo=0, p_hi=None, out=None):
    """Spin doubling of (l,l,l,l) -> rows [2 p_lo, 2 p_hi) of (2l,2l,2l,2l)
    (basis_set.py:772-774), optionally fused with the anti-symmetrisation
    (:776-778) and the complex cast (:634).

    ``u`` may also be a leading-index slab ``u[a:b]`` of shape (rows,l,l,l) -- the
    p-sharded layout, where no rank holds the whole tensor; ``p_lo``/``p_hi`` then
    count rows of the slab (the expansion is slab-local: output row 2p+s needs
    input row p only)."""
    lib = _lib.load()
    dt = result_dtype(u)
    u = _dev(u, dt)
    if u.dim() != 4:
        raise ValueError("u must be (l,l,l,l)")
    rows, l = u.shape[0], u.shape[-1]
    if tuple(u.shape[1:]) != (l, l, l) or rows > l or rows < 1:
        raise ValueError("u must be (l,l,l,l) or a leading-index slab (rows,l,l,l)")
    p_hi = rows if p_hi is None else p_hi
    if not 0 <= p_lo < p_hi <= rows:
        raise ValueError(f"rows [{p_lo}, {p_hi}) are not inside the {rows} rows of u")
    odt = dt if out_dtype is None else out_dtype
    shape = (2 * (p_hi - p_lo), 2 * l, 2 * l, 2 * l)
    if out is None:
        out = torch.empty(shape, dtype=odt, device=u.device)
    else:
        _check_out(out, shape, odt, "spin_expand_two_body")
    with _on_device_of(u, out):
        _ran(
            lib.qs_spin_expand_two_body(
                dtype_code(dt), dtype_code(odt), u.data_ptr(), out.data_ptr(), l, p_lo, p_hi,
                1 if antisymmetrize else 0, _stream(),
            ),
            "qs_spin_expand_two_body",
        )
    return out


@_plain
def spin_expand_two_body_block(u_block, antisymmetrize=False, out_dtype=None, out=None):
    """Spin doubling of a block ``u[p0:p0+np, q0:q0+nq, :, :]`` of shape (np, nq, l, l) ->
    (2 np, 2 nq, 2l, 2l): what a rank of a sharded tensor holds, whichever of the two leading
    indices is the sharded one (basis_set.py:772-778, :634 on the rank's share)."""
    lib = _lib.load()
    dt = result_dtype(u_block)
    u_block = _dev(u_block, dt)
    if u_block.dim() != 4 or u_block.shape[2] != u_block.shape[3]:
        raise ValueError("u_block must be (np, nq, l, l)")
    np_, nq, l = u_block.shape[0], u_block.shape[1], u_block.shape[3]
    if np_ > l or nq > l or np_ < 1 or nq < 1:
        raise ValueError("block extents must be within 1..l")
    odt = dt if out_dtype is None else out_dtype
    shape = (2 * np_, 2 * nq, 2 * l, 2 * l)
    if out is None:
        out = torch.empty(shape, dtype=odt, device=u_block.device)
    else:
        _check_out(out, shape, odt, "spin_expand_two_body_block")
    with _on_device_of(u_block, out):
        _ran(
            lib.qs_spin_expand_two_body_block(
                dtype_code(dt), dtype_code(odt), u_block.data_ptr(), out.data_ptr(), l, np_, nq,
                1 if antisymmetrize else 0, _stream(),
            ),
            "qs_spin_expand_two_body_block",
        )
    return out


@_plain
def add_spin_one_body(h, out_dtype=None):
    """``kron(h, I2)`` for (l,l) or a stack (n,l,l) (basis_set.py:768-770)."""
    lib = _lib.load()
    dt = result_dtype(h)
    h = _dev(h, dt)
    l = h.shape[-1]
    if h.shape[-2] != l:
        raise ValueError("last two axes must be square")
    nmat = h.numel() // (l * l)
    odt = dt if out_dtype is None else out_dtype
    out = torch.empty(tuple(h.shape[:-2]) + (2 * l, 2 * l), dtype=odt, device=h.device)
    with _on_device_of(h):
        _ran(
            lib.qs_add_spin_one_body(
                dtype_code(dt), dtype_code(odt), h.data_ptr(), out.data_ptr(), nmat, l, _stream()
            ),
            "qs_add_spin_one_body",
        )
    return out


@_plain
def spin_squared_two_body(S, antisymmetrize=False, p_lo=0, p_hi=None):
    """Two-body S^2 from the stacked (3,n,n) spin matrices
    (basis_set.py:745-747)."""
    lib = _lib.load()
    S = _dev(S, _C128)
    n = S.shape[-1]
    if tuple(S.shape) != (3, n, n):
        raise ValueError("S must be (3,n,n)")
    p_hi = n if p_hi is None else p_hi
    out = torch.empty((p_hi - p_lo, n, n, n), dtype=_C128, device=S.device)
    with _on_device_of(S):
        _ran(
            lib.qs_spin_squared_two_body(
                S.data_ptr(), out.data_ptr(), n, p_lo, p_hi, 1 if antisymmetrize else 0, _stream()
            ),
            "qs_spin_squared_two_body",
        )
    return out


@_plain
def two_body_from_grid(K, C, C_tilde=None, antisymmetrize=False):
    """Two-body elements of an interaction that is DIAGONAL on a grid / DVR basis,

        out[p,q,r,s] = sum_ab Ct[p,a] Ct[q,b] K[a,b] C[a,r] C[b,s]

    -- the transform of a sinc-DVR ``u`` kept in its 2-d form
    (sinc_dvr/one_dim/sinc_dvr.py:217-246, optional fused anti-symmetrisation
    :247-256) and, with ``C_tilde = C.T``, the grid quadrature that builds the
    ``u`` of a 1-D quantum dot (quantum_dots/one_dim/one_dim_qd.py:275-280).
    Two GEMMs on the MFMA kernels instead of a five-operand einsum:
    ``rho[a,(p,r)] = Ct[p,a] C[a,r]``, ``W = K rho``, ``out[(p,r),(q,s)] = rho^T W``;
    O(N^2 M^2 + N M^4) for N grid points and M orbitals.  ``C_tilde`` defaults to
    ``C.conj().T`` as in the reference."""
    Ct = default_bra(C) if C_tilde is None else C_tilde
    dt = result_dtype(K, C, Ct)
    K, C, Ct = _dev(K, dt), _dev(C, dt), _dev(Ct, dt)
    N, M = C.shape
    if tuple(K.shape) != (N, N) or tuple(Ct.shape) != (M, N):
        raise ValueError(f"K {tuple(K.shape)}, C {tuple(C.shape)}, C_tilde {tuple(Ct.shape)} do not fit")
    rho = (Ct.transpose(0, 1).unsqueeze(2) * C.unsqueeze(1)).reshape(N, M * M)
    W = matmul(K, rho)                                            # (N, (q,s))
    out = matmul(rho.transpose(0, 1).contiguous(), W)             # ((p,r), (q,s))
    out = out.reshape(M, M, M, M).permute(0, 2, 1, 3).contiguous()
    if antisymmetrize:
        antisymmetrize_(out)
    return out


@_plain
def antisymmetrize_(u):
    """In-place form of ``antisymmetrize``."""
    return antisymmetrize(u, out=u)


def _mean_field_operands(u, D, d_dims, r_lo):
    """Device operands of the mean-field kernels: ``u`` (P, R, L, L) and ``D`` (L, L) (``d_dims`` = 2) or (ND, L, L)
    (3), and the slab's extents.  Returns ``(u, D, udt, dt, P, R, L)``."""
    d_shape = "(L, L)" if d_dims == 2 else "(ND, L, L)"
    dt = result_dtype(u, D)
    udt = _F64 if isinstance(u, torch.Tensor) and u.dtype == _F64 else dt
    u = _dev(u, udt)
    D = _dev(D, dt)
    if u.dim() != 4 or D.dim() != d_dims:
        raise ValueError(f"u must be (P, R, L, L) and D {d_shape}")
    P, R, L = u.shape[0], u.shape[1], u.shape[3]
    if u.shape[2] != L or tuple(D.shape[-2:]) != (L, L) or (d_dims == 3 and D.shape[0] < 1):
        raise ValueError(f"u has shape {tuple(u.shape)}, D {tuple(D.shape)}: need u (P, R, L, L) and D {d_shape}"
                         + (", ND >= 1" if d_dims == 3 else ""))
    if not (1 <= P <= L and 1 <= R and 0 <= r_lo and r_lo + R <= L):
        raise ValueError(f"slab of {P} rows and second indices [{r_lo}, {r_lo + R}) does not fit L = {L}")
    return u, D, udt, dt, P, R, L


@_plain
def mean_field(u, D, cj=1.0, ck=0.0, r_lo=0, out=None):
    """Mean-field contraction of the two-body tensor with a one-body density, both sums from one read of ``u``
    (``qs_mean_field``):

        W[p,q] = cj * sum_rs u[p,r,q,s] D[s,r]  +  ck * sum_rs u[p,r,s,q] D[s,r]

    ``u`` is (P, R, L, L): the whole tensor, a rows slab ``u[lo:hi]`` or a second-index slab ``u[:, lo:hi]`` whose
    ``r`` starts at ``r_lo`` (then ``W`` is the partial sum over the slab's ``r``).  ``D`` is (L, L).  A real ``u``
    with a complex ``D`` stays real (complex ``W``).  Returns ``W`` (P, L)."""
    lib = _lib.load()
    u, D, udt, dt, P, R, L = _mean_field_operands(u, D, 2, r_lo)
    ucode, dcode = dtype_code(udt), dtype_code(dt)
    nbytes = check(lib.qs_mean_field_workspace(ucode, dcode, L, P, R), "workspace query")
    if out is None:
        out = torch.empty((P, L), dtype=dt, device=u.device)
    else:
        _check_out(out, (P, L), dt, "mean_field")
    with _on_device_of(u, D, out):
        work = workspace.get(nbytes, u.device)
        _ran(
            lib.qs_mean_field(
                ucode, dcode, u.data_ptr(), D.data_ptr(), out.data_ptr(), L, P, R, int(r_lo), float(cj), float(ck),
                work.data_ptr(), work.numel(), _stream(),
            ),
            "qs_mean_field",
        )
    return out


def _weights(x, nd, name):
    """A scalar or a length-ND sequence of weights as a host array of ND doubles."""
    if isinstance(x, torch.Tensor):
        x = x.tolist()
    scalar = getattr(x, "ndim", None) == 0 or not hasattr(x, "__len__")       # a 0-d array has __len__ and no length
    vals = [float(x)] * nd if scalar else [float(v) for v in x]
    if len(vals) != nd:
        raise ValueError(f"{name} has {len(vals)} weights for {nd} densities")
    return (ctypes.c_double * nd)(*vals)


@_plain
def mean_field_batch(u, D, cj=1.0, ck=0.0, r_lo=0, out=None):
    """The mean-field contraction of ``mean_field`` for a batch of densities from ONE read of ``u`` per group of G of
    them (``qs_mean_field_batch``):

        W[k,p,q] = cj[k] * sum_rs u[p,r,q,s] D[k,s,r]  +  ck[k] * sum_rs u[p,r,s,q] D[k,s,r]

    ``u`` is (P, R, L, L) as for ``mean_field``, ``D`` is (ND, L, L), ``cj`` / ``ck`` are scalars or length-ND
    sequences.  ``W[k]`` has the same bits whether ``D[k]`` is sent alone or anywhere in a batch of any size.
    Returns ``W`` (ND, P, L)."""
    lib = _lib.load()
    u, D, udt, dt, P, R, L = _mean_field_operands(u, D, 3, r_lo)
    ND = D.shape[0]
    wj, wk = _weights(cj, ND, "cj"), _weights(ck, ND, "ck")
    ucode, dcode = dtype_code(udt), dtype_code(dt)
    nbytes = check(lib.qs_mean_field_batch_workspace(ucode, dcode, L, P, R, ND), "workspace query")
    if out is None:
        out = torch.empty((ND, P, L), dtype=dt, device=u.device)
    else:
        _check_out(out, (ND, P, L), dt, "mean_field_batch")
    with _on_device_of(u, D, out):
        work = workspace.get(nbytes, u.device)
        _ran(
            lib.qs_mean_field_batch(
                ucode, dcode, u.data_ptr(), D.data_ptr(), out.data_ptr(), L, P, R, int(r_lo), ND,
                ctypes.cast(wj, ctypes.c_void_p), ctypes.cast(wk, ctypes.c_void_p),
                work.data_ptr(), work.numel(), _stream(),
            ),
            "qs_mean_field_batch",
        )
    return out


@_plain
def lead_contract(A, B, out=None):
    """``A @ B`` for a few rows: ``A`` (m, k) with ``1 <= m <= 32``, ``B`` (k, n) -- contiguous, or a column slice
    ``W[:, :n]`` of a wider row-major buffer, read in place -- on the streaming kernel of ``qs_lead_contract``: one
    read of ``B``, every element one fused multiply-add chain over ascending ``a``.  A real ``B`` with a complex ``A``
    stays real (complex result).  Returns ``T`` (m, n)."""
    lib = _lib.load()
    dt = result_dtype(A, B)
    bdt = _F64 if isinstance(B, torch.Tensor) and B.dtype == _F64 else dt
    A = _dev(A, dt)
    if not isinstance(B, torch.Tensor):
        raise TypeError("expected a torch.Tensor")
    if A.dim() != 2 or B.dim() != 2 or B.shape[0] != A.shape[1]:
        raise ValueError("A must be (m, k) and B (k, n)")
    if not (B.is_cuda and B.dtype == bdt and not B.is_conj() and B.stride(1) == 1 and
            (B.shape[0] == 1 or B.stride(0) >= B.shape[1])):
        B = _dev(B, bdt)
    m, k = A.shape
    n = B.shape[1]
    ldb = B.stride(0) if k > 1 else max(n, B.stride(0))
    if not 1 <= m <= 32:
        raise ValueError(f"lead_contract takes 1 ... 32 rows, got {m}")
    if out is None:
        out = torch.empty((m, n), dtype=dt, device=B.device)
    else:
        _check_out(out, (m, n), dt, "lead_contract")
    with _on_device_of(A, B, out):
        _ran(
            lib.qs_lead_contract(dtype_code(dt), dtype_code(bdt), A.data_ptr(), B.data_ptr(), out.data_ptr(), m, n, k,
                                 k, ldb, n, _stream()),
            "qs_lead_contract",
        )
    return out


@_plain
def pair_contract(u, T, out=None):
    """``S[k,p,q] = sum_rs u[p,q,r,s] T[k,r,s]`` (no conjugation) on the streaming kernel of ``qs_pair_contract``: one
    read of ``u`` per group of G amplitudes, ``u`` never reshaped or copied.  ``u`` is (P, Q, R, S'), contiguous, a
    leading slice ``w[lo:hi]`` of a contiguous tensor, or rows of R S' contiguous elements at one uniform distance
    (``w[:, :, :R * S'].unflatten(2, (R, S'))`` of a wider buffer), all read in place; ``T`` is (K, R, S') or (R, S').  A real ``u`` with a complex
    ``T`` stays real (complex result).  ``S[k]`` has the same bits alone and anywhere in a batch of any size, and a row
    ``(p, q)`` the same bits whatever slice of ``u`` it is sent in.  Returns (K, P, Q), or (P, Q) for a 2-D ``T``."""
    lib = _lib.load()
    dt = result_dtype(u, T)
    udt = _F64 if isinstance(u, torch.Tensor) and u.dtype == _F64 else dt
    if not isinstance(u, torch.Tensor):
        raise TypeError("expected a torch.Tensor")
    if u.dim() != 4 or not isinstance(T, torch.Tensor) or T.dim() not in (2, 3):
        raise ValueError("u must be (P, Q, R, S) and T (K, R, S) or (R, S)")
    # rows (p, q) of R * S contiguous elements at one uniform distance ldu >= R * S are read in place
    ldu = u.stride(1) if u.shape[0] * u.shape[1] > 1 else u.shape[2] * u.shape[3]
    if not (u.is_cuda and u.dtype == udt and not u.is_conj() and min(u.shape) >= 1 and u.stride(3) == 1 and
            u.stride(2) == u.shape[3] and ldu >= u.shape[2] * u.shape[3] and
            (u.shape[0] == 1 or u.shape[1] == 1 or u.stride(0) == u.shape[1] * ldu)):
        u = _dev(u, udt)
        ldu = u.shape[2] * u.shape[3]
    elif u.shape[1] == 1 and u.shape[0] > 1:
        ldu = u.stride(0)
    T = _dev(T, dt)
    single = T.dim() == 2
    if single:
        T = T[None]
    P, Q, R, S_ = u.shape
    K = T.shape[0]
    if tuple(T.shape[1:]) != (R, S_) or K < 1 or min(P, Q, R, S_) < 1:
        raise ValueError(f"u has shape {tuple(u.shape)}, T {tuple(T.shape)}: need u (P, Q, R, S) and T (K, R, S), K >= 1")
    X, Y = P * Q, R * S_
    ucode, tcode = dtype_code(udt), dtype_code(dt)
    nbytes = check(lib.qs_pair_contract_workspace(ucode, tcode, X, Y, K), "workspace query")
    if out is None:
        out = torch.empty((P, Q) if single else (K, P, Q), dtype=dt, device=u.device)
    else:
        _check_out(out, (P, Q) if single else (K, P, Q), dt, "pair_contract")
    with _on_device_of(u, T, out):
        _ran(
            lib.qs_pair_contract(ucode, tcode, u.data_ptr(), T.data_ptr(), out.data_ptr(), X, Y, K, ldu,
                                 *_work(nbytes, u.device), _stream()),
            "qs_pair_contract",
        )
    return out


def _pair_contract_triangle(name, min_l, u, T, out):
    """The two pair contractions on a packed triangle of ``u`` (``name``: the C entry, ``min_l``: its smallest l): ``u``
    (l, l, l, l) read in place where its rows (p, q) lie at one uniform distance, ``T`` (K, l, l) or (l, l); a real
    ``u`` with a complex ``T`` as 2 K fp64 columns."""
    lib = _lib.load()
    dt = result_dtype(u, T)
    udt = _F64 if isinstance(u, torch.Tensor) and u.dtype == _F64 else dt
    if not isinstance(u, torch.Tensor):
        raise TypeError("expected a torch.Tensor")
    if u.dim() != 4 or len(set(u.shape)) != 1 or u.shape[0] < min_l or not isinstance(T, torch.Tensor) or T.dim() not in (2, 3):
        raise ValueError(f"u must be (l, l, l, l) with l >= {min_l} and T (K, l, l) or (l, l)")
    l = u.shape[0]
    ldu = u.stride(1) if l > 1 else 1
    if not (u.is_cuda and u.dtype == udt and not u.is_conj() and (l == 1 or (
            u.stride(3) == 1 and u.stride(2) == l and ldu >= l * l and u.stride(0) == l * ldu))):
        u = _dev(u, udt)
        ldu = l * l
    T = _dev(T, dt)
    single = T.dim() == 2
    if single:
        T = T[None]
    K = T.shape[0]
    if tuple(T.shape[1:]) != (l, l) or K < 1:
        raise ValueError(f"u has shape {tuple(u.shape)}, T {tuple(T.shape)}: need u (l, l, l, l) and T (K, l, l), K >= 1")
    shape = (l, l) if single else (K, l, l)
    if out is not None:
        _check_out(out, shape, dt, name[3:])
    split = udt != dt                      # real u, complex T: (re, im) of every amplitude as two fp64 columns
    if split:
        cols = torch.view_as_real(T).permute(0, 3, 1, 2).reshape(2 * K, l, l).contiguous()
        res = torch.empty((2 * K, l, l), dtype=_F64, device=u.device)
    else:
        cols = T
        res = out if out is not None else torch.empty(shape, dtype=dt, device=u.device)
    code, ncols = dtype_code(udt), cols.shape[0]
    nbytes = check(getattr(lib, name + "_workspace")(code, code, l, ncols), "workspace query")
    with _on_device_of(u, cols, res):
        _ran(getattr(lib, name)(code, code, u.data_ptr(), cols.data_ptr(), res.data_ptr(), l, ncols, ldu,
                                *_work(nbytes, u.device), _stream()), name)
    if split:
        parts = res.view(K, 2, l, l)
        S = torch.complex(parts[:, 0], parts[:, 1])
        S = S[0] if single else S
        if out is None:
            return S
        out.copy_(S)
    return out if out is not None else res


@_plain
def pair_contract_antisym(u, T, out=None):
    """``S[k,p,q] = sum_rs u[p,q,r,s] T[k,r,s]`` (no conjugation) for an anti-symmetrised ``u`` (minus itself under
    ``p <-> q`` and under ``r <-> s``) and amplitudes ``T[k] = -T[k]^T``, on the kernel of ``qs_pair_contract_antisym``:
    only ``p < q``, ``r < s`` of ``u`` and ``r < s`` of ``T`` are read, a quarter of the bytes of ``pair_contract``;
    ``S[k,p,q] = 2 sum_{r<s}``, ``S[k,q,p]`` its negation, a zero diagonal.  The symmetries are the caller's word and
    are not checked.  ``u`` is (l, l, l, l), contiguous or rows (p, q) at one uniform
    distance, read in place; ``T`` is (K, l, l) or (l, l).  A real ``u`` with a complex ``T`` runs the fp64
    kernel on the real and the imaginary parts as 2 K amplitudes: exact, and one read of ``u`` per group as well.
    Returns (K, l, l), or (l, l) for a 2-D ``T``."""
    return _pair_contract_triangle("qs_pair_contract_antisym", 2, u, T, out)


@_plain
def pair_contract_exchange(u, T, out=None):
    """``S[k,p,q] = sum_rs u[p,q,r,s] T[k,r,s]`` (no conjugation) for ALL p, q and ANY amplitudes, for a ``u`` with
    particle-exchange symmetry ``u[p,q,r,s] = u[q,p,s,r]`` (spatial orbitals; ``two_body_exchange_symmetric``), on the
    kernel of ``qs_pair_contract_exchange``: only ``r <= s`` of ``u`` is read, half of the bytes and of the products
    of ``pair_contract``.  The symmetry is the caller's word and is not checked.  ``u`` is (l, l, l, l), contiguous or
    rows (p, q) at one uniform distance, read in place (a permuted ``u`` is made contiguous); ``T`` is (K, l, l) or
    (l, l).  A real ``u`` with a complex ``T`` runs the fp64 kernel on the real and the imaginary parts as 2 K
    amplitudes: exact, and one read of ``u`` per group as well.  Returns (K, l, l), or (l, l) for a 2-D ``T``."""
    return _pair_contract_triangle("qs_pair_contract_exchange", 1, u, T, out)


def _dets_checked(dets):
    """The determinant list every determinant kernel takes: a 1-D int64 tensor."""
    if not isinstance(dets, torch.Tensor) or dets.dtype != torch.int64 or dets.dim() != 1:
        raise ValueError("dets must be a 1-D int64 tensor of occupation masks")


def _det_ci_operands(ht, ut, dets, *more):
    """Device operands of the determinant kernels: ``ht`` (m, m), ``ut`` (m, m, m, m) in one dtype, ``dets`` int64."""
    _dets_checked(dets)
    dt = result_dtype(ht, ut, *more)
    ht, ut = _dev(ht, dt), _dev(ut, dt)
    dets = _dev(dets)
    m = ht.shape[-1]
    if tuple(ht.shape) != (m, m) or tuple(ut.shape) != (m, m, m, m) or dets.numel() < 1:
        raise ValueError(f"need ht (m, m), ut (m, m, m, m) and at least one determinant, got {tuple(ht.shape)}, "
                         f"{tuple(ut.shape)}, {tuple(dets.shape)}")
    return dt, ht, ut, dets, m


@_plain
def det_ci_diagonal(ht, ut, dets, N, out=None):
    """``D[I] = <I|H|I>`` (real, fp64) of the determinants ``dets`` (ascending int64 occupation masks of ``N`` bits over
    the m orbitals of ``ht`` (m, m) and the anti-symmetrised ``ut`` (m, m, m, m)) on ``qs_det_ci_diagonal``: the
    preconditioner of a Davidson iteration and the diagonal term ``det_ci_sigma`` takes."""
    lib = _lib.load()
    dt, ht, ut, dets, m = _det_ci_operands(ht, ut, dets)
    dim = dets.numel()
    if out is None:
        out = torch.empty(dim, dtype=_F64, device=dets.device)
    else:
        _check_out(out, (dim,), _F64, "det_ci_diagonal")
    with _on_device_of(ht, ut, dets, out):
        _ran(
            lib.qs_det_ci_diagonal(dtype_code(dt), ht.data_ptr(), ut.data_ptr(), dets.data_ptr(), out.data_ptr(),
                                   m, int(N), dim, _stream()),
            "qs_det_ci_diagonal",
        )
    return out


@_plain
def det_ci_sigma(ht, ut, dets, N, diag, c, out=None):
    """``sigma[k, I] = sum_J <I|H|J> c[k, J]`` on the determinants ``dets`` for ``c`` (K, dim) or (dim,), on
    ``qs_det_ci_sigma``: one walk over every determinant's single and double excitations per group of G vectors,
    ceil(K / G) launches.  ``diag`` is ``det_ci_diagonal(ht, ut, dets, N)``.  The kernel reads ``c`` with the K values
    of a determinant adjacent: a ``c`` that is the transposed view of a contiguous (dim, K) tensor is read in place,
    any other is copied into that layout first.  ``sigma[k]`` has the same bits alone and anywhere in a batch."""
    lib = _lib.load()
    if not isinstance(c, torch.Tensor) or c.dim() not in (1, 2):
        raise ValueError("c must be (K, dim) or (dim,)")
    dt, ht, ut, dets, m = _det_ci_operands(ht, ut, dets, c)
    dim = dets.numel()
    single = c.dim() == 1
    if single:
        c = c[None]
    K = c.shape[0]
    if c.shape[1] != dim or K < 1:
        raise ValueError(f"c has shape {tuple(c.shape)}: need (K, {dim}) with K >= 1")
    ct = _dev(c.transpose(0, 1), dt)                                               # (dim, K), K adjacent
    diag = _dev(diag, _F64)
    if tuple(diag.shape) != (dim,):
        raise ValueError(f"diag has shape {tuple(diag.shape)}: need ({dim},)")
    code = dtype_code(dt)
    nbytes = check(lib.qs_det_ci_workspace(code, code, m, int(N), dim, K), "workspace query")
    if out is None:
        out = torch.empty((dim,) if single else (K, dim), dtype=dt, device=dets.device)
    else:
        _check_out(out, (dim,) if single else (K, dim), dt, "det_ci_sigma")
    with _on_device_of(ht, ut, dets, diag, ct, out):
        _ran(
            lib.qs_det_ci_sigma(code, code, ht.data_ptr(), ut.data_ptr(), dets.data_ptr(), diag.data_ptr(),
                                ct.data_ptr(), out.data_ptr(), m, int(N), dim, K, K, *_work(nbytes, dets.device),
                                _stream()),
            "qs_det_ci_sigma",
        )
    return out


@_plain
def det_ci_density1(dets, c, m, N, out=None):
    """``rho[q, p] = sum_IJ conj(c[I]) <I|a+_p a_q|J> c[J]`` of ONE vector ``c`` (dim,) on the determinants ``dets``
    over ``m`` orbitals (``qs_det_ci_density1``), in the index order ``compute_particle_density(rho_qp)`` takes."""
    lib = _lib.load()
    _dets_checked(dets)
    dt = result_dtype(c)
    c, dets = _dev(c, dt), _dev(dets)
    dim = dets.numel()
    if tuple(c.shape) != (dim,) or dim < 1:
        raise ValueError(f"c has shape {tuple(c.shape)}: need ({dim},), one vector")
    m = int(m)
    if out is None:
        out = torch.empty((m, m) if 1 <= m <= 63 else (0, 0), dtype=dt, device=dets.device)
    else:
        _check_out(out, (m, m), dt, "det_ci_density1")
    with _on_device_of(dets, c, out):
        _ran(
            lib.qs_det_ci_density1(dtype_code(dt), dets.data_ptr(), c.data_ptr(), out.data_ptr(), m, int(N), dim,
                                   _stream()),
            "qs_det_ci_density1",
        )
    return out


def _det_ci_pair(dets, bra, ket, m, what):
    """Device operands of the transition densities: ``dets`` int64 and two vectors (dim,) in one dtype."""
    _dets_checked(dets)
    dt = result_dtype(bra, ket)
    same = bra is ket
    bra, dets = _dev(bra, dt), _dev(dets)
    ket = bra if same else _dev(ket, dt)
    dim = dets.numel()
    if tuple(bra.shape) != (dim,) or tuple(ket.shape) != (dim,) or dim < 1:
        raise ValueError(f"{what}: bra and ket have shapes {tuple(bra.shape)}, {tuple(ket.shape)}: need ({dim},) each")
    return dt, dets, bra, ket, dim, int(m)


@_plain
def det_ci_transition_density1(dets, bra, ket, m, N, out=None):
    """``rho[q, p] = sum_IJ conj(bra[I]) <I|a+_p a_q|J> ket[J]`` of two vectors (dim,) on the determinants ``dets`` over
    ``m`` orbitals (``qs_det_ci_transition_density1``): the kernel of ``det_ci_density1`` with a second vector, and with
    ``bra is ket`` its bits.  A real and a complex vector promote to complex128."""
    lib = _lib.load()
    dt, dets, bra, ket, dim, m = _det_ci_pair(dets, bra, ket, m, "det_ci_transition_density1")
    if out is None:
        out = torch.empty((m, m) if 1 <= m <= 63 else (0, 0), dtype=dt, device=dets.device)
    else:
        _check_out(out, (m, m), dt, "det_ci_transition_density1")
    with _on_device_of(dets, bra, ket, out):
        _ran(
            lib.qs_det_ci_transition_density1(dtype_code(dt), dets.data_ptr(), bra.data_ptr(), ket.data_ptr(),
                                              out.data_ptr(), m, int(N), dim, _stream()),
            "qs_det_ci_transition_density1",
        )
    return out


@_plain
def det_ci_density2(dets, bra, ket, m, N, out=None):
    """``gamma2[p, q, r, s] = sum_IJ conj(bra[I]) <I|a+_p a+_q a_s a_r|J> ket[J]`` (m, m, m, m) of two vectors (dim,) on the
    determinants ``dets`` (``qs_det_ci_density2``): ``bra is ket`` gives the two-body density of a state.  With
    ``det_ci_transition_density1`` ``<bra|H|ket> = sum ht[p,q] rho[q,p] + 1/4 sum ut[p,q,r,s] gamma2[p,q,r,s]``.  Every
    element is written; the anti-symmetry in (p, q) and in (r, s) is exact and repeated calls give the same bits."""
    lib = _lib.load()
    dt, dets, bra, ket, dim, m = _det_ci_pair(dets, bra, ket, m, "det_ci_density2")
    if out is None:
        out = torch.empty((m, m, m, m) if 1 <= m <= 63 else (0, 0, 0, 0), dtype=dt, device=dets.device)
    else:
        _check_out(out, (m, m, m, m), dt, "det_ci_density2")
    with _on_device_of(dets, bra, ket, out):
        _ran(
            lib.qs_det_ci_density2(dtype_code(dt), dets.data_ptr(), bra.data_ptr(), ket.data_ptr(), out.data_ptr(),
                                   m, int(N), dim, _stream()),
            "qs_det_ci_density2",
        )
    return out


# Byte budget of the D and G panels of ONE qs_string_ci_sigma call: ``string_ci_sigma`` sends a batch in groups of as
# many vectors as fit it, and where one vector alone is over it, in passes over as many alpha rows of that vector's D
# and G as fit it (``qs_string_ci_sigma_rows``, at least one row); also of the two panels of one pass of
# ``string_ci_density2`` and of ``string_ci_density2_spin``, which take as many alpha rows per pass as fit it (at least
# one).  The tuning key
# ``string_ci_bytes`` overrides it for the calling thread.
STRING_CI_BYTES = 2 << 30


def string_ci_budget():
    """The byte budget in force on the calling thread -- the tuning key ``string_ci_bytes`` where it is set, else
    ``STRING_CI_BYTES`` --, read off ``qs_string_ci_group`` on lists of one string, whose two panels are 32 bytes per
    vector: exact to 32 bytes, at most 64 GiB."""
    return 32 * check(_lib.load().qs_string_ci_group(QS_F64, QS_F64, 1, 1, 1, (1 << 31) - 1, STRING_CI_BYTES), "group query")


def _strings_checked(strings, what):
    if not isinstance(strings, torch.Tensor) or strings.dtype != torch.int64 or strings.dim() != 1 or strings.numel() < 1:
        raise ValueError(f"{what} must be a non-empty 1-D int64 tensor of occupation strings")
    return _dev(strings)


def _string_tables(ta, tb, m):
    """The two replacement tables (n, m^2) int32 of the string kernels; the SAME tensor twice stays one."""
    for t in (ta, tb):
        if not isinstance(t, torch.Tensor) or t.dtype != torch.int32 or t.dim() != 2 or t.shape[1] != m * m or t.shape[0] < 1:
            raise ValueError(f"a replacement table must be an (n, {m * m}) int32 tensor (string_ci_table)")
    same = ta is tb
    ta = _dev(ta)
    return ta, (ta if same else _dev(tb))


@_plain
def string_ci_table(strings, m, N, out=None):
    """Replacement table ``T[K, p m + q]`` (n, m^2) int32 of the ascending int64 occupation ``strings`` (``N`` bits over
    ``m`` spatial orbitals) on ``qs_string_ci_table``: ``+-(index of J + 1)`` where ``<K|E_pq|J> = +-1``, 0 where the
    replacement is empty or its target is not in the list."""
    lib = _lib.load()
    strings = _strings_checked(strings, "strings")
    n, m = strings.numel(), int(m)
    if out is None:
        out = torch.empty((n, m * m) if 1 <= m <= 63 else (0, 0), dtype=torch.int32, device=strings.device)
    else:
        _check_out(out, (n, m * m), torch.int32, "string_ci_table")
    with _on_device_of(strings, out):
        _ran(lib.qs_string_ci_table(strings.data_ptr(), n, m, int(N), out.data_ptr(), _stream()), "qs_string_ci_table")
    return out


@_plain
def string_ci_diagonal(ht, ut, strings_a, Na, strings_b, Nb, out=None):
    """``D[Ia, Ib] = <I|H|I>`` (na, nb), real fp64, of the determinants of two string lists over the m spatial orbitals of
    ``ht`` (m, m) and the plain ``ut = <pq|rs>`` (m, m, m, m), on ``qs_string_ci_diagonal``."""
    lib = _lib.load()
    dt = result_dtype(ht, ut)
    ht, ut = _dev(ht, dt), _dev(ut, dt)
    sa, sb = _strings_checked(strings_a, "strings_a"), _strings_checked(strings_b, "strings_b")
    m = ht.shape[-1]
    if tuple(ht.shape) != (m, m) or tuple(ut.shape) != (m, m, m, m):
        raise ValueError(f"need ht (m, m) and ut (m, m, m, m), got {tuple(ht.shape)}, {tuple(ut.shape)}")
    na, nb = sa.numel(), sb.numel()
    if out is None:
        out = torch.empty((na, nb), dtype=_F64, device=sa.device)
    else:
        _check_out(out, (na, nb), _F64, "string_ci_diagonal")
    with _on_device_of(ht, ut, sa, sb, out):
        _ran(
            lib.qs_string_ci_diagonal(dtype_code(dt), ht.data_ptr(), ut.data_ptr(), sa.data_ptr(), na, int(Na),
                                      sb.data_ptr(), nb, int(Nb), m, out.data_ptr(), _stream()),
            "qs_string_ci_diagonal",
        )
    return out


def string_ci_sigma_plan(m, na, nb, c_dtype, K=1, h_dtype=None):
    """``(rows, passes, columns, work_bytes)`` of ``qs_string_ci_sigma_rows`` on ``K`` vectors of ``c_dtype`` (``h_dtype``:
    the dtype of ``k`` and ``W``, default the same) under ``STRING_CI_BYTES`` or the calling thread's ``string_ci_bytes``:
    alpha rows per pass, passes, columns of one pass's product, workspace bytes.  ``passes == 1`` exactly where the D
    and G of the K vectors fit the budget; ``string_ci_sigma`` takes the passes where one vector does not."""
    plan = (ctypes.c_int64 * 4)()
    hcode = dtype_code(c_dtype if h_dtype is None else h_dtype)
    check(_lib.load().qs_string_ci_sigma_plan(hcode, dtype_code(c_dtype), int(m), int(na), int(nb), int(K), STRING_CI_BYTES,
                                              ctypes.addressof(plan)), "plan query")
    return tuple(plan)


def _sigma_operands(k, W, ta, tb, c, out, dims, name):
    """The operands of a sigma on the device: ``k`` (m, m), ``W`` (m^2, m^2), the tables, ``c`` as (K, na, nb) and the
    result buffer in the same view.  Returns ``(k, W, ta, tb, c3, out, o3, hcode, ccode)``."""
    if not isinstance(c, torch.Tensor) or c.dim() not in (2, 3):
        raise ValueError(f"c must be (K, {dims}) or ({dims})")
    hdt = result_dtype(k, W)
    dt = result_dtype(k, W, c)
    k, W, c = _dev(k, hdt), _dev(W, hdt), _dev(c, dt)
    m = k.shape[-1]
    if tuple(k.shape) != (m, m) or tuple(W.shape) != (m * m, m * m):
        raise ValueError(f"need k (m, m) and W (m^2, m^2), got {tuple(k.shape)}, {tuple(W.shape)}")
    ta, tb = _string_tables(ta, tb, m)
    single = c.dim() == 2
    c3 = c[None] if single else c
    if tuple(c3.shape[1:]) != (ta.shape[0], tb.shape[0]) or c3.shape[0] < 1:
        raise ValueError(f"c has shape {tuple(c.shape)}: need (K, {ta.shape[0]}, {tb.shape[0]}) with K >= 1")
    if out is None:
        out = torch.empty(tuple(c.shape), dtype=dt, device=c.device)
    else:
        _check_out(out, tuple(c.shape), dt, name)
    return k, W, ta, tb, c3, out, (out[None] if single else out), dtype_code(hdt), dtype_code(dt)


@_plain
def string_ci_sigma(k, W, ta, tb, c, out=None):
    """``sigma[j] = H c[j]`` for ``c`` (K, na, nb) or (na, nb) on ``qs_string_ci_sigma``: ``k`` (m, m) and ``W``
    (m^2, m^2) as in ``include/qs_amd.h``, ``ta`` (na, m^2) and ``tb`` (nb, m^2) from ``string_ci_table``.  Per group of
    vectors one expand, ONE product ``W . D`` on the product dispatcher and one fold; the groups are as large as
    ``STRING_CI_BYTES`` of workspace allow.  A real ``k`` and ``W`` with a complex ``c`` stay real (fp64 product on the
    re / im pairs).  Where the D and G of ONE vector are over the budget, each vector goes to
    ``qs_string_ci_sigma_rows`` instead: passes over as many alpha rows of the intermediate as fit, which add into
    ``sigma`` on the stream.  Repeating a call gives the same bits; another grouping or another budget agrees to
    rounding.  One ``dispatch_log`` entry names the kernels of the whole call."""
    lib = _lib.load()
    k, W, ta, tb, c3, out, o3, hcode, ccode = _sigma_operands(k, W, ta, tb, c, out, "na, nb", "string_ci_sigma")
    m, (K, na, nb) = k.shape[-1], c3.shape
    group = check(lib.qs_string_ci_group(hcode, ccode, m, na, nb, K, STRING_CI_BYTES), "group query")
    ran = []
    # one vector alone is over the budget: passes over alpha rows (qs_string_ci_sigma_rows), one vector per call, so that
    # the fold's extra walks of the alpha table and round trips of sigma stay linear in K
    _, passes, _, rows_bytes = string_ci_sigma_plan(m, na, nb, c3.dtype, 1, k.dtype)
    if passes > 1:
        group = 1
    with _on_device_of(k, W, ta, tb, c3, out):
        for k0 in range(0, K, group):
            kg = min(group, K - k0)
            args = (hcode, ccode, k.data_ptr(), W.data_ptr(), ta.data_ptr(), tb.data_ptr(), m, na, nb,
                    c3[k0:k0 + kg].data_ptr(), kg, o3[k0:k0 + kg].data_ptr())
            if passes > 1:
                check(lib.qs_string_ci_sigma_rows(*args, *_work(rows_bytes, c3.device), STRING_CI_BYTES, _stream()),
                      "qs_string_ci_sigma_rows")
            else:
                nbytes = check(lib.qs_string_ci_workspace(hcode, ccode, m, na, nb, kg), "workspace query")
                check(lib.qs_string_ci_sigma(*args, *_work(nbytes, c3.device), _stream()), "qs_string_ci_sigma")
            if dispatch_log is not None:
                ran.append(lib.qs_last_dispatch().decode())
    if dispatch_log is not None:
        dispatch_log.append(" | ".join(ran))
    return out


def _sym_plan(hcode, ccode, m, n, K, bounds=False):
    """``(rc, plan, boundaries)`` of ``qs_string_ci_sigma_sym_plan``; the boundaries only where asked for."""
    lib = _lib.load()
    plan = (ctypes.c_int64 * 4)()
    rc = lib.qs_string_ci_sigma_sym_plan(hcode, ccode, int(m), int(n), int(K), STRING_CI_BYTES, ctypes.addressof(plan), None, 0)
    if rc or not bounds:
        return rc, tuple(plan), None
    cuts = (ctypes.c_int64 * (plan[0] + 1))()
    rc = lib.qs_string_ci_sigma_sym_plan(hcode, ccode, int(m), int(n), int(K), STRING_CI_BYTES, ctypes.addressof(plan),
                                         ctypes.addressof(cuts), len(cuts))
    return rc, tuple(plan), tuple(cuts)


def string_ci_sigma_sym_plan(m, n, c_dtype, K=1, h_dtype=None):
    """``((passes, longest, columns, work_bytes), boundaries)`` of ``qs_string_ci_sigma_sym`` on ``K`` vectors (n, n) of
    ``c_dtype`` (``h_dtype``: the dtype of ``k`` and ``W``, default the same) under ``STRING_CI_BYTES`` or the calling
    thread's ``string_ci_bytes``: the passes over packed rows, the largest packed length ``off(b[i+1]) - off(b[i])`` with
    ``off(r) = r (r + 1) / 2``, the columns of the largest product, the workspace bytes, and the ``passes + 1`` row
    boundaries ``b``, greedy from row 0."""
    hcode = dtype_code(c_dtype if h_dtype is None else h_dtype)
    rc, plan, cuts = _sym_plan(hcode, dtype_code(c_dtype), m, n, K, bounds=True)
    check(rc, "plan query")
    return plan, cuts


@_plain
def string_ci_sigma_sym(k, W, t, c, parity, out=None):
    """``sigma[j] = H c[j]`` for vectors of definite parity under the exchange of the two spins,
    ``c[j] == parity * c[j].T`` with ``parity = +-1``, on ``qs_string_ci_sigma_sym``: ``c`` (K, n, n) or (n, n), ONE
    table ``t`` (n, m^2) for both spins, ``k`` and ``W`` as for ``string_ci_sigma``.  Only the lower triangle of the
    expanded intermediate is formed -- half of the expand, of the product and of the fold's gathers, half of the
    workspace --, in passes over packed rows under ``STRING_CI_BYTES``; ``c`` and the result are full arrays, and the
    result has the parity bit for bit.  The parity of ``c`` is NOT checked: for another ``c`` the result is
    deterministic and unspecified (``StringCI.sigma`` symmetrises first).  All K vectors go in one call where their
    plan is one pass; else, where one vector is one pass, in groups of the largest size whose plan is; else one vector
    per call, for the reason given at ``string_ci_sigma``.  One ``dispatch_log`` entry names the kernels of the whole
    call."""
    lib = _lib.load()
    if parity not in (1, -1):
        raise ValueError(f"parity must be +1 or -1, got {parity!r}")
    k, W, t, _, c3, out, o3, hcode, ccode = _sigma_operands(k, W, t, t, c, out, "n, n", "string_ci_sigma_sym")
    m, K, n = k.shape[-1], c3.shape[0], t.shape[0]

    def one_pass(g):
        rc, plan, _ = _sym_plan(hcode, ccode, m, n, g)
        return rc == 0 and plan[0] == 1

    check(_sym_plan(hcode, ccode, m, n, 1)[0], "plan query")              # the extents of one vector
    group = 1
    if one_pass(K):
        group = K
    elif one_pass(1):
        lo, hi = 1, K                                                     # one_pass(lo) holds, one_pass(hi) does not
        while hi - lo > 1:
            mid = (lo + hi) // 2
            lo, hi = (mid, hi) if one_pass(mid) else (lo, mid)
        group = lo
    ran = []
    with _on_device_of(k, W, t, c3, out):
        for k0 in range(0, K, group):
            kg = min(group, K - k0)
            rc, plan, _ = _sym_plan(hcode, ccode, m, n, kg)
            check(rc, "plan query")
            check(lib.qs_string_ci_sigma_sym(hcode, ccode, k.data_ptr(), W.data_ptr(), t.data_ptr(), m, n, int(parity),
                                             c3[k0:k0 + kg].data_ptr(), kg, o3[k0:k0 + kg].data_ptr(),
                                             *_work(plan[3], c3.device), STRING_CI_BYTES, _stream()), "qs_string_ci_sigma_sym")
            if dispatch_log is not None:
                ran.append(lib.qs_last_dispatch().decode())
    if dispatch_log is not None:
        dispatch_log.append(" | ".join(ran))
    return out


def _bra_ket(ta, tb, m, bra, ket):
    """The operands of a density on the device: the tables and two vectors (na, nb) of one dtype; ``bra is ket`` stays one
    tensor.  Returns ``(m, ta, tb, bra, ket, na, nb, dtype, dtype code)``."""
    m = int(m)
    ta, tb = _string_tables(ta, tb, m)
    dt = result_dtype(bra, ket)
    same = bra is ket
    bra = _dev(bra, dt)
    ket = bra if same else _dev(ket, dt)
    na, nb = ta.shape[0], tb.shape[0]
    if tuple(bra.shape) != (na, nb) or tuple(ket.shape) != (na, nb):
        raise ValueError(f"bra and ket have shapes {tuple(bra.shape)}, {tuple(ket.shape)}: need ({na}, {nb}) each")
    code = dtype_code(dt)
    return m, ta, tb, bra, ket, na, nb, dt, code


@_plain
def string_ci_density1(ta, tb, m, bra, ket, out=None):
    """Spin-summed ``rho[q, p] = <bra| E_pq |ket>`` (m, m) of two vectors (na, nb) on ``qs_string_ci_density1``: one
    expand of ``ket`` and one fixed-order sum per element; ``bra is ket`` is the density of a state, in the index order
    ``compute_particle_density(rho_qp)`` takes."""
    lib = _lib.load()
    m, ta, tb, bra, ket, na, nb, dt, code = _bra_ket(ta, tb, m, bra, ket)
    nbytes = check(lib.qs_string_ci_workspace(code, code, m, na, nb, 1), "workspace query")
    if out is None:
        out = torch.empty((m, m), dtype=dt, device=bra.device)
    else:
        _check_out(out, (m, m), dt, "string_ci_density1")
    with _on_device_of(ta, tb, bra, ket, out):
        _ran(
            lib.qs_string_ci_density1(code, ta.data_ptr(), tb.data_ptr(), m, na, nb, bra.data_ptr(), ket.data_ptr(),
                                      out.data_ptr(), *_work(nbytes, bra.device), _stream()),
            "qs_string_ci_density1",
        )
    return out


def _string_ci_density2(entry, ngamma, nrho, outs, ta, tb, m, bra, ket, out):
    """Either two-body density on ``qs_<entry>``: the operands, the workspace query, ``out`` -- a tuple of ``ngamma``
    buffers (m, m, m, m) and ``nrho`` buffers (m, m), allocated here or checked; ``outs`` names it in the error -- and the
    call.  Returns the tuple."""
    lib = _lib.load()
    m, ta, tb, bra, ket, na, nb, dt, code = _bra_ket(ta, tb, m, bra, ket)
    nbytes = check(getattr(lib, f"qs_{entry}_workspace")(code, m, na, nb, STRING_CI_BYTES), "workspace query")
    shapes = ((m, m, m, m),) * ngamma + ((m, m),) * nrho
    if out is None:
        out = tuple(torch.empty(shape, dtype=dt, device=bra.device) for shape in shapes)
    else:
        if not isinstance(out, (tuple, list)) or len(out) != len(shapes):
            raise ValueError(f"{entry}: `out` must be {outs}")
        out = tuple(_check_out(o, shape, dt, entry) for o, shape in zip(out, shapes))
    with _on_device_of(ta, tb, bra, ket, *out):
        _ran(
            getattr(lib, f"qs_{entry}")(code, ta.data_ptr(), tb.data_ptr(), m, na, nb, bra.data_ptr(), ket.data_ptr(),
                                        *(o.data_ptr() for o in out), *_work(nbytes, bra.device), STRING_CI_BYTES, _stream()),
            f"qs_{entry}",
        )
    return out


@_plain
def string_ci_density2(ta, tb, m, bra, ket, out=None):
    """``(gamma, rho)`` of two vectors (na, nb) on ``qs_string_ci_density2``: the spin-summed two-body density
    ``gamma[p, q, r, s] = sum_spins <bra| a+_p a+_q a_s a_r |ket>`` (m, m, m, m) and ``rho[q, p] = <bra| E_pq |ket>``
    (m, m) from the same pass; ``bra is ket`` is a state.  The expanded panels are cut into passes over alpha rows that
    fit ``STRING_CI_BYTES`` (tuning key ``string_ci_bytes``); every pass is one batched product on the product
    dispatcher.  With the plain ``ut``, ``<bra|H|ket> = sum ht[p,q] rho[q,p] + 1/2 sum ut[p,q,r,s] gamma[p,q,r,s]``.
    ``out`` is a pair ``(gamma, rho)`` of buffers.  Repeating a call gives the same bits; another budget agrees to
    rounding."""
    return _string_ci_density2("string_ci_density2", 1, 1, "a pair (gamma, rho)", ta, tb, m, bra, ket, out)


def string_ci_density2_spin_plan(m, na, nb, c_dtype):
    """``(rows, passes, T, kc, work_bytes)`` of ``qs_string_ci_density2_spin`` on vectors of ``c_dtype`` under
    ``STRING_CI_BYTES`` or the calling thread's ``string_ci_bytes``: alpha rows per pass, passes, slices of ``kc``
    determinants per pass, workspace bytes."""
    plan = (ctypes.c_int64 * 5)()
    check(_lib.load().qs_string_ci_density2_spin_plan(dtype_code(c_dtype), int(m), int(na), int(nb), STRING_CI_BYTES,
                                                      ctypes.addressof(plan)), "qs_string_ci_density2_spin_plan")
    return tuple(int(x) for x in plan)


@_plain
def string_ci_density2_spin(ta, tb, m, bra, ket, out=None):
    """``(gamma_aa, gamma_ab, gamma_bb, rho_a, rho_b)`` of two vectors (na, nb) on ``qs_string_ci_density2_spin``: the
    spin-resolved two-body densities ``gamma_st[p, q, r, s] = <bra| a+_ps a+_qt a_st a_rs |ket>`` (m, m, m, m) and the
    one-body densities ``rho_s[q, p] = <bra| a+_ps a_qs |ket>`` (m, m) from the same passes; ``bra is ket`` is a state.
    The beta-alpha block is ``gamma_ab.permute(1, 0, 3, 2)``; the four blocks add up to ``string_ci_density2``'s
    ``gamma``, the two ``rho`` to its ``rho``.  Passes and budget as there (``STRING_CI_BYTES``, tuning key
    ``string_ci_bytes``); every pass is two batched products on the product dispatcher.  ``out`` is a 5-tuple of
    buffers.  Repeating a call gives the same bits; another budget agrees to rounding."""
    return _string_ci_density2("string_ci_density2_spin", 3, 2, "a 5-tuple (gamma_aa, gamma_ab, gamma_bb, rho_a, rho_b)", ta, tb, m,
                               bra, ket, out)


@_plain
def string_ci_spin_squared(ta, tb, m, Na, Nb, c, out=None):
    """``out[k] = S^2 c[k]`` for ``c`` (K, na, nb) or (na, nb) with ``Na`` alpha and ``Nb`` beta particles on
    ``qs_string_ci_spin_squared``: ``S^2 = S_z (S_z + 1) + N_beta - sum_pq E^alpha_qp E^beta_pq`` as one gather through
    both replacement tables per (p, q).  On a truncated list a missing target contributes nothing."""
    lib = _lib.load()
    m = int(m)
    ta, tb = _string_tables(ta, tb, m)
    if not isinstance(c, torch.Tensor) or c.dim() not in (2, 3):
        raise ValueError("c must be (K, na, nb) or (na, nb)")
    dt = result_dtype(c)
    c = _dev(c, dt)
    na, nb = ta.shape[0], tb.shape[0]
    K = 1 if c.dim() == 2 else c.shape[0]
    if tuple(c.shape[-2:]) != (na, nb) or K < 1:
        raise ValueError(f"c has shape {tuple(c.shape)}: need (K, {na}, {nb}) with K >= 1")
    if out is None:
        out = torch.empty(tuple(c.shape), dtype=dt, device=c.device)
    else:
        _check_out(out, tuple(c.shape), dt, "string_ci_spin_squared")
    with _on_device_of(ta, tb, c, out):
        _ran(
            lib.qs_string_ci_spin_squared(dtype_code(dt), ta.data_ptr(), tb.data_ptr(), m, na, nb, int(Na), int(Nb),
                                          c.data_ptr(), K, out.data_ptr(), _stream()),
            "qs_string_ci_spin_squared",
        )
    return out


@_plain
def string_ci_one_body(A_up, ta, tb, m, c, A_down=None, out=None):
    """``out[x, k] = (sum_pq A_up[x,p,q] E^alpha_pq + A_down[x,p,q] E^beta_pq) c[k]`` on ``qs_string_ci_one_body``: ``A_up``
    (m, m) or (d, m, m), ``c`` (na, nb) or (K, na, nb); the result has the leading axis of ``A_up`` (if present), then that of
    ``c`` (if present), then (na, nb).  ``A_down=None`` is the spin-free operator ``sum_pq A[p,q] E_pq``.  One gather
    through the replacement tables, no intermediate and no workspace.  The result is complex if ``A`` or ``c`` is; a real
    ``A`` with a complex ``c`` stays real, a real ``c`` under a complex ``A`` is converted once.  Repeating a call gives the
    same bits."""
    lib = _lib.load()
    m = int(m)
    ta, tb = _string_tables(ta, tb, m)
    if not isinstance(c, torch.Tensor) or c.dim() not in (2, 3):
        raise ValueError("c must be (K, na, nb) or (na, nb)")
    ops = (A_up,) if A_down is None else (A_up, A_down)
    hdt = result_dtype(*ops)
    dt = result_dtype(*ops, c)
    A_up = _dev(A_up, hdt)
    if A_up.dim() not in (2, 3) or tuple(A_up.shape[-2:]) != (m, m) or A_up.shape[0] < 1:
        raise ValueError(f"A_up has shape {tuple(A_up.shape)}: need ({m}, {m}) or (d, {m}, {m}) with d >= 1")
    if A_down is not None:
        A_down = _dev(A_down, hdt)
        if tuple(A_down.shape) != tuple(A_up.shape):
            raise ValueError(f"A_down has shape {tuple(A_down.shape)}: need that of A_up, {tuple(A_up.shape)}")
    c = _dev(c, dt)
    na, nb = ta.shape[0], tb.shape[0]
    K = 1 if c.dim() == 2 else c.shape[0]
    d = 1 if A_up.dim() == 2 else A_up.shape[0]
    if tuple(c.shape[-2:]) != (na, nb) or K < 1:
        raise ValueError(f"c has shape {tuple(c.shape)}: need (K, {na}, {nb}) with K >= 1")
    shape = tuple(A_up.shape[:-2]) + tuple(c.shape[:-2]) + (na, nb)
    if out is None:
        out = torch.empty(shape, dtype=dt, device=c.device)
    else:
        _check_out(out, shape, dt, "string_ci_one_body")
    with _on_device_of(A_up, *(() if A_down is None else (A_down,)), ta, tb, c, out):
        _ran(
            lib.qs_string_ci_one_body(dtype_code(hdt), dtype_code(dt), A_up.data_ptr(), None if A_down is None else A_down.data_ptr(),
                                      d, ta.data_ptr(), tb.data_ptr(), m, na, nb, c.data_ptr(), K, out.data_ptr(), _stream()),
            "qs_string_ci_one_body",
        )
    return out


@_plain
def string_ci_ladder_table(target, source, m, out=None):
    """Ladder table ``L[J, p]`` (n_t, m) int32 between two ascending int64 string lists of ONE spin on
    ``qs_string_ci_ladder_table``: ``+-(index in source of target[J] ^ bit p, plus 1)`` with the sign
    ``(-1)^(bits of target[J] below p)``, 0 where that string is not in ``source``.  A ``source`` one particle richer than
    ``target`` gives the table of annihilation, one a particle poorer that of creation."""
    lib = _lib.load()
    target, source = _strings_checked(target, "target"), _strings_checked(source, "source")
    n_t, m = target.numel(), int(m)
    if out is None:
        out = torch.empty((n_t, m) if 1 <= m <= 63 else (0, 0), dtype=torch.int32, device=target.device)
    else:
        _check_out(out, (n_t, m), torch.int32, "string_ci_ladder_table")
    with _on_device_of(target, source, out):
        _ran(lib.qs_string_ci_ladder_table(target.data_ptr(), n_t, source.data_ptr(), source.numel(), m, out.data_ptr(), _stream()),
             "qs_string_ci_ladder_table")
    return out


@_plain
def string_ci_ladder(phi, table, spin, n_alpha, c, out=None):
    """``out[x, k] = sum_p phi[x, p] a_p c[k]`` or ``sum_p phi[x, p] a+_p c[k]`` for the particles of ``spin`` (0: alpha, 1:
    beta) on ``qs_string_ci_ladder``: ``table`` (n_t, m) from ``string_ci_ladder_table`` decides which, ``phi`` is (m,) or
    (d, m) and is not conjugated, ``c`` (na, nb) or (K, na, nb) lives on the source lists, ``n_alpha`` is the number of
    alpha particles (the sign a beta ladder picks up).  The result has the leading axis of ``phi`` (if present), then that
    of ``c`` (if present), then (n_t, nb) for alpha or (na, n_t) for beta.  No intermediate, no workspace.  The result is
    complex if ``phi`` or ``c`` is; a real ``phi`` with a complex ``c`` stays real, a real ``c`` under a complex ``phi`` is
    converted once.  Repeating a call gives the same bits."""
    lib = _lib.load()
    spin = int(spin)
    if spin not in (0, 1):
        raise ValueError(f"spin must be 0 (alpha) or 1 (beta), got {spin}")
    if not isinstance(table, torch.Tensor) or table.dtype != torch.int32 or table.dim() != 2 or table.shape[0] < 1:
        raise ValueError("a ladder table must be an (n_t, m) int32 tensor (string_ci_ladder_table)")
    if not isinstance(c, torch.Tensor) or c.dim() not in (2, 3):
        raise ValueError("c must be (K, na, nb) or (na, nb)")
    n_t, m = table.shape
    hdt = result_dtype(phi)
    dt = result_dtype(phi, c)
    phi, table, c = _dev(phi, hdt), _dev(table), _dev(c, dt)
    if phi.dim() not in (1, 2) or phi.shape[-1] != m or phi.shape[0] < 1:
        raise ValueError(f"phi has shape {tuple(phi.shape)}: need ({m},) or (d, {m}) with d >= 1")
    na, nb = c.shape[-2:]
    K = 1 if c.dim() == 2 else c.shape[0]
    d = 1 if phi.dim() == 1 else phi.shape[0]
    if K < 1 or na < 1 or nb < 1:
        raise ValueError(f"c has shape {tuple(c.shape)}: need (K, na, nb) with K, na, nb >= 1")
    shape = tuple(phi.shape[:-1]) + tuple(c.shape[:-2]) + ((n_t, nb) if spin == 0 else (na, n_t))
    if out is None:
        out = torch.empty(shape, dtype=dt, device=c.device)
    else:
        _check_out(out, shape, dt, "string_ci_ladder")
    with _on_device_of(phi, table, c, out):
        _ran(
            lib.qs_string_ci_ladder(dtype_code(hdt), dtype_code(dt), phi.data_ptr(), d, spin, table.data_ptr(), m, int(n_alpha), na, nb,
                                    n_t, c.data_ptr(), K, out.data_ptr(), _stream()),
            "qs_string_ci_ladder",
        )
    return out


@_plain
def transform_two_body_blocks(u, Ct0, Ct1, C2, C3, out=None):
    """``out[pqrs] = Ct0[pa] Ct1[qb] u[abcd] C2[cr] C3[ds]``: one coefficient matrix per index
    (``qs_transform_two_body_blocks``), contracted in the order a, b, d, c so that small blocks in front shrink the
    tensor first -- ``<ij|ab>`` costs one read of ``u``.  ``Ct0`` (M0, L) and ``Ct1`` (M1, L) are bra ROWS, ``C2``
    (L, M2) and ``C3`` (L, M3) ket COLUMNS.  A real ``u`` against complex coefficients stays real."""
    lib = _lib.load()
    dt = result_dtype(u, Ct0, Ct1, C2, C3)
    udt = _F64 if isinstance(u, torch.Tensor) and u.dtype == _F64 else dt
    u = _dev(u, udt)
    Ct0, Ct1, C2, C3 = _dev(Ct0, dt), _dev(Ct1, dt), _dev(C2, dt), _dev(C3, dt)
    if u.dim() != 4 or any(c.dim() != 2 for c in (Ct0, Ct1, C2, C3)):
        raise ValueError("u must be (L, L, L, L) and the coefficient blocks 2-D")
    L = u.shape[0]
    M0, M1, M2, M3 = Ct0.shape[0], Ct1.shape[0], C2.shape[1], C3.shape[1]
    if tuple(u.shape) != (L, L, L, L) or not (Ct0.shape[1] == Ct1.shape[1] == C2.shape[0] == C3.shape[0] == L):
        raise ValueError(
            f"u {tuple(u.shape)}, bras {tuple(Ct0.shape)} {tuple(Ct1.shape)}, kets {tuple(C2.shape)} {tuple(C3.shape)}: "
            "need u (L,L,L,L), bras (M0,L) (M1,L) and kets (L,M2) (L,M3)")
    ucode, code = dtype_code(udt), dtype_code(dt)
    nbytes = check(lib.qs_transform_two_body_blocks_workspace(ucode, code, L, M0, M1, M2, M3), "workspace query")
    if out is None:
        out = torch.empty((M0, M1, M2, M3), dtype=dt, device=u.device)
    else:
        _check_out(out, (M0, M1, M2, M3), dt, "transform_two_body_blocks")
    with _on_device_of(u, Ct0, Ct1, C2, C3, out):
        work = workspace.get(nbytes, u.device)
        _ran(
            lib.qs_transform_two_body_blocks(
                ucode, code, u.data_ptr(), Ct0.data_ptr(), Ct1.data_ptr(), C2.data_ptr(), C3.data_ptr(), out.data_ptr(),
                work.data_ptr(), work.numel(), L, M0, M1, M2, M3, _stream(),
            ),
            "qs_transform_two_body_blocks",
        )
    return out


class CholeskyState:
    """What a run of ``cholesky_two_body`` leaves behind and a later call continues from: the vector buffer
    ``(capacity, m, m)``, the residual diagonal ``(m*m,)``, the pivots ``(capacity,)`` int64 and the rank."""

    __slots__ = ("vectors", "diag", "pivots", "rank")

    def __init__(self, vectors, diag, pivots, rank):
        self.vectors, self.diag, self.pivots, self.rank = vectors, diag, pivots, rank

    @property
    def capacity(self):
        return self.vectors.shape[0]


@_plain
def cholesky_two_body(u, tol, max_rank=None, state=None):
    """Pivoted Cholesky vectors of the two-body tensor (``qs_cholesky_two_body``): ``L`` with

        u[p,q,r,s] = sum_x conj(L[x,r,p]) L[x,q,s]   to within ``tol`` per element,

    for a plain (not anti-symmetrised) ``u`` (m, m, m, m) whose ``G[(r,p),(q,s)] = u[p,q,r,s]`` is Hermitian positive
    semidefinite; ``u`` is read in place.  The run stops when the largest residual diagonal is ``<= tol`` or at
    ``max_rank`` vectors (the capacity of the buffer; default ``min(8 m, m*m)``).  With ``state`` (of an earlier call on
    the same ``u`` and ``tol``) the run CONTINUES from ``state.rank``; a ``max_rank`` above the state's capacity moves
    the vectors to a larger buffer first.  The bits do not depend on where a run was interrupted.

    Returns ``(L, pivots, (dmax, dmin), state)``: views ``(rank, m, m)`` and ``(rank,)`` of the state's buffers, the
    largest and the smallest residual diagonal at exit, and the state.  A NaN on the residual diagonal ends the run at
    the next pivot with ``dmax`` NaN (``cholesky.decompose`` raises on it).  The call blocks (one read-back of the device's
    stop flag per ``qs_cholesky_two_body_block()`` steps)."""
    lib = _lib.load()
    if not isinstance(u, torch.Tensor):
        raise TypeError("expected a torch.Tensor")
    dt = _C128 if u.dtype in (torch.complex64, _C128) else _F64
    u = _dev(u, dt)
    if u.dim() != 4 or len(set(u.shape)) != 1:
        raise ValueError(f"u must be (m, m, m, m), got {tuple(u.shape)}")
    m = u.shape[0]
    n = m * m
    have = 0 if state is None else state.capacity
    cap = max(have, min(8 * m, n)) if max_rank is None else int(max_rank)
    if cap < 1 or (state is not None and cap < state.rank):
        raise ValueError(f"max_rank = {cap} must be at least 1 and at least the rank of the state")
    code = dtype_code(dt)
    nbytes = check(lib.qs_cholesky_two_body_workspace(code, m, cap), "workspace query")
    if state is None:
        state = CholeskyState(torch.empty((cap, m, m), dtype=dt, device=u.device),
                              torch.empty(n, dtype=_F64, device=u.device),
                              torch.empty(cap, dtype=torch.int64, device=u.device), 0)
    else:
        if state.vectors.dtype != dt or tuple(state.vectors.shape[1:]) != (m, m) or state.vectors.device != u.device:
            raise ValueError("state does not belong to this tensor")
        if cap != have:
            r = state.rank
            vectors = torch.empty((cap, m, m), dtype=dt, device=u.device)
            pivots = torch.empty(cap, dtype=torch.int64, device=u.device)
            vectors[:r].copy_(state.vectors[:r])
            pivots[:r].copy_(state.pivots[:r])
            state = CholeskyState(vectors, state.diag, pivots, r)
    rank = ctypes.c_int64(state.rank)
    extremes = (ctypes.c_double * 2)()
    with _on_device_of(u, state.vectors, state.diag, state.pivots):
        work = workspace.get(nbytes, u.device)
        _ran(
            lib.qs_cholesky_two_body(
                code, u.data_ptr(), m, float(tol), state.vectors.data_ptr(), cap, ctypes.byref(rank),
                state.diag.data_ptr(), state.pivots.data_ptr(), extremes, work.data_ptr(), work.numel(), _stream(),
            ),
            "qs_cholesky_two_body",
        )
    state.rank = r = int(rank.value)
    return state.vectors[:r], state.pivots[:r], (float(extremes[0]), float(extremes[1])), state


# Byte budget of the blocks X of ONE pass of ``coupled_cluster.RCCD.triples``: all o^3 blocks where they fit it (one
# ``triples_energy`` launch over every triple), else passes over as many triples as their own blocks fit (at least one).
# The tuning key ``triples_bytes`` overrides it for the calling thread.
TRIPLES_BYTES = 8 << 30


def triples_budget():
    """The byte budget in force on the calling thread: the tuning key ``triples_bytes`` where it is set, else
    ``TRIPLES_BYTES``."""
    return check(_lib.load().qs_triples_energy_budget(TRIPLES_BYTES), "budget query")


def triples_tile(dtype):
    """Tile edge of ``triples_energy`` along each virtual index for ``dtype``: 8 for float64, 6 for complex128."""
    return check(_lib.load().qs_triples_energy_tile(dtype_code(dtype)), "tile query")


@_plain
def triples_energy(X, slots, eo3, ev, out=None):
    """``e[x] = sum_abc Re(conj(W) Z) / (eo3[x] - ev[a] - ev[b] - ev[c])`` of n occupied triples (``qs_triples_energy``),
    without the triple's weight:

        W[a,b,c] = X0[a,b,c] + X1[a,c,b] + X2[b,a,c] + X3[b,c,a] + X4[c,a,b] + X5[c,b,a]
        Z[a,b,c] = (4 W[abc] + W[bca] + W[cab] - 2 W[acb] - 2 W[cba] - 2 W[bac]) / 3

    with ``X0 ... X5`` the blocks ``X[slots[x]]`` of ``X`` (nblocks, v, v, v), float64 or complex128; ``slots`` (n, 6)
    int32 with every entry in ``0 ... nblocks - 1`` (equal entries allowed), ``eo3`` (n,) and ``ev`` (v,) float64.  One
    read of the blocks, neither W nor Z stored, no atomics: the same bits on every run and for a triple alone or in a
    batch.  Returns ``e`` (n,) float64."""
    lib = _lib.load()
    if not isinstance(X, torch.Tensor) or X.dtype not in (_F64, _C128):
        raise TypeError("X must be a float64 or complex128 tensor")
    if X.dim() != 4 or X.shape[0] < 1 or X.shape[1] < 1 or not X.shape[1] == X.shape[2] == X.shape[3]:
        raise ValueError(f"X must be (nblocks, v, v, v), got {tuple(X.shape)}")
    dt, (nblocks, v) = X.dtype, X.shape[:2]
    if not isinstance(slots, torch.Tensor) or slots.dtype != torch.int32 or slots.dim() != 2 or slots.shape[1] != 6 or slots.shape[0] < 1:
        raise ValueError("slots must be an (n, 6) int32 tensor of block indices")
    n = slots.shape[0]
    for name, arr, length in (("eo3", eo3, n), ("ev", ev, v)):
        if not isinstance(arr, torch.Tensor) or arr.dtype != _F64 or tuple(arr.shape) != (length,):
            raise ValueError(f"{name} must be a float64 tensor of shape ({length},)")
    X, slots, eo3, ev = _dev(X), _dev(slots), _dev(eo3), _dev(ev)
    lo, hi = slots.aminmax()
    if int(lo) < 0 or int(hi) >= nblocks:
        raise ValueError(f"slots must lie in 0 ... {nblocks - 1}, got {int(lo)} ... {int(hi)}")
    code = dtype_code(dt)
    nbytes = check(lib.qs_triples_energy_workspace(code, v, n), "workspace query")
    if out is None:
        out = torch.empty(n, dtype=_F64, device=X.device)
    else:
        _check_out(out, (n,), _F64, "triples_energy")
    with _on_device_of(X, slots, eo3, ev, out):
        work = workspace.get(nbytes, X.device)
        _ran(
            lib.qs_triples_energy(code, X.data_ptr(), nblocks, slots.data_ptr(), eo3.data_ptr(), ev.data_ptr(), v, n,
                                  out.data_ptr(), work.data_ptr(), work.numel(), _stream()),
            "qs_triples_energy",
        )
    return out


@_plain
def triples_energy_singles(X, slots, eo3, ev, A, G, sslots, out=None):
    """``(e, es)``: ``e`` as ``triples_energy`` and, beside it in the same read of the blocks, the singles part of (T)
    (``qs_triples_energy_singles``)

        es[x] = sum_abc Re(conj(V'[abc]) Z[abc]) / (eo3[x] - ev[a] - ev[b] - ev[c])

    with ``V'`` made like ``W`` from the outer products ``Y_beta[p,q,r] = A[sa][p] G[sg][q,r]``, ``(sa, sg) =
    sslots[x, beta]``, which are never stored.  ``A`` (na, v) and ``G`` (ng, v, v) in the dtype of ``X``; ``sslots``
    (n, 6, 2) int32 with ``sa`` in ``0 ... na - 1`` and ``sg`` in ``0 ... ng - 1``.  ``out``: a pair of (n,) float64
    tensors.  The same bits on every run and for a triple alone or in a batch."""
    lib = _lib.load()
    if not isinstance(X, torch.Tensor) or X.dtype not in (_F64, _C128):
        raise TypeError("X must be a float64 or complex128 tensor")
    if X.dim() != 4 or X.shape[0] < 1 or X.shape[1] < 1 or not X.shape[1] == X.shape[2] == X.shape[3]:
        raise ValueError(f"X must be (nblocks, v, v, v), got {tuple(X.shape)}")
    dt, (nblocks, v) = X.dtype, X.shape[:2]
    if not isinstance(slots, torch.Tensor) or slots.dtype != torch.int32 or slots.dim() != 2 or slots.shape[1] != 6 or slots.shape[0] < 1:
        raise ValueError("slots must be an (n, 6) int32 tensor of block indices")
    n = slots.shape[0]
    for name, arr, length in (("eo3", eo3, n), ("ev", ev, v)):
        if not isinstance(arr, torch.Tensor) or arr.dtype != _F64 or tuple(arr.shape) != (length,):
            raise ValueError(f"{name} must be a float64 tensor of shape ({length},)")
    if not isinstance(A, torch.Tensor) or A.dtype != dt or A.dim() != 2 or A.shape[0] < 1 or A.shape[1] != v:
        raise ValueError(f"A must be an (na, {v}) tensor of the dtype of X")
    if not isinstance(G, torch.Tensor) or G.dtype != dt or G.dim() != 3 or G.shape[0] < 1 or tuple(G.shape[1:]) != (v, v):
        raise ValueError(f"G must be an (ng, {v}, {v}) tensor of the dtype of X")
    if not isinstance(sslots, torch.Tensor) or sslots.dtype != torch.int32 or tuple(sslots.shape) != (n, 6, 2):
        raise ValueError(f"sslots must be an ({n}, 6, 2) int32 tensor of (A row, G block) indices")
    na, ng = A.shape[0], G.shape[0]
    X, slots, eo3, ev, A, G, sslots = _dev(X), _dev(slots), _dev(eo3), _dev(ev), _dev(A), _dev(G), _dev(sslots)
    # the three ranges in one trip to the host
    tables = (("slots", slots, nblocks), ("sslots[..., 0]", sslots[..., 0], na), ("sslots[..., 1]", sslots[..., 1], ng))
    ends = torch.stack([torch.stack(table.aminmax()) for _, table, _ in tables]).tolist()
    for (name, _, top), (lo, hi) in zip(tables, ends):
        if lo < 0 or hi >= top:
            raise ValueError(f"{name} must lie in 0 ... {top - 1}, got {lo} ... {hi}")
    code = dtype_code(dt)
    nbytes = check(lib.qs_triples_energy_singles_workspace(code, v, n), "workspace query")
    if out is None:
        e, es = torch.empty(n, dtype=_F64, device=X.device), torch.empty(n, dtype=_F64, device=X.device)
    else:
        if not isinstance(out, (tuple, list)) or len(out) != 2:
            raise ValueError("out must be a pair (e, es) of tensors")
        e, es = out
        _check_out(e, (n,), _F64, "triples_energy_singles")
        _check_out(es, (n,), _F64, "triples_energy_singles")
    with _on_device_of(X, slots, eo3, ev, A, G, sslots, e, es):
        work = workspace.get(nbytes, X.device)
        _ran(
            lib.qs_triples_energy_singles(code, X.data_ptr(), nblocks, slots.data_ptr(), eo3.data_ptr(), ev.data_ptr(),
                                          A.data_ptr(), na, G.data_ptr(), ng, sslots.data_ptr(), v, n, e.data_ptr(),
                                          es.data_ptr(), work.data_ptr(), work.numel(), _stream()),
            "qs_triples_energy_singles",
        )
    return e, es


class RcclComm:
    """The C ABI's communicator (``qs_comm_init``: RCCL over xGMI, one process per GPU) for hosts that drive the
    library from Python without ``torch.distributed``.  ``unique_id()`` on one rank, the 128 bytes to the others by
    any means, then ``RcclComm(rank, world, id_bytes)`` on every rank (collective)."""

    @staticmethod
    def unique_id():
        import ctypes

        buf = (ctypes.c_char * 128)()
        check(_lib.load().qs_comm_unique_id(ctypes.cast(buf, ctypes.c_void_p)), "qs_comm_unique_id")
        return bytes(buf)

    def __init__(self, rank, world, unique_id, rows_coalesce=False):
        import ctypes

        if len(unique_id) != 128:
            raise ValueError("the unique id is 128 bytes")
        self._handle = ctypes.c_void_p()
        buf = ctypes.create_string_buffer(bytes(unique_id), 128)
        check(_lib.load().qs_comm_init(ctypes.byref(self._handle), int(rank), int(world),
                                       ctypes.cast(buf, ctypes.c_void_p)), "qs_comm_init")
        self.rank, self.world = int(rank), int(world)
        if rows_coalesce:
            self.set_option("rows_coalesce", 1)

    def set_option(self, key, value):
        """Per-handle option (``qs_comm_set_option``; every rank must choose the same).  ``rows_coalesce`` = 1: the rows
        exchange as ONE message per peer and step through a staging area instead of one per peer and result row."""
        check(_lib.load().qs_comm_set_option(self._handle, key.encode(), int(value)), "qs_comm_set_option")

    def close(self):
        if self._handle:
            check(_lib.load().qs_comm_destroy(self._handle), "qs_comm_destroy")
            self._handle = None

    def abort(self):
        """Tear down without waiting for outstanding operations: after a call failed in the middle of its exchange."""
        if self._handle:
            handle, self._handle = self._handle, None
            check(_lib.load().qs_comm_abort(handle), "qs_comm_abort")

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
        return False

    @_plain
    def transform_two_body_rows(self, rows, C, C_tilde=None, in_part=None, chunk_rows=0, out=None):
        """Rows of one leading index of ``u`` in, rows of the other transformed leading index out, everything else
        O(chunk_rows l^3): ``qs_transform_two_body_sharded_rows`` (see include/qs_amd.h and
        ``sharded.transform_two_body_rows``, the same algorithm on torch.distributed).  ``rows`` (il, L, L, L) follows
        ``in_part`` (a ``sharded.SlabPartition``; balanced by default); a real ``rows`` against complex coefficients
        is not copied to complex.  Returns the (jl, M, M, M) view of the result buffer (``out`` may supply the flat
        buffer to reuse it across the steps of a time loop)."""
        import ctypes

        lib = _lib.load()
        if C_tilde is None:
            C_tilde = default_bra(C)
        dt = result_dtype(rows, C, C_tilde)
        in_dt = _F64 if (dt == _C128 and rows.dtype == _F64 and mixed_real_u) else dt
        rows, C, Ct = _dev(rows, in_dt), _dev(C, dt), _dev(C_tilde, dt)
        L, M = C.shape
        code = dtype_code(dt)
        starts = None
        if in_part is not None:
            if (in_part.n, in_part.world) != (L, self.world):
                raise ValueError("the input partition does not describe L rows over this communicator's ranks")
            starts = (ctypes.c_int64 * (self.world + 1))(*in_part.starts)
        il = (in_part or SlabPartition(L, self.world)).count(self.rank)
        jl = SlabPartition(M, self.world).count(self.rank)
        if tuple(rows.shape) != (il, L, L, L) or tuple(Ct.shape) != (M, L):
            raise ValueError(f"rank {self.rank}: expected rows of shape {(il, L, L, L)} and C_tilde {(M, L)}")
        p_starts = ctypes.cast(starts, ctypes.c_void_p) if starts is not None else None
        ni = int(chunk_rows)
        if ni < 1:
            ni = check(lib.qs_sharded_rows_default_chunk(code, L, M, self.world, p_starts), "chunk query")
        es = 16 if dt == _C128 else 8
        out_bytes = check(lib.qs_transform_two_body_sharded_rows_out_bytes(code, L, M, self.world, self.rank), "size query")
        if out is None:
            out = torch.empty(out_bytes // es, dtype=dt, device=rows.device)
        elif (not isinstance(out, torch.Tensor) or out.dtype != dt or out.numel() * es < out_bytes
              or not out.is_contiguous() or out.device != rows.device):
            raise ValueError(f"`out` must be a contiguous {dt} buffer of at least {out_bytes // es} elements")
        nbytes = check(lib.qs_comm_rows_workspace(self._handle, code, L, M, ni), "workspace query")
        with _on_device_of(rows, C, Ct, out):
            work = workspace.get(nbytes, rows.device)
            _ran(
                lib.qs_transform_two_body_sharded_rows(
                    self._handle, dtype_code(in_dt), code, rows.data_ptr(), p_starts, C.data_ptr(), Ct.data_ptr(),
                    out.data_ptr(), out.numel() * es, work.data_ptr(), work.numel(), L, M, ni, _stream(),
                ),
                "qs_transform_two_body_sharded_rows",
            )
        return out.reshape(-1)[: jl * M * M * M].view(jl, M, M, M)

    def transform_two_body(self, u_bslab, C, C_tilde=None, out=None, nchunks=4):
        """``out[p_lo:p_hi]`` of the transform from ``u[:, b_lo:b_hi]`` (balanced splits): the whole sharded
        transform in ONE C-ABI call -- local contractions, chunked grouped send / receive on the communicator's
        stream overlapped with them, closing contraction (``qs_transform_two_body_sharded``)."""
        lib = _lib.load()
        if C_tilde is None:
            C_tilde = default_bra(C)
        dt = result_dtype(u_bslab, C, C_tilde)
        u_bslab, C, Ct = _dev(u_bslab, dt), _dev(C, dt), _dev(C_tilde, dt)
        L, M = C.shape
        code = dtype_code(dt)
        pc, bl = SlabPartition(M, self.world).count(self.rank), SlabPartition(L, self.world).count(self.rank)
        if tuple(u_bslab.shape) != (L, bl, L, L) or tuple(Ct.shape) != (M, L):
            raise ValueError(f"rank {self.rank}: expected a slab of shape {(L, bl, L, L)} and C_tilde {(M, L)}")
        if out is None:
            out = torch.empty((pc, M, M, M), dtype=dt, device=u_bslab.device)
        else:
            _check_out(out, (pc, M, M, M), dt, "RcclComm.transform_two_body")
        nbytes = check(lib.qs_transform_two_body_sharded_workspace(code, L, M, self.world, self.rank), "workspace query")
        with _on_device_of(u_bslab, C, Ct, out):
            work = workspace.get(nbytes, u_bslab.device)
            _ran(
                lib.qs_transform_two_body_sharded(
                    self._handle, code, u_bslab.data_ptr(), C.data_ptr(), Ct.data_ptr(), out.data_ptr(),
                    work.data_ptr(), work.numel(), L, M, int(nchunks), _stream(),
                ),
                "qs_transform_two_body_sharded",
            )
        return out


def tuning_set(key, value):
    """Tuning / test hook: kernel-choice override for the CALLING THREAD only
    (the library keeps no process-global mutable state)."""
    check(_lib.load().qs_tuning_set(key.encode(), int(value)), "qs_tuning_set")


def tuning_reset():
    """Back to the automatic kernel choice on the calling thread."""
    check(_lib.load().qs_tuning_reset(), "qs_tuning_reset")


class tuning:
    """``with tuning(gemm_fast=0): ...`` -- overrides for the block, automatic policy after it."""

    def __init__(self, **knobs):
        self.knobs = knobs

    def __enter__(self):
        for key, value in self.knobs.items():
            tuning_set(key, value)
        return self

    def __exit__(self, *exc):
        tuning_reset()
        return False


def last_dispatch():
    """Names (as rocprofv3 prints them) of the kernels the calling thread's most
    recent library call launched, e.g. ``qs::gemm_fast_kernel<false, 4, 4, true, false> x4``."""
    return _lib.load().qs_last_dispatch().decode()
