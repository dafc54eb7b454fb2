"""Time ``kernels.mean_field`` against the array-module route to the same numbers and against the streaming roof.

    python tools/mean_field_bench.py [--out FILE] [--reps N] [--cases fp64:64,fp64:128,...]

Per case (dtype form : l), in ONE process on one device, the two routes alternating ``reps`` times after warm-ups (the
copy before them), HIP events around each call, medians with ranges:
  new    kernels.mean_field(u, D, cj=1, ck=-0.5)                      one read of u
  old    hip.einsum("prqs,sr->pq", u, D) - 0.5 * hip.einsum("prsq,sr->pq", u, D)   (mixed: after u.to(complex128))
  copy   qs_probe_stream_copy of as many bytes as u holds (moves twice that): the roof of a streaming kernel
and the results of the two routes are compared (max relative difference).  ``fraction of roof`` = (bytes of u / new)
/ (2 x bytes of u / copy)."""

import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from quantum_systems_amd import _lib, hip, kernels  # noqa: E402

DEFAULT = "fp64:64,fp64:128,fp64:256,complex128:128,mixed:128,mixed:256"


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b), out


def fill(shape, dtype, seed):
    gen = torch.Generator(device="cuda").manual_seed(seed)
    t = torch.empty(shape, dtype=dtype, device="cuda")
    flat = torch.view_as_real(t).reshape(-1) if t.is_complex() else t.reshape(-1)
    step = 1 << 28
    for i in range(0, flat.numel(), step):
        flat[i:i + step].normal_(generator=gen)
    return t


def stats(xs):
    return f"{statistics.median(xs):10.4f} ms  [{min(xs):.4f}, {max(xs):.4f}]"


def run_case(form, l, reps, emit):
    cplx = torch.complex128
    u = fill((l, l, l, l), cplx if form == "complex128" else torch.float64, 1)
    D = fill((l, l), torch.float64 if form == "fp64" else cplx, 2)
    nbytes = u.numel() * u.element_size()
    lib = _lib.load()

    def new():
        return kernels.mean_field(u, D, cj=1.0, ck=-0.5)

    def old():
        uu = u.to(cplx) if form == "mixed" else u
        return hip.einsum("prqs,sr->pq", uu, D) - 0.5 * hip.einsum("prsq,sr->pq", uu, D)

    dst = torch.empty(nbytes, dtype=torch.uint8, device="cuda")

    def copy():
        _lib.check(lib.qs_probe_stream_copy(u.data_ptr(), dst.data_ptr(), nbytes, kernels._stream()), "stream copy")

    # the roof first (its destination is freed before the old route needs its temporaries), then new / old alternating
    t_new, t_old, t_copy = [], [], []
    for i in range(2 + reps):
        t = timed(copy)[0]
        if i >= 2:
            t_copy.append(t)
    del dst
    torch.cuda.empty_cache()
    for _ in range(2):
        w_new, w_old = new(), old()
    torch.cuda.synchronize()
    rel = float((w_new - w_old).abs().max() / w_old.abs().max())
    for _ in range(reps):
        t_new.append(timed(new)[0])
        t_old.append(timed(old)[0])
    m_new, m_old, m_copy = (statistics.median(x) for x in (t_new, t_old, t_copy))
    emit(f"{form} l={l}: u = {nbytes / 1e9:.3f} GB, max rel difference new/old {rel:.2e}, kernels: {kernels.last_dispatch()}")
    emit(f"  new  {stats(t_new)}   {nbytes / m_new / 1e9:8.3f} TB/s of u")
    emit(f"  old  {stats(t_old)}   speed-up {m_old / m_new:6.2f}x   (slowest new {max(t_new):.4f} vs fastest old {min(t_old):.4f})")
    emit(f"  copy {stats(t_copy)}   {2 * nbytes / m_copy / 1e9:8.3f} TB/s read + write")
    emit(f"  fraction of roof {(nbytes / m_new) / (2 * nbytes / m_copy):.3f}")
    del u
    torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--cases", default=DEFAULT)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("mean_field_bench needs a GPU: timings are not taken on a CPU")
    fh = open(args.out, "a") if args.out else None

    def emit(line):
        print(line, flush=True)
        if fh:
            fh.write(line + "\n")
            fh.flush()

    emit(f"# mean_field_bench: {torch.cuda.get_device_name(0)}, reps {args.reps}, new / old alternating (copy before them), HIP events, median [min, max]")
    for case in args.cases.split(","):
        form, l = case.split(":")
        run_case(form, int(l), args.reps, emit)


if __name__ == "__main__":
    main()
