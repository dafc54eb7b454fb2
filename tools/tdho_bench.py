"""Time the two generators of the 2-D harmonic-oscillator Coulomb elements: the closed form
(``qs_tdho_coulomb_elements``) and the quadrature (``qs_tdho_coulomb_quadrature``).

    python tools/tdho_bench.py [--out FILE] [--reps N] [--both 28,55] [--quadrature 105,153,253]

One process.  Output and workspace are allocated once per size and both entry points are called through the C ABI, so a
time holds the launches of one call and nothing else.  After two warm-ups the generators alternate ``reps`` times (the
closed form at most 3 times from l = 55 on: it takes seconds there), HIP events around each call, median [min, max].
"beats" is the rule for the README's recommendation: the slowest quadrature run is faster than the fastest closed-form
run.  The quadrature is store-bound (l^4 doubles, every one written once), so its rate is the bytes of the output over
the median time, beside two probes taken in the same run on a buffer of 8 GiB: ``fill`` (torch ``zero_``, stores only)
and ``copy`` (``qs_probe_stream_copy``, its reads and writes counted).  "diff" is the largest difference between the two
tensors.  Needs a GPU."""

import argparse
import ctypes
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from quantum_systems_amd import _lib  # noqa: E402

PROBE_BYTES = 1 << 33


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def stats(xs):
    return f"{statistics.median(xs):10.4f} ms [{min(xs):10.4f}, {max(xs):10.4f}]"


def probes(reps):
    """GB/s of stores of a fill, and GB/s (read + write) of the stream copy."""
    lib = _lib.load()
    n = PROBE_BYTES
    dst = torch.empty(n, dtype=torch.uint8, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream
    fills = [timed(lambda: dst.zero_()) for _ in range(reps + 2)][2:]
    src = torch.zeros(n, dtype=torch.uint8, device="cuda")
    copies = [timed(lambda: _lib.check(lib.qs_probe_stream_copy(src.data_ptr(), dst.data_ptr(), n, stream), "copy"))
              for _ in range(reps + 2)][2:]
    return n / (statistics.median(fills) * 1e-3) / 1e9, 2 * n / (statistics.median(copies) * 1e-3) / 1e9


def run(l, reps, with_closed, fill_rate, copy_rate, emit):
    lib = _lib.load()
    stream = torch.cuda.current_stream().cuda_stream
    out = torch.empty((l,) * 4, dtype=torch.float64, device="cuda")
    need = ctypes.c_int64(0)
    _lib.check(lib.qs_tdho_coulomb_quadrature_workspace(l, 0, ctypes.byref(need)), "workspace")
    work = torch.empty(need.value, dtype=torch.uint8, device="cuda")
    nbytes = out.numel() * 8

    def quadrature():
        _lib.check(lib.qs_tdho_coulomb_quadrature(out.data_ptr(), None, l, 0, 0, l, work.data_ptr(), need.value, stream),
                   "qs_tdho_coulomb_quadrature")

    def closed():
        _lib.check(lib.qs_tdho_coulomb_elements(ref.data_ptr(), l, 0, l, stream), "qs_tdho_coulomb_elements")

    t_quad, t_closed = [], []
    if with_closed:
        ref = torch.empty_like(out)
        closed_reps = reps if l < 55 else min(reps, 3)
        closed()
        for _ in range(2):
            quadrature()
        for i in range(reps):
            t_quad.append(timed(quadrature))
            if i < closed_reps:
                t_closed.append(timed(closed))
        diff = float((out - ref).abs().max())
    else:
        for _ in range(2):
            quadrature()
        t_quad = [timed(quadrature) for _ in range(reps)]
    rate = nbytes / (statistics.median(t_quad) * 1e-3) / 1e9
    line = (f"l={l:3d}: u = {nbytes / 1e9:8.4f} GB  quadrature {stats(t_quad)}  {rate:7.1f} GB/s of stores "
            f"({rate / fill_rate:.2f} of fill, {rate / copy_rate:.2f} of copy)")
    if with_closed:
        line += (f"  closed form {stats(t_closed)}  gain {statistics.median(t_closed) / statistics.median(t_quad):8.1f}x  "
                 f"beats {max(t_quad) < min(t_closed)}  diff {diff:.1e}")
    emit(line)
    del out, work
    torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--both", default="28,55")
    ap.add_argument("--quadrature", default="105,153,253")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tdho_bench needs a GPU: timings are not taken on a CPU")
    fh = open(args.out, "a") if args.out else None

    def emit(line):
        print(line, flush=True)
        if fh:
            fh.write(line + "\n")
            fh.flush()

    emit(f"# tdho_bench: {torch.cuda.get_device_name(0)}, reps {args.reps}, HIP events around one call, median [min, max]")
    fill_rate, copy_rate = probes(args.reps)
    emit(f"# probes on {PROBE_BYTES >> 30} GiB: fill {fill_rate:.1f} GB/s of stores, qs_probe_stream_copy {copy_rate:.1f} GB/s read + write")
    for l in filter(None, args.both.split(",")):
        run(int(l), args.reps, True, fill_rate, copy_rate, emit)
    for l in filter(None, args.quadrature.split(",")):
        run(int(l), args.reps, False, fill_rate, copy_rate, emit)


if __name__ == "__main__":
    main()
