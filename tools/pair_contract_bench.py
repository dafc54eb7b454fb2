"""Time ``kernels.pair_contract`` against the tall product it replaces, for every candidate group size G.

    python tools/pair_contract_bench.py [--out FILE] [--reps N] [--cases fp64:128,...] [--k 1,2,4,8,16] [--groups 0,1,2,4,8]

  new   ONE call of kernels.pair_contract(u, T)                            ceil(K / G) reads of u
  old   kernels.matmul(u.view(l^2, l^2), T^T) -- for the mixed form the same on [Re T; Im T] (2 K real columns),
        the only route that needs no complex copy of u

One process; after two warm-ups the two routes alternate ``reps`` times, HIP events around each, median [min, max].
G = 0 is the shipped group size of the form, the others are set through the tuning knob ``pair_contract_g``.
"holds" says whether the SLOWEST new run beat the FASTEST old run.  "of copy" is bytes of u over the new route's median
time against the rate of ``qs_probe_stream_copy`` (read + write counted) measured in the same run.  Needs a GPU."""

import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from quantum_systems_amd import _lib, kernels  # noqa: E402

DEFAULT = "fp64:128,complex128:128,mixed:128,fp64:256"


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
    return f"{statistics.median(xs):9.4f} ms [{min(xs):9.4f}, {max(xs):9.4f}]"


def copy_rate(reps):
    """GB/s of the 16-byte-per-lane device copy on 2 GiB (read + write counted)."""
    lib = _lib.load()
    n = 1 << 31
    src, dst = torch.empty(n, dtype=torch.uint8, device="cuda"), torch.empty(n, dtype=torch.uint8, device="cuda")
    src.zero_()
    stream = torch.cuda.current_stream().cuda_stream
    ts = []
    for i in range(reps + 2):
        t = timed(lambda: _lib.check(lib.qs_probe_stream_copy(src.data_ptr(), dst.data_ptr(), n, stream), "copy"))[0]
        if i >= 2:
            ts.append(t)
    return 2 * n / (statistics.median(ts) * 1e-3) / 1e9


def run_case(form, l, ks, groups, reps, roof, emit):
    cplx = torch.complex128
    u = fill((l, l, l, l), cplx if form == "complex128" else torch.float64, 1)
    T = fill((max(ks), l, l), torch.float64 if form == "fp64" else cplx, 2)
    U2 = u.view(l * l, l * l)
    nbytes = u.numel() * u.element_size()
    emit(f"{form} l={l}: u = {nbytes / 1e9:.3f} GB")
    for k in ks:
        Tk = T[:k]
        if form == "mixed":
            B = torch.cat([Tk.real, Tk.imag]).reshape(2 * k, l * l).transpose(0, 1).contiguous()
        else:
            B = Tk.reshape(k, l * l).transpose(0, 1).contiguous()

        def old():
            return kernels.matmul(U2, B)

        def new():
            return kernels.pair_contract(u, Tk)

        for G in groups:
            with kernels.tuning(pair_contract_g=G):
                for _ in range(2):
                    s_old, s_new = old(), new()
                torch.cuda.synchronize()
                ref = s_old.transpose(0, 1).reshape(-1, l, l)
                ref = torch.complex(ref[:k], ref[k:]) if form == "mixed" else ref
                rel = float((s_new - ref).abs().max() / ref.abs().max())
                t_old, t_new = [], []
                for _ in range(reps):
                    t_new.append(timed(new)[0])
                    t_old.append(timed(old)[0])
                launched = kernels.last_dispatch()
            m_old, m_new = statistics.median(t_old), statistics.median(t_new)
            passes = launched.count("pair_contract_kernel")
            emit(f"  K={k:2d} G={G}: old {stats(t_old)}  new {stats(t_new)}  gain {m_old / m_new:5.2f}x  "
                 f"holds {max(t_new) < min(t_old)}  u at {nbytes / (m_new * 1e-3) / 1e9:7.1f} GB/s per call "
                 f"({nbytes / (m_new * 1e-3) / 1e9 / (roof / 2):.2f} of copy for one read)  rel diff {rel:.1e}  [{launched}; {passes} name(s)]")
    del u, U2
    torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--cases", default=DEFAULT)
    ap.add_argument("--k", default="1,2,4,8,16")
    ap.add_argument("--groups", default="0,1,2,4,8")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("pair_contract_bench needs a GPU: timings are not taken on a CPU")
    fh = open(args.out, "a") if args.out else None

    def emit(line):
        print(line, flush=True)
        if fh:
            fh.write(line + "\n")
            fh.flush()

    emit(f"# pair_contract_bench: {torch.cuda.get_device_name(0)}, reps {args.reps}, new / old alternating, HIP events, "
         "median [min, max]")
    roof = copy_rate(args.reps)
    emit(f"# qs_probe_stream_copy on 2 GiB: {roof:.1f} GB/s read + write, {roof / 2:.1f} GB/s of reads")
    ks, groups = [int(x) for x in args.k.split(",")], [int(x) for x in args.groups.split(",")]
    for case in args.cases.split(","):
        form, l = case.split(":")
        run_case(form, int(l), ks, groups, args.reps, roof, emit)


if __name__ == "__main__":
    main()
