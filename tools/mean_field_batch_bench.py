"""Time ``kernels.mean_field_batch`` against ND sequential ``kernels.mean_field`` calls (the only route to several
mean fields before the batch entry) for every candidate group size G.

    python tools/mean_field_batch_bench.py [--out FILE] [--reps N] [--cases fp64:128,...] [--nd 1,2,4,8,16] [--groups 0,2,4,8]

  loop   ND calls of kernels.mean_field(u, D[k], cj=1, ck=-0.5)          ND reads of u
  batch  ONE call of kernels.mean_field_batch(u, D, cj=1, ck=-0.5)       ceil(ND / G) reads of u

One process; after two warm-ups the two routes alternate ``reps`` times, HIP events around each, median [min, max].
G = 0 is the shipped group size of the form, the others are set through the tuning knob ``mean_field_batch_g``.
"holds" says whether the SLOWEST batch run beat the FASTEST loop run.  Needs a GPU."""

import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from quantum_systems_amd import kernels  # noqa: E402

DEFAULT = "fp64:128,mixed:128,complex128:128,fp64:256,mixed:256"


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


def run_case(form, l, nds, groups, reps, emit):
    cplx = torch.complex128
    u = fill((l, l, l, l), cplx if form == "complex128" else torch.float64, 1)
    D = fill((max(nds), l, l), torch.float64 if form == "fp64" else cplx, 2)
    nbytes = u.numel() * u.element_size()
    emit(f"{form} l={l}: u = {nbytes / 1e9:.3f} GB")
    for nd in nds:
        Dn = D[:nd]

        def loop():
            return [kernels.mean_field(u, Dn[k], cj=1.0, ck=-0.5) for k in range(nd)]

        def batch():
            return kernels.mean_field_batch(u, Dn, cj=1.0, ck=-0.5)

        for G in groups:
            with kernels.tuning(mean_field_batch_g=G):
                for _ in range(2):
                    w_loop, w_batch = loop(), batch()
                torch.cuda.synchronize()
                rel = max(float((w_batch[k] - w_loop[k]).abs().max() / w_loop[k].abs().max()) for k in range(nd))
                t_loop, t_batch = [], []
                for _ in range(reps):
                    t_loop.append(timed(loop)[0])
                    t_batch.append(timed(batch)[0])
                launched = kernels.last_dispatch()
            m_loop, m_batch = statistics.median(t_loop), statistics.median(t_batch)
            emit(f"  ND={nd:2d} G={G}: loop {stats(t_loop)}  batch {stats(t_batch)}  gain {m_loop / m_batch:5.2f}x  "
                 f"per density {m_batch / nd:8.4f} ms  holds {max(t_batch) < min(t_loop)}  rel diff {rel:.1e}  [{launched}]")
    del u
    torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--cases", default=DEFAULT)
    ap.add_argument("--nd", default="1,2,4,8,16")
    ap.add_argument("--groups", default="0,2,4,8")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("mean_field_batch_bench needs a GPU: timings are not taken on a CPU")
    fh = open(args.out, "a") if args.out else None

    def emit(line):
        print(line, flush=True)
        if fh:
            fh.write(line + "\n")
            fh.flush()

    emit(f"# mean_field_batch_bench: {torch.cuda.get_device_name(0)}, reps {args.reps}, loop / batch alternating, HIP events, "
         "median [min, max]")
    nds, groups = [int(x) for x in args.nd.split(",")], [int(x) for x in args.groups.split(",")]
    for case in args.cases.split(","):
        form, l = case.split(":")
        run_case(form, int(l), nds, groups, args.reps, emit)


if __name__ == "__main__":
    main()
