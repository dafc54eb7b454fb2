"""Time the Cholesky vectors of a two-body tensor of the quantum dot's shape: the decomposition against the streaming
roof, the change of basis of the vectors against the four-index transform of ``u``, and ``reconstruct``.

    python tools/cholesky_bench.py [--out FILE] [--reps N] [--cases 55,105,153] [--rel-tol 1e-9] [--input synthetic|dot]

The input is a seeded fp64 tensor of EXACT rank 4 l, ``u = sum_x B_x^T (x) B_x`` -- the rank of the dot's Coulomb tensor,
whose cost the decomposition shares: it depends on (l, rank) alone.  ``--input dot`` takes the Coulomb tensor of the
GPU generator instead; its closed form is ill-conditioned from about 9 shells on, so beyond l = 45
the generated tensor is low-rank and positive semidefinite only to the generator's own error and wants a ``--rel-tol``
above it.

Per case (l orbitals), in ONE process on one device, HIP events around each call after a warm-up, medians with ranges:
  decompose   cholesky.decompose(u, rel_tol * max|u|), the whole call: its two launches per step and the read-backs of
              the stop flag.  Bytes of the model: the update sum reads j m^2 elements at step j, the step reads the
              pivot column and the diagonal and writes the vector and the diagonal:
                  e m^2 r (r - 1) / 2  +  r m^2 (2 e + 16),     e = bytes per element, r = rank.
              ``fraction of roof`` = (model bytes / time) / (2 x bytes / copy time) of qs_probe_stream_copy on 1 GiB,
              the probe ``bench.py --full`` reports as the streaming ceiling.
  transform   chol.transform(C) for a seeded unitary complex C, against kernels.transform_two_body(u, C) at the same l
              (skipped above --full-transform-max orbitals, where the l^4 complex result no longer fits beside u).
  reconstruct chol.reconstruct() into a preallocated tensor.
and the largest element of |u - reconstruct()| over max|u| is printed beside the residual extremes."""

import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from quantum_systems_amd import _lib, cholesky, kernels  # noqa: E402
from quantum_systems_amd.two_dim_ho import get_coulomb_elements  # noqa: E402


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b), out


def stats(xs):
    return f"{statistics.median(xs):10.3f} ms  [{min(xs):.3f}, {max(xs):.3f}]"


def copy_rate(reps):
    """Bytes per millisecond (read + write) of the streaming copy probe on 1 GiB."""
    nbytes = 1 << 30
    src = torch.empty(nbytes, dtype=torch.uint8, device="cuda").zero_()
    dst = torch.empty_like(src)
    lib = _lib.load()
    ts = []
    for i in range(2 + reps):
        t = timed(lambda: _lib.check(lib.qs_probe_stream_copy(src.data_ptr(), dst.data_ptr(), nbytes, kernels._stream()),
                                     "stream copy"))[0]
        if i >= 2:
            ts.append(t)
    return 2 * nbytes / statistics.median(ts), ts


def unitary(l, seed):
    gen = torch.Generator(device="cuda").manual_seed(seed)
    a = torch.randn((l, l), dtype=torch.complex128, device="cuda", generator=gen)
    return torch.linalg.qr(a)[0].contiguous()


def make_input(l, kind):
    if kind == "dot":
        return get_coulomb_elements(l)
    gen = torch.Generator(device="cuda").manual_seed(l)
    B = torch.randn((4 * l, l, l), dtype=torch.float64, device="cuda", generator=gen)
    return cholesky.CholeskyTwoBody(B).reconstruct()


def run_case(l, reps, rel_tol, roof, full_max, kind, emit):
    u = make_input(l, kind)
    scale = float(u.abs().max())
    tol = rel_tol * scale
    m2, e = l * l, u.element_size()

    chol = cholesky.decompose(u, tol)                       # warm-up (code objects, the workspace)
    t_dec = []
    for _ in range(reps):
        t, chol = timed(lambda: cholesky.decompose(u, tol))
        t_dec.append(t)
    # the kernels of the decomposition itself (decompose resumes after a doubling: the last call's launches)
    kernels.cholesky_two_body(u, tol, max_rank=max(chol.rank, 1))
    ran = kernels.last_dispatch()
    r = chol.rank
    model = e * m2 * r * (r - 1) // 2 + r * m2 * (2 * e + 16)
    m_dec = statistics.median(t_dec)
    emit(f"l={l} ({kind}): u = {u.numel() * e / 1e9:.3f} GB fp64, rank {r} of {m2} ({r / l:.2f} l), converged {chol.converged}, "
         f"vectors {r * m2 * e / 1e9:.4f} GB, residual max {chol.residual[0]:.2e} min {chol.residual[1]:.2e} (tol {tol:.2e})")
    emit(f"  decompose   {stats(t_dec)}   model {model / 1e9:.3f} GB -> {model / m_dec / 1e9:7.3f} TB/s, "
         f"fraction of roof {model / m_dec / roof:.3f}   kernels: {ran}")

    out = torch.empty_like(u)
    chol.reconstruct(out=out)
    err = float((out - u).abs().max()) / scale
    t_rec = [timed(lambda: chol.reconstruct(out=out))[0] for _ in range(reps)]
    emit(f"  reconstruct {stats(t_rec)}   max |u - reconstruct()| / max|u| = {err:.2e}")
    del out

    C = unitary(l, 3)
    chol.transform(C)
    t_vec = [timed(lambda: chol.transform(C))[0] for _ in range(reps)]
    emit(f"  transform   {stats(t_vec)}   (vectors: {r} one-body transforms)")
    if l <= full_max:
        kernels.transform_two_body(u, C)
        t_full = [timed(lambda: kernels.transform_two_body(u, C))[0] for _ in range(reps)]
        emit(f"  full        {stats(t_full)}   kernels.transform_two_body(u, C): {statistics.median(t_full) / statistics.median(t_vec):.1f}x the vectors")
    else:
        emit("  full        not measured (above --full-transform-max)")
    del u
    torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--cases", default="55,105,153")
    ap.add_argument("--rel-tol", type=float, default=1e-9)
    ap.add_argument("--full-transform-max", type=int, default=160)
    ap.add_argument("--input", choices=("synthetic", "dot"), default="synthetic")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("cholesky_bench needs a GPU: timings are not taken on a CPU")
    fh = open(args.out, "a") if args.out else None

    def emit(line):
        print(line, flush=True)
        if fh:
            fh.write(line + "\n")
            fh.flush()

    roof, ts = copy_rate(args.reps)
    emit(f"# cholesky_bench: {torch.cuda.get_device_name(0)}, reps {args.reps}, HIP events, median [min, max]; "
         f"streaming copy of 1 GiB {stats(ts)} = {roof / 1e9:.3f} TB/s read + write")
    for l in args.cases.split(","):
        run_case(int(l), args.reps, args.rel_tol, roof, args.full_transform_max, args.input, emit)


if __name__ == "__main__":
    main()
