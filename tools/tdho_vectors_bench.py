"""Time the Coulomb vectors of the 2-D harmonic oscillator (``qs_tdho_coulomb_vectors``) and what runs on
them: generation, one RHF iteration's mean field, the change of basis and MP2.

    python tools/tdho_vectors_bench.py [--out FILE] [--reps N] [--generate 55,153,253,528] [--consume 253,528] [--tensor 253]

One process.  Generation: output and workspace are allocated once per size and the entry point is called through the C
ABI, so a time holds the three launches of one call and nothing else; after two warm-ups ``reps`` runs, HIP events around
each, median [min, max].  The store kernel is the only part with volume (rank l^2 doubles, every one written once), so
its rate is the bytes of the output over the median time, beside the ``fill`` probe (torch ``zero_`` on 8 GiB, stores
only) taken in the same run.  Consumers, at the sizes of ``--consume``: the mean field of one closed-shell density on
the vectors (``CholeskyTwoBody.mean_field``, cj = 1, ck = -1/2: one RHF iteration's O(rank l^3) step), ``transform`` with
a unitary ``C``, and the MP2 block ``transform_blocks`` for 6 occupied orbitals with its energy sum; at the sizes of
``--tensor`` the mean field on ``u`` itself (``kernels.mean_field``) in the same process.  Building a basis set at 32
shells is timed once (``basis``): its host loops (single-particle functions, position integrals) are not part of this
work.  Nothing here is a gate.  Needs a GPU."""

import argparse
import ctypes
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from quantum_systems_amd import _lib, kernels  # noqa: E402
from quantum_systems_amd import two_dim_ho as td  # noqa: E402
from quantum_systems_amd.cholesky import CholeskyTwoBody  # noqa: E402

PROBE_BYTES = 1 << 33
OCCUPIED = 6


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def stats(xs):
    return f"{statistics.median(xs):10.4f} ms [{min(xs):10.4f}, {max(xs):10.4f}]"


def runs(fn, reps, warm=2):
    for _ in range(warm):
        fn()
    return [timed(fn) for _ in range(reps)]


def fill_probe(reps):
    dst = torch.empty(PROBE_BYTES, dtype=torch.uint8, device="cuda")
    t = runs(lambda: dst.zero_(), reps)
    return PROBE_BYTES / (statistics.median(t) * 1e-3) / 1e9


def generate(l, reps, fill_rate, emit):
    lib = _lib.load()
    stream = torch.cuda.current_stream().cuda_stream
    rank = td.coulomb_vectors_rank(l)
    out = torch.empty((rank, l, l), dtype=torch.float64, device="cuda")
    need = ctypes.c_int64(0)
    _lib.check(lib.qs_tdho_coulomb_vectors_workspace(l, 0, ctypes.byref(need)), "workspace")
    work = torch.empty(need.value, dtype=torch.uint8, device="cuda")
    nbytes = out.numel() * 8

    def call():
        _lib.check(lib.qs_tdho_coulomb_vectors(out.data_ptr(), None, l, 0, 0, rank, work.data_ptr(), need.value, stream),
                   "qs_tdho_coulomb_vectors")

    t = runs(call, reps)
    rate = nbytes / (statistics.median(t) * 1e-3) / 1e9
    emit(f"l={l:3d}: rank {rank:4d}  vectors = {nbytes / 1e9:8.4f} GB (u would be {8 * l**4 / 1e9:9.3f} GB)  generate {stats(t)}  "
         f"{rate:7.1f} GB/s of stores ({rate / fill_rate:.2f} of fill)")
    del out, work
    torch.cuda.empty_cache()


def consume(l, reps, with_tensor, emit):
    chol = CholeskyTwoBody(td.get_coulomb_vectors(l))
    gen = torch.Generator(device="cuda").manual_seed(l)
    C = torch.linalg.qr(torch.randn((l, l), dtype=torch.float64, device="cuda", generator=gen))[0].contiguous()
    Co, Cv = C[:, :OCCUPIED].contiguous(), C[:, OCCUPIED:].contiguous()
    rho = (2.0 * Co @ Co.T).contiguous()
    eps = torch.arange(l, dtype=torch.float64, device="cuda")
    eo, ev = eps[:OCCUPIED], eps[OCCUPIED:] + 1.0
    D = eo[:, None, None, None] + eo[None, :, None, None] - ev[None, None, :, None] - ev[None, None, None, :]

    def mp2():
        g = chol.transform_blocks((Co.T, Co.T), (Cv, Cv))
        return (g * (2.0 * g - g.transpose(0, 1)) / D).sum()

    t_mf = runs(lambda: chol.mean_field(rho, cj=1.0, ck=-0.5), reps)
    line = f"l={l:3d}: rank {chol.rank:4d}  mean field on vectors {stats(t_mf)}"
    if with_tensor:
        u = td.get_coulomb_elements(l, method="quadrature")
        t_u = runs(lambda: kernels.mean_field(u, rho, cj=1.0, ck=-0.5), reps)
        diff = float((kernels.mean_field(u, rho, cj=1.0, ck=-0.5) - chol.mean_field(rho, cj=1.0, ck=-0.5)).abs().max())
        line += f"  on u {stats(t_u)}  diff {diff:.1e}"
        del u
        torch.cuda.empty_cache()
    emit(line)
    emit(f"l={l:3d}: MP2 block <ij|ab> ({OCCUPIED} occupied) and its sum {stats(runs(mp2, reps))}")
    chol._Mc = None                    # the materialised M^T is rebuilt by the transform's result, not needed here
    torch.cuda.empty_cache()
    emit(f"l={l:3d}: transform (unitary C) {stats(runs(lambda: chol.transform(C), min(reps, 3), warm=1))}")
    del chol
    torch.cuda.empty_cache()


def basis(l, emit):
    from quantum_systems_amd import TwoDimensionalHarmonicOscillator, hip

    t0 = time.perf_counter()
    b = TwoDimensionalHarmonicOscillator(l, 8.0, 11, coulomb="quadrature", two_body="vectors", np=hip)
    torch.cuda.synchronize()
    emit(f"l={l:3d}: TwoDimensionalHarmonicOscillator(two_body=\"vectors\") built in {time.perf_counter() - t0:8.2f} s "
         f"(host loops included), {b.two_body.L.numel() * 8 / 1e9:.3f} GB held")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--generate", default="55,153,253,528")
    ap.add_argument("--consume", default="253,528")
    ap.add_argument("--tensor", default="253")
    ap.add_argument("--basis", default="")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tdho_vectors_bench needs a GPU: timings are not taken on a CPU")
    fh = open(args.out, "a") if args.out else None

    def emit(line):
        print(line, flush=True)
        if fh:
            fh.write(line + "\n")
            fh.flush()

    emit(f"# tdho_vectors_bench: {torch.cuda.get_device_name(0)}, reps {args.reps}, HIP events around one call, median [min, max]")
    fill_rate = fill_probe(args.reps)
    emit(f"# probe on {PROBE_BYTES >> 30} GiB: fill {fill_rate:.1f} GB/s of stores")
    for l in filter(None, args.generate.split(",")):
        generate(int(l), args.reps, fill_rate, emit)
    tensor = {int(l) for l in filter(None, args.tensor.split(","))}
    for l in filter(None, args.consume.split(",")):
        consume(int(l), args.reps, int(l) in tensor, emit)
    for l in filter(None, args.basis.split(",")):
        basis(int(l), emit)


if __name__ == "__main__":
    main()
