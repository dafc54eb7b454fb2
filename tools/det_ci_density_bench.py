"""Time ``kernels.det_ci_density2`` and ``kernels.det_ci_transition_density1`` on full determinant spaces, next to one
``kernels.det_ci_sigma`` call at the same size.

    python tools/det_ci_density_bench.py [--out FILE] [--reps N] [--cases 24:3,32:4,40:4] [--forms fp64,complex128] [--k 8]

  density2             ONE call on the full space C(m, N): a memset of the m^4 output and C(m,2)^2 workgroups, each of
                       which strides over all dim determinants
  transition_density1  ONE call: m^2 workgroups, the same stride
  sigma                ONE call with K vectors, to set the scale (tools/det_ci_bench.py sweeps it)

One process; after two warm-ups every call runs ``reps`` times, HIP events around each, median [min, max].  "scans" is
workgroups * dim, the determinants a call looks at.  Needs a GPU."""

import argparse
import os
import statistics
import sys
from math import comb

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

import quantum_systems_amd as qs  # noqa: E402
from quantum_systems_amd import kernels  # noqa: E402

from det_ci_bench import hamiltonian, stats, timed  # noqa: E402  (the same clock and the same Hamiltonian)


def measure(call, reps):
    for _ in range(2):
        call()
    torch.cuda.synchronize()
    return [timed(call)[0] for _ in range(reps)]


def run_case(m, N, cplx, K, reps, emit):
    dt = torch.complex128 if cplx else torch.float64
    dets = torch.from_numpy(qs.full_space(m, N)).cuda()
    dim = dets.numel()
    gen = torch.Generator(device="cuda").manual_seed(2)
    vec = torch.empty(2, dim, dtype=dt, device="cuda")
    (torch.view_as_real(vec) if cplx else vec).normal_(generator=gen)
    bra, ket = vec[0].contiguous(), vec[1].contiguous()
    form = "complex128" if cplx else "fp64"
    npair = comb(m, 2)
    emit(f"{form} m={m} N={N}: dim = {dim}, gamma2 = {m ** 4 * bra.element_size() / 1e6:.1f} MB, {npair ** 2} + {m * m} workgroups")
    G = torch.empty(m, m, m, m, dtype=dt, device="cuda")
    rho = torch.empty(m, m, dtype=dt, device="cuda")
    ts = measure(lambda: kernels.det_ci_density2(dets, bra, ket, m, N, out=G), reps)
    med = statistics.median(ts)
    emit(f"  density2:            {stats(ts)}  {npair ** 2 * dim / (med * 1e-3) / 1e9:8.2f} G scans/s  [{kernels.last_dispatch()}]")
    ts = measure(lambda: kernels.det_ci_transition_density1(dets, bra, ket, m, N, out=rho), reps)
    med = statistics.median(ts)
    emit(f"  transition_density1: {stats(ts)}  {m * m * dim / (med * 1e-3) / 1e9:8.2f} G scans/s  [{kernels.last_dispatch()}]")
    ht, ut = hamiltonian(m, cplx, 1)
    diag = kernels.det_ci_diagonal(ht, ut, dets, N)
    ct = torch.empty(dim, K, dtype=dt, device="cuda")                  # K adjacent: read in place
    (torch.view_as_real(ct) if cplx else ct).normal_(generator=gen)
    c = ct.transpose(0, 1)
    ts = measure(lambda: kernels.det_ci_sigma(ht, ut, dets, N, diag, c), reps)
    emit(f"  sigma K={K}:           {stats(ts)}  [{kernels.last_dispatch()}]")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--cases", default="24:3,32:4,40:4")
    ap.add_argument("--forms", default="fp64,complex128")
    ap.add_argument("--k", type=int, default=8)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("det_ci_density_bench needs a GPU: timings are not taken on a CPU")
    fh = open(args.out, "a") if args.out else None

    def emit(line):
        print(line, flush=True)
        if fh:
            fh.write(line + "\n")
            fh.flush()

    emit(f"# det_ci_density_bench: {torch.cuda.get_device_name(0)}, reps {args.reps}, HIP events, median [min, max]")
    for form in args.forms.split(","):
        for case in [x for x in args.cases.split(",") if x]:
            m, N = (int(x) for x in case.split(":"))
            run_case(m, N, form == "complex128", args.k, args.reps, emit)
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
