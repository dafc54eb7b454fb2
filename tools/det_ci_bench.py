"""Time ``kernels.det_ci_sigma`` on full determinant spaces, for every candidate group size G.

    python tools/det_ci_bench.py [--out FILE] [--reps N] [--cases 24:3,32:4,40:4] [--forms fp64,complex128] [--k 8]
                                 [--groups 0,1,2,4,8] [--pair-m 24,32,40]

  sigma   ONE call of kernels.det_ci_sigma on the full space C(m, N) with K vectors: ceil(K / G) launches
  pair    at N = 2, the sigma vector of two_particle.TwoParticleCI at the same m (identity orbitals) next to
          det_ci_sigma on the C(m, 2) determinants: the one comparison inside the project

One process; after two warm-ups every setting runs ``reps`` times, HIP events around each call, median [min, max].
G = 0 is the shipped group size of the form, the others are set through the tuning knob ``det_ci_g``.  "connections" is
dim * (1 + N (m - N) + C(N,2) C(m-N,2)) * K, the matrix elements a call forms and applies (every target of a full
space is found).  Needs a GPU."""

import argparse
import os
import statistics
import sys
from math import comb

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy  # noqa: E402
import torch  # noqa: E402

import quantum_systems_amd as qs  # noqa: E402
from quantum_systems_amd import hip, kernels  # noqa: E402


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b), out


def stats(xs):
    return f"{statistics.median(xs):10.4f} ms [{min(xs):10.4f}, {max(xs):10.4f}]"


def hamiltonian(m, cplx, seed):
    """Hermitian ht and Hermitian anti-symmetrised ut on the device."""
    gen = torch.Generator(device="cuda").manual_seed(seed)
    dt = torch.complex128 if cplx else torch.float64

    def draw(*shape):
        t = torch.empty(shape, dtype=dt, device="cuda")
        (torch.view_as_real(t) if cplx else t).normal_(generator=gen)
        return t

    a = draw(m, m)
    ht = 0.5 * (a + a.conj().T) + torch.diag(torch.arange(m, dtype=torch.float64, device="cuda")).to(dt)
    w = 0.1 * draw(m, m, m, m)
    v = w + w.conj().permute(2, 3, 0, 1)
    v = v + v.permute(1, 0, 3, 2)
    return ht.contiguous(), (v - v.permute(0, 1, 3, 2)).contiguous()


def sweep(call, groups, reps):
    out = []
    for G in groups:
        with kernels.tuning(det_ci_g=G):
            for _ in range(2):
                call()
            torch.cuda.synchronize()
            ts = [timed(call)[0] for _ in range(reps)]
            out.append((G, ts, kernels.last_dispatch()))
    return out


def run_case(m, N, cplx, K, groups, reps, emit):
    ht, ut = hamiltonian(m, cplx, 1)
    dets = torch.from_numpy(qs.full_space(m, N)).cuda()
    dim = dets.numel()
    diag = kernels.det_ci_diagonal(ht, ut, dets, N)
    gen = torch.Generator(device="cuda").manual_seed(2)
    ct = torch.empty(dim, K, dtype=ht.dtype, device="cuda")              # K adjacent: read in place
    (torch.view_as_real(ct) if cplx else ct).normal_(generator=gen)
    c = ct.transpose(0, 1)
    per = 1 + N * (m - N) + comb(N, 2) * comb(m - N, 2)
    form = "complex128" if cplx else "fp64"
    emit(f"{form} m={m} N={N}: dim = {dim}, {per} connections per determinant, ut = {ut.numel() * ut.element_size() / 1e6:.1f} MB")
    for G, ts, ran in sweep(lambda: kernels.det_ci_sigma(ht, ut, dets, N, diag, c), groups, reps):
        med = statistics.median(ts)
        emit(f"  K={K} G={G}: {stats(ts)}  {med / K:10.4f} ms per sigma  {dim * per * K / (med * 1e-3) / 1e9:8.3f} G connections/s  [{ran}]")


def run_pair(m, cplx, K, groups, reps, emit):
    """N = 2: TwoParticleCI.sigma (pair_contract on the untransformed u) against det_ci_sigma on the C(m, 2) determinants."""
    ht, ut = hamiltonian(m, cplx, 3)
    system = qs.GeneralOrbitalSystem(2, qs.setup_basis_set(2, m, hip.asarray(torch.eye(m, dtype=ht.dtype, device="cuda")),
                                                           hip.asarray(ht), hip.asarray(ut), 2, -1, hip, True, True))
    pair = qs.TwoParticleCI(system)
    gen = torch.Generator(device="cuda").manual_seed(4)
    a = torch.empty(K, m, m, dtype=ht.dtype, device="cuda")
    (torch.view_as_real(a) if cplx else a).normal_(generator=gen)
    a = (a - a.transpose(1, 2)).contiguous()
    dets = torch.from_numpy(qs.full_space(m, 2)).cuda()
    diag = kernels.det_ci_diagonal(ht, ut, dets, 2)
    hi = torch.from_numpy(numpy.array([int(x).bit_length() - 1 for x in dets.tolist()])).cuda()
    lo = torch.from_numpy(numpy.array([(int(x) & -int(x)).bit_length() - 1 for x in dets.tolist()])).cuda()
    ct = (a[:, lo, hi] * (2.0 ** 0.5)).transpose(0, 1).contiguous()     # |c> on determinants, K adjacent
    c = ct.transpose(0, 1)
    form = "complex128" if cplx else "fp64"
    emit(f"{form} m={m} N=2: dim = {dets.numel()}")
    for _ in range(2):
        s_pair = pair.sigma(a)
    torch.cuda.synchronize()
    t_pair = [timed(lambda: pair.sigma(a))[0] for _ in range(reps)]
    s_det = kernels.det_ci_sigma(ht, ut, dets, 2, diag, c)
    rel = float((s_det - s_pair[:, lo, hi] * (2.0 ** 0.5)).abs().max() / s_det.abs().max())
    emit(f"  K={K} TwoParticleCI.sigma: {stats(t_pair)}   rel diff of the two routes {rel:.1e}")
    for G, ts, ran in sweep(lambda: kernels.det_ci_sigma(ht, ut, dets, 2, diag, c), groups, reps):
        emit(f"  K={K} G={G} det_ci_sigma:     {stats(ts)}  gain {statistics.median(t_pair) / statistics.median(ts):6.2f}x  [{ran}]")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--cases", default="24:3,32:4,40:4")
    ap.add_argument("--forms", default="fp64,complex128")
    ap.add_argument("--k", type=int, default=8)
    ap.add_argument("--groups", default="0,1,2,4,8")
    ap.add_argument("--pair-m", default="24,32,40")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("det_ci_bench needs a GPU: timings are not taken on a CPU")
    fh = open(args.out, "a") if args.out else None

    def emit(line):
        print(line, flush=True)
        if fh:
            fh.write(line + "\n")
            fh.flush()

    emit(f"# det_ci_bench: {torch.cuda.get_device_name(0)}, reps {args.reps}, HIP events, median [min, max]")
    groups = [int(x) for x in args.groups.split(",")]
    for form in args.forms.split(","):
        cplx = form == "complex128"
        for case in [x for x in args.cases.split(",") if x]:
            m, N = (int(x) for x in case.split(":"))
            run_case(m, N, cplx, args.k, groups, args.reps, emit)
            torch.cuda.empty_cache()
        for m in [int(x) for x in args.pair_m.split(",") if x]:
            run_pair(m, cplx, args.k, groups, args.reps, emit)
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
