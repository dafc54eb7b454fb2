"""Time ``kernels.string_ci_sigma`` (spin-free string CI, one dense product per sigma) next to ``kernels.det_ci_sigma`` on
the S_z sector of the spin-doubled problem.

    python tools/string_ci_bench.py [--out FILE] [--reps 3] [--both 12:2:2,16:2:2,20:2:2] [--alone 12:3:3,14:4:4,16:4:4]
                                    [--forms fp64,complex128] [--k 8]

  both    (m spatial, Na, Nb): ONE string_ci_sigma call on all strings against ONE det_ci_sigma call on
          sz_sector(2 m, Na + Nb, Na - Nb) of the spin-doubled, anti-symmetrised tensor, K vectors each, and the largest
          difference of the two results after ``determinant_order``
  alone   string_ci_sigma only, where the spin-orbital route gets slow or large

One process; after two warm-ups every call runs ``reps`` times, HIP events around each, median [min, max].  The split:
"product" is ``kernels.matmul(W, D)`` alone on a D of the call's shape (the line says whether the dispatcher chose the
kernel it chose inside the sigma call; if not, the subtraction below is only indicative); "streams" = sigma - product
is expand + fold together, whose traffic is counted as m^2 K dim elements written (D), read (G) and the two gathers of
c per element in each of the two kernels, 6 m^2 K dim elements in all.  expand is not an entry of its own in the C
ABI; the nearest one is "density1", ONE ``string_ci_density1`` call = the expand of one vector plus m^2 dot products,
4 m^2 dim elements (D written, D read, the two gathers of the ket).  Needs a GPU."""

import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

import quantum_systems_amd as qs  # noqa: E402
from quantum_systems_amd import kernels  # noqa: E402
from quantum_systems_amd.string_ci import determinant_order, full_strings  # noqa: E402


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b), out


def stats(xs):
    return f"{statistics.median(xs):10.4f} ms [{min(xs):10.4f}, {max(xs):10.4f}]"


def measure(fn, reps):
    for _ in range(2):
        fn()
    torch.cuda.synchronize()
    return [timed(fn)[0] for _ in range(reps)]


def hamiltonian(m, cplx, seed):
    """Hermitian ht and a plain ut with ut[pqrs] = conj(ut[rspq]) = ut[qpsr] on the device."""
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
    return ht.contiguous(), (v + v.permute(1, 0, 3, 2)).contiguous()


def run_case(m, Na, Nb, cplx, K, reps, with_det, emit):
    ht, ut = hamiltonian(m, cplx, 1)
    k = (ht - 0.5 * torch.einsum("pqqr->pr", ut)).contiguous()
    W = (0.5 * ut.permute(0, 2, 1, 3)).reshape(m * m, m * m).contiguous()
    sa, sb = full_strings(m, Na), full_strings(m, Nb)
    ta = kernels.string_ci_table(torch.from_numpy(sa).cuda(), m, Na)
    tb = ta if Na == Nb else kernels.string_ci_table(torch.from_numpy(sb).cuda(), m, Nb)
    na, nb = len(sa), len(sb)
    dim, es = na * nb, (16 if cplx else 8)
    gen = torch.Generator(device="cuda").manual_seed(2)
    c = torch.empty(K, na, nb, dtype=ht.dtype, device="cuda")
    (torch.view_as_real(c) if cplx else c).normal_(generator=gen)
    form = "complex128" if cplx else "fp64"
    emit(f"{form} m={m} Na={Na} Nb={Nb}: {na} x {nb} = {dim} determinants, D and G {2 * m * m * K * dim * es / 1e9:.3f} GB")
    ts = measure(lambda: kernels.string_ci_sigma(k, W, ta, tb, c), reps)
    ran = kernels.last_dispatch()
    D = torch.empty(m * m, K * dim, dtype=ht.dtype, device="cuda")
    (torch.view_as_real(D) if cplx else D).normal_(generator=gen)
    G = torch.empty_like(D)
    tp = measure(lambda: kernels.matmul(W, D, out=G), reps)
    same = any(part.strip() and part.strip() in ran for part in kernels.last_dispatch().split(";"))
    del D, G
    td1 = measure(lambda: kernels.string_ci_density1(ta, tb, m, c[0], c[0]), reps)
    med, medp = statistics.median(ts), statistics.median(tp)
    flop = (8 if cplx else 2) * m ** 4 * K * dim
    emit(f"  K={K} string_ci_sigma: {stats(ts)}  {med / K:10.4f} ms per sigma   [last group: {ran}]")
    emit(f"       product alone:   {stats(tp)}  {flop / (medp * 1e-3) / 1e12:7.2f} Tflop/s  "
         f"({'the kernel of the sigma call' if same else 'NOT the kernel of the sigma call'})")
    emit(f"       density1 (expand of one vector + m^2 dots): {stats(td1)}  "
         f"{4 * m * m * dim * es / (statistics.median(td1) * 1e-3) / 1e12:6.2f} TB/s")
    if med > medp:
        emit(f"       streams (expand + fold) = sigma - product: {med - medp:10.4f} ms, "
             f"{6 * m * m * K * dim * es / ((med - medp) * 1e-3) / 1e12:6.2f} TB/s of D, G and the gathers of c")
    if not with_det:
        return
    masks, perm, phase = determinant_order(sa, sb)
    h2, u2 = kernels.add_spin_one_body(ht), kernels.spin_expand_two_body(ut, antisymmetrize=True)
    dets = torch.from_numpy(masks).cuda()
    N = Na + Nb
    diag = kernels.det_ci_diagonal(h2, u2, dets, N)
    ph, pm = torch.from_numpy(phase).cuda().to(c.dtype), torch.from_numpy(perm).cuda()
    ct = (c.reshape(K, dim) * ph)[:, pm].transpose(0, 1).contiguous()      # K adjacent: read in place
    td = measure(lambda: kernels.det_ci_sigma(h2, u2, dets, N, diag, ct.transpose(0, 1)), reps)
    s_det = kernels.det_ci_sigma(h2, u2, dets, N, diag, ct.transpose(0, 1))
    s_str = (kernels.string_ci_sigma(k, W, ta, tb, c).reshape(K, dim) * ph)[:, pm]
    rel = float((s_det - s_str).abs().max() / s_det.abs().max())
    emit(f"  K={K} det_ci_sigma on {2 * m} spin orbitals: {stats(td)}  string route {statistics.median(td) / med:6.2f}x "
         f"as fast, rel diff of the two routes {rel:.1e}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--both", default="12:2:2,16:2:2,20:2:2")
    ap.add_argument("--alone", default="12:3:3,14:4:4,16:4:4")
    ap.add_argument("--forms", default="fp64,complex128")
    ap.add_argument("--k", type=int, default=8)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("string_ci_bench needs a GPU: timings are not taken on a CPU")
    fh = open(args.out, "a") if args.out else None

    def emit(line):
        print(line, flush=True)
        if fh:
            fh.write(line + "\n")
            fh.flush()

    emit(f"# string_ci_bench: {torch.cuda.get_device_name(0)}, reps {args.reps}, HIP events, median [min, max]")
    for form in args.forms.split(","):
        for with_det, cases in ((True, args.both), (False, args.alone)):
            for case in [x for x in cases.split(",") if x]:
                m, Na, Nb = (int(x) for x in case.split(":"))
                run_case(m, Na, Nb, form == "complex128", args.k, args.reps, with_det, emit)
                torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
