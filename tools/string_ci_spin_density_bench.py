"""Time ``kernels.string_ci_density2_spin`` (the spin-resolved two-body densities as two Gram products of panels that keep
the alpha and the beta replacement apart) next to the spin-summed ``kernels.string_ci_density2`` and to the only route to
the spin blocks that does not use it: ``determinant_order``, ``kernels.det_ci_density2`` on the interleaved determinants of
the spin-doubled problem, and the block slices ``G[a::2, b::2, a::2, b::2]``.

    python tools/string_ci_spin_density_bench.py [--out FILE] [--reps 3] [--cases 10:5:5,12:6:6] [--forms fp64,complex128]
                                                 [--det-max-ms 20000]

One process; after two warm-ups every call runs ``reps`` times, HIP events around each, median [min, max].
  density2_spin  ONE string_ci_density2_spin call (bra is ket), flop/s from 2 (3 m^4 + 2 m^2) dim (times 4 for complex128)
  density2       ONE spin-summed string_ci_density2 call on the same vector, and the ratio of the two
  det route      the comparison leg; its first call is timed alone, and when that takes longer than --det-max-ms it is the
                 only one (the line says so).  The three blocks of the two routes are compared.
Needs a GPU."""

import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from quantum_systems_amd import kernels  # noqa: E402
from quantum_systems_amd.string_ci import determinant_order, full_strings  # noqa: E402

BLOCKS = {"aa": (0, 0), "ab": (0, 1), "bb": (1, 1)}


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


def run_case(m, Na, Nb, cplx, reps, det_max_ms, emit):
    dt = torch.complex128 if cplx else torch.float64
    sa, sb = full_strings(m, Na), full_strings(m, Nb)
    ta = kernels.string_ci_table(torch.from_numpy(sa).cuda(), m, Na)
    tb = ta if Na == Nb else kernels.string_ci_table(torch.from_numpy(sb).cuda(), m, Nb)
    na, nb = len(sa), len(sb)
    dim = na * nb
    gen = torch.Generator(device="cuda").manual_seed(2)
    c = torch.empty((na, nb), dtype=dt, device="cuda")
    (torch.view_as_real(c) if cplx else c).normal_(generator=gen)
    c /= torch.linalg.vector_norm(c)
    rows, passes, T, kc, nbytes = kernels.string_ci_density2_spin_plan(m, na, nb, dt)
    form = "complex128" if cplx else "fp64"
    emit(f"{form} m={m} Na={Na} Nb={Nb}: {na} x {nb} = {dim} determinants; {passes} pass(es) of {rows} rows, T = {T} slices of "
         f"kc = {kc}, workspace {nbytes / 1e9:.3f} GB")
    t3 = measure(lambda: kernels.string_ci_density2_spin(ta, tb, m, c, c), reps)
    ran = kernels.last_dispatch()
    med = statistics.median(t3)
    flop = (8 if cplx else 2) * (3 * m ** 4 + 2 * m * m) * dim
    emit(f"  density2_spin: {stats(t3)}  {flop / (med * 1e-3) / 1e12:7.2f} Tflop/s   [{ran}]")
    t2 = measure(lambda: kernels.string_ci_density2(ta, tb, m, c, c), reps)
    med2 = statistics.median(t2)
    emit(f"  density2:      {stats(t2)}  (spin-summed); density2_spin takes {med / med2:6.2f}x as long")

    masks, perm, phase = determinant_order(sa, sb)
    dets = torch.from_numpy(masks).cuda()
    ph, pm = torch.from_numpy(phase).cuda().to(dt), torch.from_numpy(perm).cuda()
    v = (c.reshape(-1) * ph)[pm].contiguous()

    def det_route():
        G = kernels.det_ci_density2(dets, v, v, 2 * m, Na + Nb)
        return [G[a::2, b::2, a::2, b::2].contiguous() for a, b in BLOCKS.values()]

    first, Gd = timed(det_route)
    if first > det_max_ms:
        td, note = [first], f"ONE call only (it took longer than {det_max_ms} ms)"
    else:
        td, note = [timed(det_route)[0] for _ in range(reps)], f"first call {first:.1f} ms, then {reps}"
    Gs = kernels.string_ci_density2_spin(ta, tb, m, c, c)[:3]
    rel = max(float((x - y).abs().max() / y.abs().max()) for x, y in zip(Gs, Gd))
    emit(f"  det route on {2 * m} spin orbitals (det_ci_density2 + block slices): {stats(td)}  ({note}); "
         f"string route {statistics.median(td) / med:8.2f}x as fast, largest rel diff of the three blocks {rel:.1e}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--cases", default="10:5:5,12:6:6")
    ap.add_argument("--forms", default="fp64,complex128")
    ap.add_argument("--det-max-ms", type=float, default=20000.0)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("string_ci_spin_density_bench needs a GPU: timings are not taken on a CPU")
    fh = open(args.out, "a") if args.out else None

    def emit(line):
        print(line, flush=True)
        if fh:
            fh.write(line + "\n")
            fh.flush()

    emit(f"# string_ci_spin_density_bench: {torch.cuda.get_device_name(0)}, reps {args.reps}, HIP events, median [min, max]")
    for form in args.forms.split(","):
        for case in [x for x in args.cases.split(",") if x]:
            m, Na, Nb = (int(x) for x in case.split(":"))
            run_case(m, Na, Nb, form == "complex128", args.reps, args.det_max_ms, emit)
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
