"""Time ``kernels.string_ci_density2`` (the spin-summed two-body density as one Gram product of two expanded panels) and
``kernels.string_ci_spin_squared``, next to the only route to the same Gamma that does not use them: ``to_determinants``
order, ``kernels.det_ci_density2`` on the interleaved determinants of the spin-doubled problem, and the spin sum
``sum_(sigma, tau) G[2p+sigma, 2q+tau, 2r+sigma, 2s+tau]``.

    python tools/string_ci_density_bench.py [--out FILE] [--reps 3] [--cases 10:5:5,12:6:6] [--forms fp64,complex128]
                                            [--k 8] [--det-max-ms 20000]

One process; after two warm-ups every call runs ``reps`` times, HIP events around each, median [min, max].
  density2      ONE string_ci_density2 call (bra is ket), flop/s from 2 m^4 dim (8 m^4 dim for complex128)
  product       the batched product of the call's schedule alone (``qs_string_ci_density2_plan``: one pass only, so this
                line is printed only when the schedule has one pass) on panels of the same shape with random entries;
                "expand + close" = density2 - product is the two expansions, the zero fill and the closing kernel together
  spin_squared  ONE string_ci_spin_squared call on K vectors, gathers/s from m^2 K dim
  det route     the comparison leg; its first call is timed alone, and when that takes longer than --det-max-ms it is the
                only one (the line says so).  The two Gammas are compared.
Needs a GPU."""

import argparse
import ctypes
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from quantum_systems_amd import _lib, kernels  # noqa: E402
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


def normal(shape, dt, gen):
    t = torch.empty(shape, dtype=dt, device="cuda")
    (torch.view_as_real(t) if dt == torch.complex128 else t).normal_(generator=gen)
    return t


def run_case(m, Na, Nb, cplx, K, reps, det_max_ms, emit):
    dt = torch.complex128 if cplx else torch.float64
    sa, sb = full_strings(m, Na), full_strings(m, Nb)
    ta = kernels.string_ci_table(torch.from_numpy(sa).cuda(), m, Na)
    tb = ta if Na == Nb else kernels.string_ci_table(torch.from_numpy(sb).cuda(), m, Nb)
    na, nb = len(sa), len(sb)
    dim, m2, es = na * nb, m * m, (16 if cplx else 8)
    gen = torch.Generator(device="cuda").manual_seed(2)
    c = normal((K, na, nb), dt, gen)
    c[0] /= torch.linalg.vector_norm(c[0])
    plan = (ctypes.c_int64 * 5)()
    _lib.load().qs_string_ci_density2_plan(1 if cplx else 0, m, na, nb, kernels.STRING_CI_BYTES, ctypes.cast(plan, ctypes.c_void_p))
    rows, passes, T, kc, nbytes = tuple(plan)
    form = "complex128" if cplx else "fp64"
    emit(f"{form} m={m} Na={Na} Nb={Nb}: {na} x {nb} = {dim} determinants; {passes} pass(es) of {rows} rows, T = {T} slices of "
         f"kc = {kc}, workspace {nbytes / 1e9:.3f} GB")
    t2 = measure(lambda: kernels.string_ci_density2(ta, tb, m, c[0], c[0]), reps)
    ran = kernels.last_dispatch()
    med = statistics.median(t2)
    flop = (8 if cplx else 2) * m ** 4 * dim
    emit(f"  density2:     {stats(t2)}  {flop / (med * 1e-3) / 1e12:7.2f} Tflop/s   [{ran}]")
    if passes == 1:
        pitch = T * kc
        A, B = normal(((m2 + 1) * pitch,), dt, gen), normal((pitch * m2,), dt, gen)
        part = torch.empty(T * (m2 + 1) * m2, dtype=dt, device="cuda")
        tp = measure(lambda: kernels.gemm_raw(dt, A, B, part, m2 + 1, m2, kc, pitch, m2, m2, batch=T, sa=kc, sb=kc * m2,
                                              sc=(m2 + 1) * m2), reps)
        medp = statistics.median(tp)
        same = any(p.strip() and p.strip() in ran for p in kernels.last_dispatch().split(";"))
        emit(f"  product:      {stats(tp)}  {flop / (medp * 1e-3) / 1e12:7.2f} Tflop/s   "
             f"({'the kernel of the density2 call' if same else 'NOT the kernel of the density2 call'}: {kernels.last_dispatch()})")
        if med > medp:
            emit(f"  expand + close = density2 - product: {med - medp:10.4f} ms, "
                 f"{(2 * m2 + 1) * dim * es / ((med - medp) * 1e-3) / 1e12:6.2f} TB/s of the two panels written")
        del A, B, part
    ts = measure(lambda: kernels.string_ci_spin_squared(ta, tb, m, Na, Nb, c), reps)
    emit(f"  spin_squared: {stats(ts)}  K = {K}, {m2 * K * dim / (statistics.median(ts) * 1e-3) / 1e9:8.2f} G gathers/s")

    masks, perm, phase = determinant_order(sa, sb)
    dets = torch.from_numpy(masks).cuda()
    ph, pm = torch.from_numpy(phase).cuda().to(dt), torch.from_numpy(perm).cuda()
    v = (c[0].reshape(-1) * ph)[pm].contiguous()

    def det_route():
        G = kernels.det_ci_density2(dets, v, v, 2 * m, Na + Nb)
        return sum(G[a::2, b::2, a::2, b::2] for a in (0, 1) for b in (0, 1))

    first, Gd = timed(det_route)
    if first > det_max_ms:
        td, note = [first], f"ONE call only (it took longer than {det_max_ms} ms)"
    else:
        td, note = [timed(det_route)[0] for _ in range(reps)], f"first call {first:.1f} ms, then {reps}"
    Gs, _ = kernels.string_ci_density2(ta, tb, m, c[0], c[0])
    rel = float((Gs - Gd).abs().max() / Gd.abs().max())
    emit(f"  det route on {2 * m} spin orbitals (det_ci_density2 + spin sum): {stats(td)}  ({note}); "
         f"string route {statistics.median(td) / med:8.2f}x as fast, rel diff of the two Gammas {rel:.1e}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--cases", default="10:5:5,12:6:6")
    ap.add_argument("--forms", default="fp64,complex128")
    ap.add_argument("--k", type=int, default=8)
    ap.add_argument("--det-max-ms", type=float, default=20000.0)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("string_ci_density_bench needs a GPU: timings are not taken on a CPU")
    fh = open(args.out, "a") if args.out else None

    def emit(line):
        print(line, flush=True)
        if fh:
            fh.write(line + "\n")
            fh.flush()

    emit(f"# string_ci_density_bench: {torch.cuda.get_device_name(0)}, reps {args.reps}, HIP events, median [min, max]")
    for form in args.forms.split(","):
        for case in [x for x in args.cases.split(",") if x]:
            m, Na, Nb = (int(x) for x in case.split(":"))
            run_case(m, Na, Nb, form == "complex128", args.k, args.reps, args.det_max_ms, emit)
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
