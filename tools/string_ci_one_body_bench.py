"""Time ``kernels.string_ci_one_body`` (d one-body operators on a state as one gather, no intermediate) next to the only
route to the same vectors that does not use it: one ``kernels.string_ci_sigma(A_x, 0 W, ...)`` per operator, which expands
m^2 dim elements, multiplies them by an m^2 x m^2 matrix of zeros and folds them again, in passes where the intermediate
is over ``kernels.STRING_CI_BYTES``.

    python tools/string_ci_one_body_bench.py [--out FILE] [--reps 3] [--cases 12:6:6,14:7:7,16:8:8] [--forms fp64,complex128]
                                             [--k 8] [--slow-ms 5000]

One process; after two warm-ups every call runs ``reps`` times, HIP events around each, median [min, max].
  one_body d    ONE string_ci_one_body call on one vector for d = 1, 2, 4 dense random operators; gathers/s from 2 m^2 dim
                table entries per call (each serves the d operators), and bytes/s from the (1 + d) dim elements read once and
                written
  sigma route   ONE string_ci_sigma(A, 0 W) call on the same vector: the time of d = 1, d of them for d operators.  Its
                first call is timed alone, and when that takes longer than --slow-ms it is the only one (the line says so)
  lanczos step  one step of response.lanczos on string_ci_sigma with a random k and W: (time of 3 steps - time of 1) / 2,
                or ONE step where sigma is slow
  spin_squared  ONE string_ci_spin_squared call on K vectors, gathers/s from m^2 K dim: the neighbour gather kernel
Needs a GPU."""

import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from quantum_systems_amd import kernels, response  # noqa: E402
from quantum_systems_amd.string_ci import full_strings  # noqa: E402


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


def guarded(fn, reps, slow_ms):
    """(times, note): the first call alone; more only where it was not slow."""
    first, _ = timed(fn)
    if first > slow_ms:
        return [first], f"ONE call only (it took longer than {slow_ms:.0f} ms)"
    fn()
    torch.cuda.synchronize()
    return [timed(fn)[0] for _ in range(reps)], f"first call {first:.1f} ms, then {reps}"


def normal(shape, dt, gen):
    t = torch.empty(shape, dtype=dt, device="cuda")
    (torch.view_as_real(t) if dt == torch.complex128 else t).normal_(generator=gen)
    return t


def run_case(m, Na, Nb, cplx, K, reps, slow_ms, emit):
    dt = torch.complex128 if cplx else torch.float64
    sa, sb = full_strings(m, Na), full_strings(m, Nb)
    ta = kernels.string_ci_table(torch.from_numpy(sa).cuda(), m, Na)
    tb = ta if Na == Nb else kernels.string_ci_table(torch.from_numpy(sb).cuda(), m, Nb)
    na, nb = len(sa), len(sb)
    dim, m2, es = na * nb, m * m, (16 if cplx else 8)
    gen = torch.Generator(device="cuda").manual_seed(2)
    c = normal((na, nb), dt, gen)
    c /= torch.linalg.vector_norm(c)
    A = normal((4, m, m), dt, gen)
    A = A + A.conj().transpose(1, 2)
    _, passes, _, work = kernels.string_ci_sigma_plan(m, na, nb, dt)
    form = "complex128" if cplx else "fp64"
    emit(f"{form} m={m} Na={Na} Nb={Nb}: {na} x {nb} = {dim} determinants, a vector of {dim * es / 1e9:.3f} GB; "
         f"sigma in {passes} pass(es), workspace {work / 1e9:.3f} GB")
    med = {}
    for d in (1, 2, 4):
        out = torch.empty((d, na, nb), dtype=dt, device="cuda")
        Ad = A[:d].contiguous()
        ts = measure(lambda: kernels.string_ci_one_body(Ad, ta, tb, m, c, out=out), reps)
        med[d] = statistics.median(ts)
        emit(f"  one_body d={d}: {stats(ts)}  {2 * m2 * dim / (med[d] * 1e-3) / 1e9:8.2f} G gathers/s, "
             f"{(1 + d) * dim * es / (med[d] * 1e-3) / 1e12:6.3f} TB/s of c and out   [{kernels.last_dispatch()}]")
        del out
    W0 = torch.zeros(m2, m2, dtype=dt, device="cuda")
    A0 = A[0].contiguous()
    tsig, note = guarded(lambda: kernels.string_ci_sigma(A0, W0, ta, tb, c), reps, slow_ms)
    sig = statistics.median(tsig)
    rel = float((kernels.string_ci_one_body(A0, ta, tb, m, c) - kernels.string_ci_sigma(A0, W0, ta, tb, c)).abs().max() /
                kernels.string_ci_one_body(A0, ta, tb, m, c).abs().max()) if len(tsig) > 1 else float("nan")
    emit(f"  sigma route (string_ci_sigma(A, 0 W), one operator): {stats(tsig)}  ({note}); one_body is "
         + ", ".join(f"{d * sig / med[d]:8.1f}x as fast for d={d}" for d in (1, 2, 4)) + f"; rel diff of the two results {rel:.1e}")
    k = A0
    W = normal((m2, m2), dt, gen)
    W = (W + W.conj().transpose(0, 1)) * (0.1 / m2)

    def sigma(V):
        return kernels.string_ci_sigma(k, W, ta, tb, V.reshape(V.shape[0], na, nb)).reshape(V.shape[0], dim)

    phi = kernels.string_ci_one_body(A[1].contiguous(), ta, tb, m, c)
    if len(tsig) > 1:
        t1 = measure(lambda: response.lanczos(sigma, phi, 1), reps)
        t3 = measure(lambda: response.lanczos(sigma, phi, 3), reps)
        step = (statistics.median(t3) - statistics.median(t1)) / 2
        emit(f"  lanczos step: {step:10.4f} ms  (3 steps {stats(t3)}, 1 step {stats(t1)}); the start vector costs "
             f"{100 * med[1] / step:5.2f} % of one step")
    else:
        t1, _ = timed(lambda: response.lanczos(sigma, phi, 1))
        emit(f"  lanczos step: {t1:10.4f} ms  (ONE step, timed once: sigma is slow here); the start vector costs "
             f"{100 * med[1] / t1:5.2f} % of it")
    del W0, W, phi
    cK = normal((K, na, nb), dt, gen)
    ts = measure(lambda: kernels.string_ci_spin_squared(ta, tb, m, Na, Nb, cK), reps)
    emit(f"  spin_squared: {stats(ts)}  K = {K}, {m2 * K * dim / (statistics.median(ts) * 1e-3) / 1e9:8.2f} G gathers/s")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--cases", default="12:6:6,14:7:7,16:8:8")
    ap.add_argument("--forms", default="fp64,complex128")
    ap.add_argument("--k", type=int, default=8)
    ap.add_argument("--slow-ms", type=float, default=5000.0)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("string_ci_one_body_bench needs a GPU: timings are not taken on a CPU")
    fh = open(args.out, "a") if args.out else None

    def emit(line):
        print(line, flush=True)
        if fh:
            fh.write(line + "\n")
            fh.flush()

    emit(f"# string_ci_one_body_bench: {torch.cuda.get_device_name(0)}, reps {args.reps}, HIP events, median [min, max]")
    for form in args.forms.split(","):
        for case in [x for x in args.cases.split(",") if x]:
            m, Na, Nb = (int(x) for x in case.split(":"))
            run_case(m, Na, Nb, form == "complex128", args.k, args.reps, args.slow_ms, emit)
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
