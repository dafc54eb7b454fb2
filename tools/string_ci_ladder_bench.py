"""Time ``kernels.string_ci_ladder`` (d combinations of ladder operators of one spin on a state as one gather into the
neighbouring sector, no intermediate) and one Lanczos step of ``response.lanczos`` on ``kernels.string_ci_sigma`` in that
sector.  There is no other route to the same vectors in the package to compare with.

    python tools/string_ci_ladder_bench.py [--out FILE] [--reps 3] [--cases 12:6:6,14:7:7,16:8:8] [--forms fp64,complex128]
                                           [--steps -1] [--slow-ms 5000]

One process; after two warm-ups every call runs ``reps`` times, HIP events around each, median [min, max].
  ladder d      ONE string_ci_ladder call on one vector: d = 1 and d = 4 dense random phi, and d = m with phi = 1 (all
                a_p c at once, three or four operator groups in each of which most p have no coefficient).  Bytes: one read of
                every row of c that a workgroup touches -- for alpha, per operator group and target string one row of nb
                elements per table entry with a coefficient in the group; for beta, per operator group and alpha string the
                row c[Ia, :] -- plus one write of out; the write alone is printed next to it
  lanczos step  one step of response.lanczos on string_ci_sigma in the neighbouring sector with a random k and W:
                (time of 3 steps - time of 1) / 2, or ONE step, timed once, where the first takes longer than --slow-ms
Needs a GPU."""

import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from quantum_systems_amd import kernels, response  # noqa: E402
from quantum_systems_amd.string_ci import full_strings  # noqa: E402

GROUP = 4       # operators per workgroup of the ladder kernel


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


def model_bytes(table, phi, spin, shape_s, shape_t, es):
    """(read, write) bytes of one call on one vector under the model of the module docstring."""
    d, m = phi.shape
    hit = (table != 0).to(torch.float64)                                   # (n_t, m)
    read = 0
    for x0 in range(0, d, GROUP):
        live = (phi[x0:x0 + GROUP] != 0).any(dim=0).to(torch.float64)      # (m,)
        if spin == 0:
            read += int((hit @ live).sum().item()) * shape_s[1] * es
        elif bool(live.any()):
            read += shape_s[0] * shape_s[1] * es
    return read, d * shape_t[0] * shape_t[1] * es


def run_case(m, Na, Nb, cplx, step, reps, slow_ms, emit):
    dt = torch.complex128 if cplx else torch.float64
    es = 16 if cplx else 8
    form = "complex128" if cplx else "fp64"
    gen = torch.Generator(device="cuda").manual_seed(2)
    lists = {N: torch.from_numpy(full_strings(m, N)).cuda() for N in {Na, Nb, Na + step, Nb + step} if 0 <= N <= m}
    shape_s = (lists[Na].numel(), lists[Nb].numel())
    c = normal(shape_s, dt, gen)
    c /= torch.linalg.vector_norm(c)
    emit(f"{form} m={m} Na={Na} Nb={Nb} step {step:+d}: {shape_s[0]} x {shape_s[1]} = {shape_s[0] * shape_s[1]} determinants, "
         f"a vector of {shape_s[0] * shape_s[1] * es / 1e9:.3f} GB")
    for spin in (0, 1):
        N_s = (Na, Nb)[spin]
        if N_s + step not in lists:
            continue
        table = kernels.string_ci_ladder_table(lists[N_s + step], lists[N_s], m)
        n_t = table.shape[0]
        shape_t = (n_t, shape_s[1]) if spin == 0 else (shape_s[0], n_t)
        for d, what in ((1, "random phi"), (4, "random phi"), (m, "phi = 1")):
            phi = torch.eye(m, dtype=dt, device="cuda") if d == m else normal((d, m), dt, gen)
            out = torch.empty((d,) + shape_t, dtype=dt, device="cuda")
            ts = measure(lambda: kernels.string_ci_ladder(phi, table, spin, Na, c, out=out), reps)
            med = statistics.median(ts) * 1e-3
            read, write = model_bytes(table, phi, spin, shape_s, shape_t, es)
            emit(f"  ladder spin {spin} -> {shape_t[0]} x {shape_t[1]}, d={d:2d} ({what}): {stats(ts)}  {(read + write) / med / 1e12:6.3f} TB/s of "
                 f"{(read + write) / 1e9:8.3f} GB read and written, the write of {write / 1e9:8.3f} GB alone {write / med / 1e12:6.3f} TB/s   "
                 f"[{kernels.last_dispatch()}]")
            del out
        if spin == 0:
            lanczos_step(m, (Na, Nb), spin, step, lists, table, c, dt, gen, reps, slow_ms, emit)
        del table
        torch.cuda.empty_cache()


def lanczos_step(m, N, spin, step, lists, table, c, dt, gen, reps, slow_ms, emit):
    Nt = (N[0] + step, N[1]) if spin == 0 else (N[0], N[1] + step)
    ta = kernels.string_ci_table(lists[Nt[0]], m, Nt[0])
    tb = ta if Nt[0] == Nt[1] else kernels.string_ci_table(lists[Nt[1]], m, Nt[1])
    na, nb = ta.shape[0], tb.shape[0]
    m2 = m * m
    k = normal((m, m), dt, gen)
    k = k + k.conj().transpose(0, 1)
    W = normal((m2, m2), dt, gen)
    W = (W + W.conj().transpose(0, 1)) * (0.1 / m2)

    def sigma(V):
        return kernels.string_ci_sigma(k, W, ta, tb, V.reshape(V.shape[0], na, nb)).reshape(V.shape[0], na * nb)

    phi = kernels.string_ci_ladder(normal((m,), dt, gen), table, spin, N[0], c)
    passes = kernels.string_ci_sigma_plan(m, na, nb, dt)[1]
    first, _ = timed(lambda: response.lanczos(sigma, phi, 1))
    if first > slow_ms:
        emit(f"  lanczos step in ({m},{Nt[0]},{Nt[1]}), {na} x {nb}, sigma in {passes} pass(es): {first:10.4f} ms  (ONE step, timed once: sigma is "
             "slow here)")
        return
    t1 = measure(lambda: response.lanczos(sigma, phi, 1), reps)
    t3 = measure(lambda: response.lanczos(sigma, phi, 3), reps)
    emit(f"  lanczos step in ({m},{Nt[0]},{Nt[1]}), {na} x {nb}, sigma in {passes} pass(es): "
         f"{(statistics.median(t3) - statistics.median(t1)) / 2:10.4f} ms  (3 steps {stats(t3)}, 1 step {stats(t1)})")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--cases", default="12:6:6,14:7:7,16:8:8")
    ap.add_argument("--forms", default="fp64,complex128")
    ap.add_argument("--steps", default="-1", help="-1 removes a particle, 1 adds one; a comma-separated list runs both")
    ap.add_argument("--slow-ms", type=float, default=5000.0)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("string_ci_ladder_bench needs a GPU: timings are not taken on a CPU")
    fh = open(args.out, "a") if args.out else None

    def emit(line):
        print(line, flush=True)
        if fh:
            fh.write(line + "\n")
            fh.flush()

    emit(f"# string_ci_ladder_bench: {torch.cuda.get_device_name(0)}, reps {args.reps}, HIP events, median [min, max]")
    for form in args.forms.split(","):
        for case in [x for x in args.cases.split(",") if x]:
            m, Na, Nb = (int(x) for x in case.split(":"))
            for step in (int(x) for x in args.steps.split(",")):
                run_case(m, Na, Nb, form == "complex128", step, args.reps, args.slow_ms, emit)
                torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
