"""Time ``kernels.string_ci_sigma`` where it runs in passes over alpha rows (``qs_string_ci_sigma_rows``): what the passes
cost next to the one-piece route, and the sizes they reach.

    python tools/string_ci_rows_bench.py [--out FILE] [--reps 3] [--budget 12:6:6] [--fractions 4,16,64]
                                         [--forms fp64,complex128] [--reach 14:7:7,16:8:8:16]

  budget  (m spatial, Na, Nb), K = 1: ONE string_ci_sigma call at a byte budget that just holds the D and G of the vector
          (the one-piece entry), then the same call at that budget divided by every one of ``fractions`` (the passes).
          Per leg the passes, the time, the products alone -- ``kernels.matmul(W, D_p)`` on panels of the passes' extents,
          as many as there are passes -- and "streams" = sigma - products: expand and fold together.  The largest difference
          of the result to the one-piece one is printed with each leg.
  reach   (m, Na, Nb[, GiB]): ONE sigma on a random vector under the shipped budget, or under ``GiB`` set by the tuning
          key: its passes, its time (after one warm-up, which also allocates the workspace) and its rate, 2 m^4 dim flop
          per sigma in fp64.

One process; HIP events around every call, median [min, max] of ``reps`` after two warm-ups in the budget leg.  The share
of the fold inside "streams" is not visible to events around a whole call: take it from a kernel trace of one leg
(``--forms fp64 --fractions 16``).  Needs a GPU."""

import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from quantum_systems_amd import _lib, kernels  # noqa: E402
from quantum_systems_amd.string_ci import full_strings  # noqa: E402
from string_ci_bench import hamiltonian, measure, stats, timed  # noqa: E402


def problem(m, Na, Nb, cplx):
    ht, ut = hamiltonian(m, cplx, 1)
    k = (ht - 0.5 * torch.einsum("pqqr->pr", ut)).contiguous()
    W = (0.5 * ut.permute(0, 2, 1, 3)).reshape(m * m, m * m).contiguous()
    ta = kernels.string_ci_table(torch.from_numpy(full_strings(m, Na)).cuda(), m, Na)
    tb = ta if Na == Nb else kernels.string_ci_table(torch.from_numpy(full_strings(m, Nb)).cuda(), m, Nb)
    c = torch.empty(ta.shape[0], tb.shape[0], dtype=ht.dtype, device="cuda")
    (torch.view_as_real(c) if cplx else c).normal_(generator=torch.Generator(device="cuda").manual_seed(2))
    return k, W, ta, tb, c


def products_alone(W, rows, passes, na, nb, reps):
    """``passes`` products W . D_p on panels of the passes' extents (the last pass may be shorter), timed as one call."""
    m2 = W.shape[0]
    flat = torch.empty(2 * m2 * rows * nb, dtype=W.dtype, device="cuda")
    (torch.view_as_real(flat) if W.is_complex() else flat).normal_(generator=torch.Generator(device="cuda").manual_seed(3))
    cols = [min(rows, na - p * rows) * nb for p in range(passes)]
    pairs = {n: (flat[:m2 * n].view(m2, n), flat[m2 * rows * nb:m2 * rows * nb + m2 * n].view(m2, n)) for n in set(cols)}

    def run():
        for n in cols:
            kernels.matmul(W, pairs[n][0], out=pairs[n][1])

    return measure(run, reps), kernels.last_dispatch()


def budget_leg(m, Na, Nb, cplx, fractions, reps, emit):
    k, W, ta, tb, c = problem(m, Na, Nb, cplx)
    na, nb = c.shape
    code = 1 if cplx else 0
    one = _lib.load().qs_string_ci_workspace(code, code, m, na, nb, 1)
    form = "complex128" if cplx else "fp64"
    flop = (8 if cplx else 2) * m ** 4 * na * nb
    emit(f"{form} m={m} Na={Na} Nb={Nb}: {na} x {nb} = {na * nb} determinants, D and G of the vector {one / 1e9:.3f} GB")
    base = None
    for f in [1] + fractions:
        with kernels.tuning(string_ci_bytes=one // f):
            rows, passes, _, nbytes = kernels.string_ci_sigma_plan(m, na, nb, c.dtype)
            ts = measure(lambda: kernels.string_ci_sigma(k, W, ta, tb, c), reps)
            ran = kernels.last_dispatch()
            out = kernels.string_ci_sigma(k, W, ta, tb, c)
        assert (ran.count("string_ci_fold_kernel<") > 1) == (passes > 1) == (f > 1), ran      # (a long log is cut short)
        tp, product = products_alone(W, rows, passes, na, nb, reps)
        med, medp = statistics.median(ts), statistics.median(tp)
        if base is None:
            base, ref = med, out
        diff = float((out - ref).abs().max() / ref.abs().max())
        emit(f"  budget one/{f:<3d} {passes:4d} passes of {rows:4d} rows, work {nbytes / 1e9:6.3f} GB: {stats(ts)}  "
             f"{med / base:6.3f}x the one-piece call, {flop / (med * 1e-3) / 1e12:6.2f} Tflop/s, rel diff {diff:.1e}")
        emit(f"         products alone: {stats(tp)}  {flop / (medp * 1e-3) / 1e12:6.2f} Tflop/s   streams (expand + fold) = "
             f"sigma - products: {med - medp:10.4f} ms = {100 * (med - medp) / med:5.1f} % of the call   [{product.split(';')[0]}]")
        del out
    del ref


def reach_leg(m, Na, Nb, gib, emit):
    free, total = torch.cuda.mem_get_info()
    k, W, ta, tb, c = problem(m, Na, Nb, False)
    na, nb = c.shape
    knobs = {"string_ci_bytes": gib << 30} if gib else {}
    with kernels.tuning(**knobs):
        rows, passes, cols, nbytes = kernels.string_ci_sigma_plan(m, na, nb, c.dtype)
        emit(f"fp64 m={m} Na={Na} Nb={Nb}: {na} x {nb} = {na * nb} determinants, one vector {c.numel() * 8 / 1e9:.3f} GB, its D and G "
             f"in one piece {2 * m * m * c.numel() * 8 / 1e9:.1f} GB; budget {'%d GiB' % gib if gib else 'shipped'}: {passes} passes of "
             f"{rows} rows, {cols} columns per product, work {nbytes / 1e9:.3f} GB; device memory free {free / 1e9:.0f} of {total / 1e9:.0f} GB")
        need = nbytes + 3 * c.numel() * 8
        if need > free:
            emit(f"  NOT RUN: {need / 1e9:.1f} GB needed")
            return
        out = torch.empty_like(c)
        kernels.string_ci_sigma(k, W, ta, tb, c, out=out)                 # warm-up: allocates the workspace
        torch.cuda.synchronize()
        ms, _ = timed(lambda: kernels.string_ci_sigma(k, W, ta, tb, c, out=out))
    flop = 2 * m ** 4 * na * nb
    emit(f"  one sigma: {ms:10.2f} ms, {flop / (ms * 1e-3) / 1e12:6.2f} Tflop/s of 2 m^4 dim = {flop:.3e} flop; finite: "
         f"{bool(torch.isfinite(out).all())}, |sigma| max {float(out.abs().max()):.3e}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--budget", default="12:6:6")
    ap.add_argument("--fractions", default="4,16,64")
    ap.add_argument("--forms", default="fp64,complex128")
    ap.add_argument("--reach", default="")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("string_ci_rows_bench needs a GPU: timings are not taken on a CPU")
    fh = open(args.out, "a") if args.out else None

    def emit(line):
        print(line, flush=True)
        if fh:
            fh.write(line + "\n")
            fh.flush()

    emit(f"# string_ci_rows_bench: {torch.cuda.get_device_name(0)}, reps {args.reps}, HIP events, median [min, max]")
    fractions = [int(x) for x in args.fractions.split(",") if x]
    for case in [x for x in args.budget.split(",") if x]:
        m, Na, Nb = (int(x) for x in case.split(":"))
        for form in [x for x in args.forms.split(",") if x]:
            budget_leg(m, Na, Nb, form == "complex128", fractions, args.reps, emit)
            torch.cuda.empty_cache()
    for case in [x for x in args.reach.split(",") if x]:
        m, Na, Nb, *gib = (int(x) for x in case.split(":"))
        reach_leg(m, Na, Nb, gib[0] if gib else 0, emit)
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
