"""Time ``kernels.string_ci_sigma_sym`` -- sigma on the lower triangle of the intermediate for c = tau c^T -- next to
``kernels.string_ci_sigma`` on the same symmetrised vector, and a ``StringCI.solve`` under a spin parity next to one
without.

    python tools/string_ci_sym_bench.py [--out FILE] [--reps 3] [--pairs 12:6:6] [--forms fp64,complex128]
                                        [--reach 14:7:7,16:8:8:16] [--solve 12:6:6]

  pairs   (m spatial, N, N), K = 1, under the shipped budget: ONE string_ci_sigma_sym call against ONE string_ci_sigma call.
          Per leg the passes, the time, the products alone -- ``kernels.matmul(W, D_p)`` on panels of the passes' extents --
          and "streams" = sigma - products: expand and fold, and for the packed route the symmetrise pass, together.
  reach   (m, N, N[, GiB]): the same pair under the shipped budget, or under ``GiB`` set by the tuning key, one timed call
          after one warm-up; the full route is skipped where its workspace does not fit the device.
  solve   (m, N, N): ``StringCI.solve(2)`` with ``spin_parity=+1`` against ``spin_parity=None`` with as many roots as reach
          two states of even parity (found from a first solve), on a seeded random Hamiltonian with well-separated levels in an orthonormal basis.

One process; HIP events around every call, median [min, max] of ``reps`` after two warm-ups in the pairs leg.  Needs a GPU."""

import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from quantum_systems_amd import kernels  # noqa: E402
from string_ci_bench import measure, stats, timed  # noqa: E402
from string_ci_rows_bench import problem  # noqa: E402


def off(r):
    return r * (r + 1) // 2


def products_alone(W, lengths, reps):
    """One product W . D_p per entry of ``lengths`` (columns), timed as one call."""
    m2 = W.shape[0]
    most = max(lengths)
    flat = torch.empty(2 * m2 * most, dtype=W.dtype, device="cuda")
    (torch.view_as_real(flat) if W.is_complex() else flat).normal_(generator=torch.Generator(device="cuda").manual_seed(3))
    pairs = {n: (flat[:m2 * n].view(m2, n), flat[m2 * most:m2 * most + m2 * n].view(m2, n)) for n in set(lengths)}

    def run():
        for n in lengths:
            kernels.matmul(W, pairs[n][0], out=pairs[n][1])

    return measure(run, reps), kernels.last_dispatch()


def symmetrised(c, tau):
    return (0.5 * (c + tau * c.transpose(0, 1))).contiguous()


def pair_leg(m, N, cplx, reps, emit):
    k, W, t, _, c = problem(m, N, N, cplx)
    n = t.shape[0]
    c = symmetrised(c, 1)
    form = "complex128" if cplx else "fp64"
    flop = (8 if cplx else 2) * m ** 4 * n * n
    rows, passes, _, nbytes = kernels.string_ci_sigma_plan(m, n, n, c.dtype)
    (tri_passes, _, _, tri_bytes), cuts = kernels.string_ci_sigma_sym_plan(m, n, c.dtype)
    emit(f"{form} m={m} N={N}: {n} x {n} = {n * n} determinants, off(n) = {off(n)} packed elements")
    tf = measure(lambda: kernels.string_ci_sigma(k, W, t, t, c), reps)
    full = kernels.string_ci_sigma(k, W, t, t, c)
    ts = measure(lambda: kernels.string_ci_sigma_sym(k, W, t, c, 1), reps)
    ran = kernels.last_dispatch()
    sym = kernels.string_ci_sigma_sym(k, W, t, c, 1)
    assert "string_ci_fold_kernel<" in ran and "qs::ScRect" not in ran, ran
    diff = float((sym - full).abs().max() / full.abs().max())
    pf, route_f = products_alone(W, [min(rows, n - p * rows) * n for p in range(passes)], reps)
    ps, route_s = products_alone(W, [off(b) - off(a) for a, b in zip(cuts, cuts[1:])], reps)
    mf, ms, mpf, mps = (statistics.median(x) for x in (tf, ts, pf, ps))
    emit(f"  string_ci_sigma     {passes:3d} passes, work {nbytes / 1e9:7.3f} GB: {stats(tf)}  {flop / (mf * 1e-3) / 1e12:6.2f} Tflop/s of the full sum")
    emit(f"         products alone: {stats(pf)}   streams (expand + fold): {mf - mpf:10.4f} ms   [{route_f.split(';')[0]}]")
    emit(f"  string_ci_sigma_sym {tri_passes:3d} passes, work {tri_bytes / 1e9:7.3f} GB: {stats(ts)}  {mf / ms:6.3f}x faster, rel diff {diff:.1e}")
    emit(f"         products alone: {stats(ps)}  {mpf / mps:6.3f}x   streams (expand + fold + symmetrise): {ms - mps:10.4f} ms  "
         f"{(mf - mpf) / (ms - mps):6.3f}x   [{route_s.split(';')[0]}]")


def reach_leg(m, N, gib, emit):
    free, total = torch.cuda.mem_get_info()
    k, W, t, _, c = problem(m, N, N, False)
    n = t.shape[0]
    c = symmetrised(c, 1)
    flop = 2 * m ** 4 * n * n
    knobs = {"string_ci_bytes": gib << 30} if gib else {}
    with kernels.tuning(**knobs):
        rows, passes, _, nbytes = kernels.string_ci_sigma_plan(m, n, n, c.dtype)
        (tri_passes, longest, cols, tri_bytes), _ = kernels.string_ci_sigma_sym_plan(m, n, c.dtype)
        emit(f"fp64 m={m} N={N}: {n} x {n} = {n * n} determinants, one vector {c.numel() * 8 / 1e9:.3f} GB; D and G in one piece: full "
             f"{2 * m * m * c.numel() * 8 / 1e9:.1f} GB, packed {2 * m * m * off(n) * 8 / 1e9:.1f} GB; budget "
             f"{'%d GiB' % gib if gib else 'shipped'}; device memory free {free / 1e9:.0f} of {total / 1e9:.0f} GB")
        out = torch.empty_like(c)
        times = {}
        for name, work, fn in (("string_ci_sigma", nbytes, lambda: kernels.string_ci_sigma(k, W, t, t, c, out=out)),
                               ("string_ci_sigma_sym", tri_bytes, lambda: kernels.string_ci_sigma_sym(k, W, t, c, 1, out=out))):
            if work + 3 * c.numel() * 8 > free:
                emit(f"  {name}: NOT RUN, {work / 1e9:.1f} GB of workspace needed")
                continue
            fn()                                                          # warm-up: allocates the workspace
            torch.cuda.synchronize()
            times[name], _ = timed(fn)
            n_pass = passes if name == "string_ci_sigma" else tri_passes
            emit(f"  {name:20s} {n_pass:4d} passes, work {work / 1e9:7.3f} GB: {times[name]:10.2f} ms, "
                 f"{flop / (times[name] * 1e-3) / 1e12:6.2f} Tflop/s of the full sum 2 m^4 dim; finite: {bool(torch.isfinite(out).all())}")
        if len(times) == 2:
            emit(f"  ratio: {times['string_ci_sigma'] / times['string_ci_sigma_sym']:6.3f}x")


def solve_leg(m, N, reps, emit):
    import numpy as np

    import quantum_systems_amd as qsa
    from quantum_systems_amd import StringCI

    rng = np.random.default_rng(12)
    bs = qsa.RandomBasisSet(m, 2)
    a = rng.standard_normal((m, m))
    bs.h = 0.05 * (a + a.T) + np.diag(np.arange(m, dtype=float))           # well-separated levels: Davidson converges
    bs.s = np.eye(m)
    u = 0.02 * rng.standard_normal((m, m, m, m))
    u = u + u.transpose(2, 3, 0, 1)
    bs.u = u + u.transpose(1, 0, 3, 2)
    system = qsa.SpatialOrbitalSystem(2 * N, bs)
    system.change_module(qsa.hip)
    even, plain = StringCI(system, spin_parity=1), StringCI(system)
    n = even.na
    roots = 2
    while True:                                                           # as many roots as hold two states of even parity
        plain.solve(roots)
        parity = [float(torch.vdot(v.reshape(-1), v.transpose(0, 1).reshape(-1)).real) for v in plain._c]
        if sum(p > 0 for p in parity) >= 2:
            break
        roots += 1
    emit(f"solve m={m} N={N}: {n} x {n} determinants; two states of even parity are among the lowest {roots} roots of the sector")
    for name, ci, r in (("spin_parity=+1, solve(2)", even, 2), (f"spin_parity=None, solve({roots})", plain, roots)):
        ts = measure(lambda: ci.solve(r), reps)
        emit(f"  {name:32s}: {stats(ts)}  {ci.iterations} iterations, {sum(ci.sigma_history)} vectors through sigma, converged {ci.converged}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--pairs", default="12:6:6")
    ap.add_argument("--forms", default="fp64,complex128")
    ap.add_argument("--reach", default="")
    ap.add_argument("--solve", default="")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("string_ci_sym_bench needs a GPU: timings are not taken on a CPU")
    fh = open(args.out, "a") if args.out else None

    def emit(line):
        print(line, flush=True)
        if fh:
            fh.write(line + "\n")
            fh.flush()

    emit(f"# string_ci_sym_bench: {torch.cuda.get_device_name(0)}, reps {args.reps}, HIP events, median [min, max]")
    for case in [x for x in args.pairs.split(",") if x]:
        m, N, _ = (int(x) for x in case.split(":"))
        for form in [x for x in args.forms.split(",") if x]:
            pair_leg(m, N, form == "complex128", args.reps, emit)
            torch.cuda.empty_cache()
    for case in [x for x in args.reach.split(",") if x]:
        m, N, _, *gib = (int(x) for x in case.split(":"))
        reach_leg(m, N, gib[0] if gib else 0, emit)
        torch.cuda.empty_cache()
    for case in [x for x in args.solve.split(",") if x]:
        m, N, _ = (int(x) for x in case.split(":"))
        solve_leg(m, N, args.reps, emit)


if __name__ == "__main__":
    main()
