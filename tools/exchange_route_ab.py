"""Same-process A/B of the transform's exchange-symmetry route against the plain route, and the route's phases.

    python tools/exchange_route_ab.py --sizes 160,192,224,256 --dtype f64 [--blocks 32,64,128] [--blocks-d 8,16,64]
                                      [--pairs 0,1] [--orders 0,2] [--leading 0,2] [--upper 0,2,3] [--reps 5]
                                      [--phases [--c-blocks 16,64]]

Per size: one symmetric tensor (bench.make_inputs), then the plain route (`exchange=0`) and every (block, block_d)
of the forced route (`exchange=2`) in ALTERNATING repetitions (NOTES.md "How to measure here"), HIP-event time per
call; the route's time includes the check kernel and its read-back, as `kernels.transform_two_body` pays them.
`--phases` replays the route's launches one phase at a time through `qs_matmul` / `qs_exchange_mirror` with an event
pair around each (the phases of qs_api.hip's transform_two_body_exchange_route, same shapes and strides): d and c both as
the launches per block / per row of `exchange_pairs=0` and as the one triangular-batch launch (`qs_matmul_pairs`) of
`exchange_pairs=1`.  `--pairs 0,1` times the whole route at both settings of that key, `--orders 0,2` at both orders of the contractions
(`exchange_order`); `--phases` then replays each of those orders' launches.  `--leading 0,2` times order 2 with its leading
indices as one product and the closing blocks, and on pairs between the two transposes (`exchange_leading`); with 2 in
the list `--phases` also replays the pair movers and the two products between them, and prints the total of either form.
`--upper 0,2` times order 2 with its leading indices on the column triangle (`exchange_upper`: two `qs_matmul_upper`
products and the fill); with 2 in the list `--phases` replays those three launches too.  `--upper 3` is that form without
the fill (`exchange_upper=2` and `exchange_lower=2`: the d launch takes the blocks below the block diagonal from the mirror
pair, `qs_matmul_pairs_lower`; 2 alone keeps the fill); with 3 in the list `--phases` adds that d launch where it exists."""

import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def timed(torch, fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def med(xs):
    s = sorted(xs)
    return s[len(s) // 2] if len(s) % 2 else 0.5 * (s[len(s) // 2 - 1] + s[len(s) // 2])


def phases(torch, K, u, C, Ct, out, blk, blk_d, reps, c_blocks=(), other_order=False, order=0, leading_pairs=False,
           leading_upper=False, lower_d=False):
    """The route's launches, phase by phase (T1 and X in one spare buffer, T2 in `out`), in the order `order` takes (0: d, c,
    mirror, a, closing, mirror; 2: a, closing, d, c, mirror -- X1 and Y in the spare buffer, X2 in `out`).  `c_blocks`: also time the c phase
    with every row a of a block [a0, a1) batched over b >= a0 instead of b >= a (needs blk_d to divide those blocks)."""
    L = C.shape[0]
    dt = u.dtype
    W = torch.empty(L**4, dtype=dt, device=u.device)
    CT = C.t().contiguous()
    scratch = torch.zeros(4, dtype=torch.int32, device=u.device)
    lib = K._lib.load()
    code = K.dtype_code(dt)
    st = K._stream()
    L2, L3 = L * L, L**3

    def check():
        assert lib.qs_two_body_exchange_symmetric(code, u.data_ptr(), L, scratch.data_ptr(), st) == 1

    def d(src=u):
        for a0 in range(0, L, blk_d):
            rows = min(L, a0 + blk_d) - a0
            K.gemm_raw(dt, src, C, W, (L - a0) * L, L, L, L, L, L, rows, L3, 0, L3,
                       a_off=a0 * L3 + a0 * L2, c_off=a0 * L3 + a0 * L2)

    def c(cb=1):
        for a in range(L):
            b0 = a // cb * cb
            K.gemm_raw(dt, CT, W, out, L, L, L, L, L, L, L - b0, 0, L2, L2, b_off=(a * L + b0) * L2, c_off=(a * L + b0) * L2)

    def d_pairs(src=u, dst=W, small=C, lower=False):
        K.gemm_raw(dt, src, small, dst, L, L, L, L, L, L, 0, L2, 0, L2, pairs=L, lower=lower)

    def c_pairs(mirror=False, src=W, dst=out, small=CT):
        K.gemm_raw(dt, small, src, dst, L, L, L, L, L, L, 0, 0, L2, L2, pairs=L, mirror=mirror)

    def a_(src=out):
        K.gemm_raw(dt, Ct, src, W, L, L3, L, L, L3, L3)

    def b():
        for p0 in range(0, L, blk):
            rows = min(L, p0 + blk) - p0
            K.gemm_raw(dt, Ct, W, out, L - p0, L2, L, L, L2, L2, rows, 0, L3, L3,
                       a_off=p0 * L, b_off=p0 * L3, c_off=p0 * L3 + p0 * L2)

    def b_full():      # the other order: b as one full product, then a per block of rows p on the columns q >= p0
        K.gemm_raw(dt, Ct, out, W, L, L2, L, L, L2, L2, L, 0, L3, L3)

    def a_blocks():
        for p0 in range(0, L, blk):
            rows = min(L, p0 + blk) - p0
            K.gemm_raw(dt, Ct, W, out, rows, (L - p0) * L2, L, L, L3, L3, a_off=p0 * L, b_off=p0 * L2, c_off=p0 * L3 + p0 * L2)

    mirror = lambda block: K.exchange_mirror_(out.view(L, L, L, L), block)     # noqa: E731
    if order == 2:
        # exchange_order=2, the leading indices first: a on u, the closing blocks, then d and c on the pairs of X2 (in
        # `out`), and the one mirror of the result over all pairs.  Same buffers: every product reads one and writes the other.
        steps = [("check", check), ("a", lambda: a_(u)), ("closing product", b), ("d, per block", lambda: d(out)),
                 ("d", lambda: d_pairs(out)), ("c, per row", c), ("c", c_pairs), ("mirror out", lambda: mirror(1))]
        if not dt.is_complex and L % 128 == 0:      # where the c launch can store the mirror itself: against "c" + "mirror out"
            steps.append(("c, storing the mirror", lambda: c_pairs(True)))
        if leading_pairs:
            # exchange_leading=2: u turned into W on the pairs d >= c, b (W -> out) and a (out -> W) as the trailing pass with
            # (Ct^T, Ct), and the way back W -> out (X2 on q >= p); in the place of "a" and "closing product"
            CtT, W4 = Ct.t().contiguous(), W.view(L, L, L, L)
            steps += [("pairs: way in", lambda: K.exchange_pair_transpose(u, W4)),
                      ("pairs: b", lambda: d_pairs(W, out, CtT)), ("pairs: a", lambda: c_pairs(False, out, W, Ct)),
                      ("pairs: way back", lambda: K.exchange_pair_transpose_back(W4, out.view(L, L, L, L)))]
        if leading_upper:
            # exchange_upper=2: b' (u -> W) and a' (W -> out) on the column blocks d >= c, then the fill of out's lower triangles
            steps += [("upper: b", lambda: K.matmul_upper(dt, Ct, u, W, L, L, 1, L, L, L2, L2, L, 0, L3, L3)),
                      ("upper: a", lambda: K.matmul_upper(dt, Ct, W, out, L, L, L, L, L, L3, L3, 1)),
                      ("upper: fill", lambda: K.exchange_mirror_lower_(out.view(L, L, L, L)))]
            if lower_d:
                # exchange_lower=2: d on the blocks (G, J >= G) of every pair, in the place of "upper: fill" and "d"
                steps.append(("upper: d, no fill", lambda: d_pairs(out, lower=True)))
    else:
        other = [("other order: b full", b_full), ("other order: a blocks", a_blocks)] if other_order else []
        steps = [("check", check), ("d, per block", d), ("d", d_pairs)] + [(f"c, b >= block {cb}", lambda cb=cb: c(cb)) for cb in c_blocks] + [
            ("c, per row", c), ("c", c_pairs), ("mirror T2", lambda: mirror(1))] + other + [
            ("a", a_), ("closing product", b), ("mirror out", lambda: mirror(blk))]
    print(f"    phases of exchange_order={order}")
    times = {name: [] for name, _ in steps}
    for _ in range(reps + 1):
        for name, fn in steps:
            times[name].append(timed(torch, fn))
    total = 0.0
    for name, _ in steps:
        t = med(times[name][1:])
        total += 0.0 if name.startswith(("c, ", "d, ", "other order", "pairs: ", "upper: ")) else t
        print(f"    phase {name:20s} {t:8.3f} ms   (runs: {' '.join('%.3f' % x for x in times[name][1:])})")
    print(f"    phases total     {total:8.3f} ms")
    if order == 2 and leading_pairs:
        blocks = med(times["a"][1:]) + med(times["closing product"][1:])
        pairs = sum(med(times[name][1:]) for name, _ in steps if name.startswith("pairs: "))
        print(f"    leading indices: a + closing product {blocks:8.3f} ms, on pairs {pairs:8.3f} ms; phases total on pairs {total - blocks + pairs:8.3f} ms")
    if order == 2 and leading_upper:
        blocks = med(times["a"][1:]) + med(times["closing product"][1:])
        upper = sum(med(times[name][1:]) for name, _ in steps if name.startswith("upper: "))
        if lower_d:
            upper -= med(times["upper: d, no fill"][1:])
        print(f"    leading indices: a + closing product {blocks:8.3f} ms, on the column triangle {upper:8.3f} ms; phases total on it {total - blocks + upper:8.3f} ms")
        if lower_d:
            fill, d_old, d_new = (med(times[n][1:]) for n in ("upper: fill", "d", "upper: d, no fill"))
            print(f"    fill + d {fill + d_old:8.3f} ms, d without the fill {d_new:8.3f} ms; phases total on it {total - blocks + upper - fill - d_old + d_new:8.3f} ms")
    del W


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="256")
    ap.add_argument("--dtype", choices=["f64", "c128"], default="f64")
    ap.add_argument("--blocks", default="64")
    ap.add_argument("--blocks-d", default="16")
    ap.add_argument("--pairs", default="1", help="exchange_pairs settings of the route to time, e.g. 0,1")
    ap.add_argument("--orders", default="1", help="exchange_order settings of the route to time, e.g. 0,2 (1: the automatic rule)")
    ap.add_argument("--leading", default="1", help="exchange_leading settings of the route to time, e.g. 0,2 (1: the automatic rule)")
    ap.add_argument("--upper", default="1", help="exchange_upper settings of the route to time, e.g. 0,2 (1: the automatic rule; 3: 2 without the fill, exchange_lower=2)")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--phases", action="store_true")
    ap.add_argument("--other-order", action="store_true", help="with --phases: also time b full, then a per block of rows")
    ap.add_argument("--c-blocks", default="", help="with --phases: also time the c phase at this block granularity")
    args = ap.parse_args()
    import torch

    import bench
    from quantum_systems_amd import kernels as K

    dev = torch.device("cuda:0")
    dtype = torch.float64 if args.dtype == "f64" else torch.complex128
    configs = [(int(b), int(bd), int(pr), int(od), int(ld), int(up)) for b in args.blocks.split(",") for bd in args.blocks_d.split(",") for pr in args.pairs.split(",")
               for od in args.orders.split(",") for ld in args.leading.split(",") for up in args.upper.split(",")]
    for l in [int(x) for x in args.sizes.split(",")]:
        u, C, Ct = bench.make_inputs(torch, l, dtype, dev)
        out = torch.empty_like(u)
        assert K.two_body_exchange_symmetric(u)

        def plain():
            with K.tuning(exchange=0):
                K.transform_two_body(u, C, Ct, out=out)

        def route(b, bd, pr, od, ld, up=1):
            lower = {"exchange_lower": 2} if up == 3 else {}
            with K.tuning(exchange=2, exchange_block=b, exchange_block_d=bd, exchange_pairs=pr, exchange_order=od, exchange_leading=ld,
                          exchange_upper=min(up, 2), **lower):
                K.transform_two_body(u, C, Ct, out=out)

        plain()
        ref = out.clone() if l <= 192 else out[:: max(1, l // 8)].clone()
        route(*configs[0])
        got = out if l <= 192 else out[:: max(1, l // 8)]
        err = (got - ref).abs().max().item() / ref.abs().max().item()
        del ref, got
        runs = {"plain": []}
        for cfg in configs:
            runs[cfg] = []
        for _ in range(args.reps):
            runs["plain"].append(timed(torch, plain))
            for cfg in configs:
                runs[cfg].append(timed(torch, lambda: route(*cfg)))
        base = med(runs["plain"])
        print(f"l={l} {args.dtype}: route vs plain max rel diff {err:.2e}")
        print(f"  plain                       median {base:8.3f} ms   runs {' '.join('%.3f' % x for x in runs['plain'])}")
        for cfg in configs:
            m = med(runs[cfg])
            print(f"  route block={cfg[0]:3d} block_d={cfg[1]:3d} pairs={cfg[2]} order={cfg[3]} leading={cfg[4]} upper={cfg[5]} median {m:8.3f} ms   runs {' '.join('%.3f' % x for x in runs[cfg])}"
                  f"   plain/route {base / m:.3f}")
        sys.stdout.flush()
        if args.phases:
            for od in sorted({cfg[3] for cfg in configs}):       # (1, the automatic rule, reads as the order it takes here)
                if od == 1:
                    route(configs[0][0], configs[0][1], 1, 1, 0, 0)
                    od = 2 if K.last_dispatch().count("exchange_transpose_kernel") == 1 else 0
                phases(torch, K, u, C, Ct, out, configs[0][0], configs[0][1], args.reps,
                       [int(x) for x in args.c_blocks.split(",") if x], args.other_order, od,
                       leading_pairs=od == 2 and any(cfg[4] == 2 for cfg in configs),
                       leading_upper=od == 2 and not dtype.is_complex and any(cfg[5] >= 2 for cfg in configs),
                       lower_d=od == 2 and not dtype.is_complex and l % 128 == 0 and any(cfg[5] == 3 for cfg in configs))
        del u, out
        K.workspace.release()
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
