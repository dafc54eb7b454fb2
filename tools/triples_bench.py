"""Time the parts of the triples correction: the products that form the blocks of a triple, ``kernels.triples_energy`` on
them, a torch restatement of the same reduction on the same blocks, and a whole ``RCCD.triples`` call.

    python tools/triples_bench.py [--out FILE] [--reps N] [--v 64,128,250] [--whole 64:3,128:3,250:3] [--dtype fp64]
    python tools/triples_bench.py --singles [--v 250] [--dtype fp64]      (and --v 120 --dtype complex128)

  products  the six particle and six hole products of ONE triple (``kernels.gemm_raw``, as a pass of ``RCCD.triples``)
  kernel    ONE call of ``kernels.triples_energy`` over n triples of six distinct blocks each, n so that the blocks
            exceed the last-level cache (about 1.5 GB); per triple = the call's time / n
  torch     the same reduction in torch ops on the same blocks: six permuted adds for W, the combination Z, the
            product, the division and the sum, triple by triple
  singles   (``--singles``, instead of the parts above) ``kernels.triples_energy_singles`` against ``kernels.triples_energy``
            on the SAME blocks and slots, alternating in one process; ``A`` (o, v), ``G`` (o^2, v, v) and the ``sslots`` of
            random occupied triples.  The yardstick: the baseline plus the time of one more read of the blocks at the
            rate the baseline reads them
"of copy" is the ``6 v^3`` elements the kernel has to read per triple over its time, against the rate of
``qs_probe_stream_copy`` (read + write counted) measured in the same run.  The whole call builds ``coupled_cluster.RCCD``
on a random closed-shell system of v + o canonical orbitals and times ``triples()`` on its first-order amplitudes; the
kernel's share is its time per triple times the triples of the call over that.  One process; after two warm-ups every
part runs ``reps`` times, HIP events around each, median [min, max].  Needs a GPU."""

import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import torch  # noqa: E402
from rccd_bench import copy_rate, exchange_symmetric_, fill, stats, timed  # noqa: E402  (the protocol of tools/rccd_bench.py)

from quantum_systems_amd import kernels  # noqa: E402


def repeat(fn, reps):
    for _ in range(2):
        out = fn()
    torch.cuda.synchronize()
    return [timed(fn)[0] for _ in range(reps)], out


def torch_restatement(X, slots, eo3, ev):
    """``e`` (n,) of ``kernels.triples_energy`` by torch ops, triple by triple."""
    D0 = -(ev[:, None, None] + ev[None, :, None] + ev[None, None, :])
    out = []
    for row, eo in zip(slots.tolist(), eo3.tolist()):
        W = (X[row[0]] + X[row[1]].permute(0, 2, 1) + X[row[2]].permute(1, 0, 2) + X[row[3]].permute(2, 0, 1)
             + X[row[4]].permute(1, 2, 0) + X[row[5]].permute(2, 1, 0))
        Z = (4 * W + W.permute(2, 0, 1) + W.permute(1, 2, 0) - 2 * W.permute(0, 2, 1) - 2 * W.permute(2, 1, 0)
             - 2 * W.permute(1, 0, 2)) / 3
        out.append(((W.conj() * Z).real / (D0 + eo)).sum())
    return torch.stack(out)


def run_parts(v, o, dt, reps, roof, emit):
    es = 16 if dt == torch.complex128 else 8
    block = v ** 3 * es
    n = max(1, -(-1500000000 // (6 * block)))
    X = fill((6 * n, v, v, v), dt, 1)
    slots = torch.arange(6 * n, dtype=torch.int32, device="cuda").reshape(n, 6)
    ev = torch.arange(v, dtype=torch.float64, device="cuda") * 0.5 + 1.0
    eo3 = -3.0 - torch.rand(n, dtype=torch.float64, device="cuda")
    t_k, e = repeat(lambda: kernels.triples_energy(X, slots, eo3, ev), reps)
    names = kernels.last_dispatch()
    t_t, e_t = repeat(lambda: torch_restatement(X, slots, eo3, ev), reps)
    rel = float((e - e_t).abs().max() / e_t.abs().max())
    # the products of one triple, on operands of the shapes of RCCD.triples
    tp, Vp = fill((o, o, v, v), dt, 2), fill((o, v, v, v), dt, 3)
    th, Hh = fill((o, v, v, o), dt, 4), fill((o, o, o, v), dt, 5)
    v2 = v * v

    def products():
        for x in range(6):
            kernels.gemm_raw(dt, tp, Vp, X, v, v2, v, v, v2, v2, c_off=x * v ** 3)
            kernels.gemm_raw(dt, th, Hh, X, v2, v, o, o, v, v, accumulate=True, c_off=x * v ** 3)

    t_p, _ = repeat(products, reps)
    m_k, m_t, m_p = statistics.median(t_k) / n, statistics.median(t_t) / n, statistics.median(t_p)
    rate = 6 * block / (m_k * 1e-3) / 1e9
    emit(f"v={v} {str(dt).split('.')[-1]}: {n} triples of 6 blocks ({6 * block / 1e6:.1f} MB per triple)  [{names}]")
    emit(f"  kernel   {stats(t_k)} per call, {m_k:9.4f} ms per triple: {rate:7.1f} GB/s read ({rate / roof:.2f} of copy)")
    emit(f"  torch    {stats(t_t)} per call, {m_t:9.4f} ms per triple: kernel {m_t / m_k:6.2f}x faster, rel diff {rel:.1e}")
    emit(f"  products {stats(t_p)} per triple (o = {o}): kernel / products = {m_k / m_p:.2f}")
    del X, tp, Vp, th, Hh
    torch.cuda.empty_cache()
    return m_k


def run_singles(v, o, dt, reps, roof, emit):
    """The singles kernel against the plain one on the same blocks: alternating calls, so that both see the same machine."""
    es = 16 if dt == torch.complex128 else 8
    block = v ** 3 * es
    n = max(1, -(-1500000000 // (6 * block)))
    X = fill((6 * n, v, v, v), dt, 1)
    slots = torch.arange(6 * n, dtype=torch.int32, device="cuda").reshape(n, 6)
    ev = torch.arange(v, dtype=torch.float64, device="cuda") * 0.5 + 1.0
    eo3 = -3.0 - torch.rand(n, dtype=torch.float64, device="cuda")
    A, G = fill((o, v), dt, 7), fill((o * o, v, v), dt, 8)
    gen = torch.Generator(device="cpu").manual_seed(9)
    ijk = torch.randint(0, o, (n, 3), generator=gen)
    orders = ((0, 1, 2), (0, 2, 1), (1, 0, 2), (1, 2, 0), (2, 0, 1), (2, 1, 0))
    sslots = torch.stack([torch.stack([ijk[:, p], ijk[:, q] * o + ijk[:, r]], dim=1) for p, q, r in orders], dim=1)
    sslots = sslots.to(torch.int32).cuda().contiguous()
    plain = lambda: kernels.triples_energy(X, slots, eo3, ev)                              # noqa: E731
    singles = lambda: kernels.triples_energy_singles(X, slots, eo3, ev, A, G, sslots)      # noqa: E731
    for _ in range(2):
        e0, (e1, es1) = plain(), singles()
    names = kernels.last_dispatch()
    torch.cuda.synchronize()
    t_p, t_s = [], []
    for _ in range(reps):
        t_p.append(timed(plain)[0])
        t_s.append(timed(singles)[0])
    same = bool((e0 == e1).all())
    m_p, m_s = statistics.median(t_p) / n, statistics.median(t_s) / n
    rate_p, rate_s = 6 * block / (m_p * 1e-3) / 1e9, 6 * block / (m_s * 1e-3) / 1e9
    emit(f"v={v} o={o} {str(dt).split('.')[-1]}: {n} triples of 6 blocks ({6 * block / 1e6:.1f} MB per triple), A {tuple(A.shape)}, "
         f"G {tuple(G.shape)} ({G.numel() * es / 1e6:.2f} MB)  [{names}]")
    emit(f"  baseline {stats(t_p)} per call, {m_p:9.4f} ms per triple: {rate_p:7.1f} GB/s read ({rate_p / roof:.2f} of copy)")
    emit(f"  singles  {stats(t_s)} per call, {m_s:9.4f} ms per triple: {rate_s:7.1f} GB/s read ({rate_s / roof:.2f} of copy)")
    emit(f"  singles / baseline = {m_s / m_p:.3f} (baseline + one more read of X at the baseline's rate = 2.000); "
         f"e equal bit for bit: {same}; sum es = {float(es1.sum()):.6e}")
    del X, A, G
    torch.cuda.empty_cache()
    return m_s / m_p


def run_whole(v, o, reps, per_triple, emit):
    import numpy as np

    import quantum_systems_amd as qsa
    from quantum_systems_amd import RCCD, hip

    l = v + o
    u = fill((l, l, l, l), torch.float64, 6)
    u.mul_(0.01 / l)
    exchange_symmetric_(u)
    # canonical by construction: h = diag(eps) - (2 J - K) of the occupied orbitals, so that the Fock matrix is diag(eps)
    # (u has the exchange symmetry and nothing else: the timing does not need a Hermitian u)
    eps = 2.0 * torch.arange(l, dtype=torch.float64, device="cuda")
    J = torch.einsum("piqi->pq", u[:, :o, :, :o])
    K = torch.einsum("piiq->pq", u[:, :o, :o, :])
    h = torch.diag(eps) - (2 * J - K)
    bs = qsa.setup_basis_set(2 * o, l, hip.asarray(np.eye(l)), hip.asarray(h), hip.asarray(u), 2, -1, hip, False, False)
    ccd = RCCD(qsa.SpatialOrbitalSystem(2 * o, bs))
    t_w, e_t = repeat(lambda: ccd.triples(canonical_tol=1e-6), reps)
    triples = sum(p[0] for p in ccd.triples_passes)
    m_w = statistics.median(t_w)
    emit(f"RCCD.triples v={v} o={o}: {stats(t_w)}, {len(ccd.triples_passes)} pass(es), {triples} triples, E_T = {e_t:.6e}; "
         f"kernel share {triples * per_triple / m_w:.2f} (at its time per triple above)")
    del ccd, bs, u
    torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--v", default="64,128,250")
    ap.add_argument("--o", type=int, default=3)
    ap.add_argument("--whole", default="64:3,128:3,250:3")
    ap.add_argument("--dtype", default="fp64", choices=["fp64", "complex128"])
    ap.add_argument("--singles", action="store_true", help="time kernels.triples_energy_singles against kernels.triples_energy")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("triples_bench needs a GPU: timings are not taken on a CPU")
    fh = open(args.out, "a") if args.out else None

    def emit(line):
        print(line, flush=True)
        if fh:
            fh.write(line + "\n")
            fh.flush()

    dt = torch.complex128 if args.dtype == "complex128" else torch.float64
    emit(f"# triples_bench: {torch.cuda.get_device_name(0)}, reps {args.reps}, HIP events, median [min, max]")
    roof = copy_rate(args.reps)
    emit(f"# qs_probe_stream_copy on 2 GiB: {roof:.1f} GB/s read + write")
    if args.singles:
        for v in (int(x) for x in filter(None, args.v.split(","))):
            run_singles(v, args.o, dt, args.reps, roof, emit)
        return
    per_triple = {}
    for v in (int(x) for x in filter(None, args.v.split(","))):
        per_triple[v] = run_parts(v, args.o, dt, args.reps, roof, emit)
    for case in filter(None, args.whole.split(",")):
        v, o = (int(x) for x in case.split(":"))
        if v not in per_triple:
            per_triple[v] = run_parts(v, o, torch.float64, args.reps, roof, emit)
        run_whole(v, o, args.reps, per_triple[v], emit)


if __name__ == "__main__":
    main()
