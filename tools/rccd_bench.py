"""Time ``kernels.pair_contract_exchange`` against ``kernels.pair_contract`` on the same tensor and the same amplitudes,
and one RCCD iteration split into its pass over ``u`` and the rest.

    python tools/rccd_bench.py [--out FILE] [--reps N] [--cases fp64:110,fp64:156,...] [--k 15,66] [--rccd 110:5,156:11,256:11]

  exchange  ONE call of kernels.pair_contract_exchange(u, T): reads r <= s of every row of u, (l + 1) / (2 l) of its bytes
  full      ONE call of kernels.pair_contract(u, T): reads all of u

``u`` is random with particle-exchange symmetry (bit for bit) and nothing else, ``T`` generic, so the two routes compute
the same S ("rel diff" is taken on all of it).  The protocol is that of tools/ccd_bench.py: one process; after two
warm-ups the two routes alternate ``reps`` times, HIP events around each, median [min, max].  "of copy" is the bytes
the route has to read per group pass over its median time, against the rate of ``qs_probe_stream_copy`` (read + write
counted) measured in the same run.  "holds" is the rule for the default ladder: the slowest exchange run beats the
fastest full run.  The RCCD part builds ``coupled_cluster.RCCD`` on a random closed-shell system of l spatial orbitals,
n of them doubly occupied, in non-canonical orbitals and times ``_ladder`` (back-transform, pass, two forward
transforms) and the whole residual under both ladder routes.  Needs a GPU."""

import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from quantum_systems_amd import _lib, kernels  # noqa: E402

DEFAULT = "fp64:110,fp64:156,fp64:256,complex128:110"


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b), out


def fill(shape, dtype, seed):
    gen = torch.Generator(device="cuda").manual_seed(seed)
    t = torch.empty(shape, dtype=dtype, device="cuda")
    flat = torch.view_as_real(t).reshape(-1) if t.is_complex() else t.reshape(-1)
    step = 1 << 28
    for i in range(0, flat.numel(), step):
        flat[i:i + step].normal_(generator=gen)
    return t


def exchange_symmetric_(u):
    """In place, no copy of u: u[p,q,r,s] = u[q,p,s,r] bit for bit (the rows p > q from their mirrors, the rows p = q
    made symmetric in (r, s))."""
    for p in range(u.shape[0]):
        u[p, p] = u[p, p] + u[p, p].transpose(0, 1)
    kernels.exchange_mirror_(u)
    assert kernels.two_body_exchange_symmetric(u)
    return u


def stats(xs):
    return f"{statistics.median(xs):9.4f} ms [{min(xs):9.4f}, {max(xs):9.4f}]"


def copy_rate(reps):
    """GB/s of the 16-byte-per-lane device copy on 2 GiB (read + write counted)."""
    lib = _lib.load()
    n = 1 << 31
    src, dst = torch.empty(n, dtype=torch.uint8, device="cuda"), torch.empty(n, dtype=torch.uint8, device="cuda")
    src.zero_()
    stream = torch.cuda.current_stream().cuda_stream
    ts = []
    for i in range(reps + 2):
        t = timed(lambda: _lib.check(lib.qs_probe_stream_copy(src.data_ptr(), dst.data_ptr(), n, stream), "copy"))[0]
        if i >= 2:
            ts.append(t)
    return 2 * n / (statistics.median(ts) * 1e-3) / 1e9


def run_case(form, l, ks, reps, roof, emit):
    dt = torch.complex128 if form == "complex128" else torch.float64
    u = exchange_symmetric_(fill((l, l, l, l), dt, 1))
    T = fill((max(ks), l, l), dt, 2)
    nbytes = u.numel() * u.element_size()
    half = nbytes * (l + 1) / (2.0 * l)                               # l^2 rows of l (l + 1) / 2 elements
    emit(f"{form} l={l}: u = {nbytes / 1e9:.3f} GB, the half read = {half / 1e9:.3f} GB (with the diagonals)")
    for k in ks:
        Tk = T[:k]

        def full():
            return kernels.pair_contract(u, Tk)

        def exch():
            return kernels.pair_contract_exchange(u, Tk)

        for _ in range(2):
            s_full, s_exch = full(), exch()
        torch.cuda.synchronize()
        rel = float((s_exch - s_full).abs().max() / s_full.abs().max())
        passes = kernels.last_dispatch()
        groups = -(-k // 8)
        t_full, t_exch = [], []
        for _ in range(reps):
            t_exch.append(timed(exch)[0])
            t_full.append(timed(full)[0])
        m_full, m_exch = statistics.median(t_full), statistics.median(t_exch)
        emit(f"  K={k:2d}: full {stats(t_full)}  exchange {stats(t_exch)}  gain {m_full / m_exch:5.2f}x  "
             f"holds {max(t_exch) < min(t_full)}  exchange {groups * half / (m_exch * 1e-3) / 1e9:7.1f} GB/s "
             f"({groups * half / (m_exch * 1e-3) / 1e9 / roof:.2f} of copy), full {groups * nbytes / (m_full * 1e-3) / 1e9:7.1f} GB/s "
             f"({groups * nbytes / (m_full * 1e-3) / 1e9 / roof:.2f} of copy)  rel diff {rel:.1e}  [{passes}]")
    del u
    torch.cuda.empty_cache()


def run_rccd(l, n, reps, emit):
    import numpy as np

    import quantum_systems_amd as qsa
    from quantum_systems_amd import RCCD, hip

    u = fill((l, l, l, l), torch.float64, 3)
    u.mul_(0.01 / l)
    exchange_symmetric_(u)
    h = torch.diag(2.0 * torch.arange(l, dtype=torch.float64, device="cuda"))
    g = 0.05 * fill((l, l), torch.float64, 4)
    C = torch.linalg.qr(torch.eye(l, dtype=torch.float64, device="cuda") + g - g.T)[0].contiguous()
    bs = qsa.setup_basis_set(2 * n, l, hip.asarray(np.eye(l)), hip.asarray(h), hip.asarray(u), 2, -1, hip, False, False)
    system = qsa.SpatialOrbitalSystem(2 * n, bs)
    eps = (C.T @ h @ C).diagonal().contiguous()
    emit(f"RCCD l_s={l} n_s={n}: K = {n * (n + 1) // 2} amplitudes per pass, u = {u.numel() * 8 / 1e9:.3f} GB")
    for ladder in ("exchange", "full"):
        ccd = RCCD(system, hip.asarray(C), hip.asarray(eps), ladder=ladder)
        t = ccd._t
        for _ in range(2):
            ccd._ladder(t)
            ccd._residual(t)
        t_lad, t_all = [], []
        for _ in range(reps):
            t_lad.append(timed(lambda: ccd._ladder(t))[0])
            t_all.append(timed(lambda: ccd._residual(t))[0])
        m_lad, m_all = statistics.median(t_lad), statistics.median(t_all)
        emit(f"  ladder={ladder:8s}: ladder {stats(t_lad)}  residual {stats(t_all)}  rest {m_all - m_lad:9.4f} ms "
             f"({(m_all - m_lad) / m_all:.2f} of the iteration)")
        del ccd
    del u, system, bs
    torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--cases", default=DEFAULT)
    ap.add_argument("--k", default="15,66")
    ap.add_argument("--rccd", default="110:5,156:11,256:11")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("rccd_bench needs a GPU: timings are not taken on a CPU")
    fh = open(args.out, "a") if args.out else None

    def emit(line):
        print(line, flush=True)
        if fh:
            fh.write(line + "\n")
            fh.flush()

    emit(f"# rccd_bench: {torch.cuda.get_device_name(0)}, reps {args.reps}, exchange / full alternating, HIP events, "
         "median [min, max]")
    roof = copy_rate(args.reps)
    emit(f"# qs_probe_stream_copy on 2 GiB: {roof:.1f} GB/s read + write")
    ks = [int(x) for x in args.k.split(",")]
    for case in filter(None, args.cases.split(",")):
        form, l = case.split(":")
        run_case(form, int(l), ks, args.reps, roof, emit)
    for case in filter(None, args.rccd.split(",")):
        l, n = case.split(":")
        run_rccd(int(l), int(n), args.reps, emit)


if __name__ == "__main__":
    main()
