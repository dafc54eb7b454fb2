"""Time ``kernels.pair_contract_antisym`` against ``kernels.pair_contract`` on the same tensor, and one CCD iteration
split into its pass over ``u`` and the rest.

    python tools/ccd_bench.py [--out FILE] [--reps N] [--cases fp64:110,fp64:156,...] [--k 15,66] [--ccd 110:6,156:12]

  antisym  ONE call of kernels.pair_contract_antisym(u, T): reads p < q, r < s of u, a quarter of its bytes
  full     ONE call of kernels.pair_contract(u, T): reads all of u

``u`` is random and anti-symmetric in its trailing pair, ``T`` anti-symmetric, so the two routes compute the same rows
p < q ("rel diff" is taken on those).  One process; after two warm-ups the two routes alternate ``reps`` times, HIP
events around each, median [min, max].  "of copy" is the bytes the route has to read (a quarter of u / all of u) per
group pass over its median time, against the rate of ``qs_probe_stream_copy`` (read + write counted) measured in the
same run; a quarter of u is larger than the 256 MB Infinity Cache from l = 107 (fp64) up.  The CCD part builds ``coupled_cluster.CCD`` on a random
system of l spin orbitals and n particles in non-canonical orbitals and times ``_ladder`` (back-transform, pass,
two forward transforms) and the whole residual under both ladder routes.  Needs a GPU."""

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
    u = fill((l, l, l, l), dt, 1)
    kernels.antisymmetrize(u, out=u)                                   # u[pqrs] - u[pqsr], in place
    T = fill((max(ks), l, l), dt, 2)
    T = (T - T.transpose(1, 2)).contiguous()
    nbytes = u.numel() * u.element_size()
    r, s = torch.triu_indices(l, l, offset=1, device="cuda")
    emit(f"{form} l={l}: u = {nbytes / 1e9:.3f} GB, the quarter read = {nbytes / 4e9:.3f} GB (less the diagonals)")
    for k in ks:
        Tk = T[:k]

        def full():
            return kernels.pair_contract(u, Tk)

        def anti():
            return kernels.pair_contract_antisym(u, Tk)

        for _ in range(2):
            s_full, s_anti = full(), anti()
        torch.cuda.synchronize()
        rel = float((s_anti[:, r, s] - s_full[:, r, s]).abs().max() / s_full[:, r, s].abs().max())
        passes = kernels.last_dispatch()
        groups = -(-k // 8)
        t_full, t_anti = [], []
        for _ in range(reps):
            t_anti.append(timed(anti)[0])
            t_full.append(timed(full)[0])
        m_full, m_anti = statistics.median(t_full), statistics.median(t_anti)
        quarter = nbytes * (l - 1) ** 2 / (4.0 * l * l)              # l (l - 1) / 2 rows of l (l - 1) / 2 elements
        emit(f"  K={k:2d}: full {stats(t_full)}  antisym {stats(t_anti)}  gain {m_full / m_anti:5.2f}x  "
             f"holds {max(t_anti) < min(t_full)}  antisym {groups * quarter / (m_anti * 1e-3) / 1e9:7.1f} GB/s "
             f"({groups * quarter / (m_anti * 1e-3) / 1e9 / roof:.2f} of copy), full {groups * nbytes / (m_full * 1e-3) / 1e9:7.1f} GB/s "
             f"({groups * nbytes / (m_full * 1e-3) / 1e9 / roof:.2f} of copy)  rel diff {rel:.1e}  [{passes}]")
    del u
    torch.cuda.empty_cache()


def run_ccd(l, n, reps, emit):
    import numpy as np

    import quantum_systems_amd as qsa
    from quantum_systems_amd import CCD, hip

    u = fill((l, l, l, l), torch.float64, 3)
    u.mul_(0.01 / l)
    kernels.antisymmetrize(u, out=u)
    h = torch.diag(2.0 * torch.arange(l, dtype=torch.float64, device="cuda"))
    g = 0.05 * fill((l, l), torch.float64, 4)
    C = torch.linalg.qr(torch.eye(l, dtype=torch.float64, device="cuda") + g - g.T)[0].contiguous()
    bs = qsa.setup_basis_set(n, l, hip.asarray(np.eye(l)), hip.asarray(h), hip.asarray(u), 2, -1, hip, True, True)
    system = qsa.GeneralOrbitalSystem(n, bs, anti_symmetrize=False)
    eps = (C.T @ h @ C).diagonal().contiguous()
    emit(f"CCD l={l} n={n}: K = {n * (n - 1) // 2} amplitudes per pass, u = {u.numel() * 8 / 1e9:.3f} GB")
    for ladder in ("antisym", "full"):
        ccd = CCD(system, hip.asarray(C), hip.asarray(eps), ladder=ladder)
        t = ccd._t
        for _ in range(2):
            ccd._ladder(t)
            ccd._residual(t)
        t_lad, t_all = [], []
        for _ in range(reps):
            t_lad.append(timed(lambda: ccd._ladder(t))[0])
            t_all.append(timed(lambda: ccd._residual(t))[0])
        m_lad, m_all = statistics.median(t_lad), statistics.median(t_all)
        emit(f"  ladder={ladder:7s}: ladder {stats(t_lad)}  residual {stats(t_all)}  rest {m_all - m_lad:9.4f} ms "
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
    ap.add_argument("--ccd", default="110:6,156:12")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("ccd_bench needs a GPU: timings are not taken on a CPU")
    fh = open(args.out, "a") if args.out else None

    def emit(line):
        print(line, flush=True)
        if fh:
            fh.write(line + "\n")
            fh.flush()

    emit(f"# ccd_bench: {torch.cuda.get_device_name(0)}, reps {args.reps}, antisym / full alternating, HIP events, "
         "median [min, max]")
    roof = copy_rate(args.reps)
    emit(f"# qs_probe_stream_copy on 2 GiB: {roof:.1f} GB/s read + write")
    ks = [int(x) for x in args.k.split(",")]
    for case in filter(None, args.cases.split(",")):
        form, l = case.split(":")
        run_case(form, int(l), ks, args.reps, roof, emit)
    for case in filter(None, args.ccd.split(",")):
        l, n = case.split(":")
        run_ccd(int(l), int(n), args.reps, emit)


if __name__ == "__main__":
    main()
