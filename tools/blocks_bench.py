"""Time ``kernels.transform_two_body_blocks`` (the <ij|ab> block) against the full transform sliced, and its first step
against the streaming roof.

    python tools/blocks_bench.py [--out FILE] [--reps N] [--cases fp64:256:6,fp64:128:16,...]

Per case (dtype form : l : o occupied), in ONE process on one device, HIP events around each call, medians with ranges:
  copy   qs_probe_stream_copy of as many bytes as u holds (moves twice that): the roof of a streaming kernel
  new    kernels.transform_two_body_blocks(u, Ct[:o], Ct[:o], C[:, o:], C[:, o:])        <ij|ab>, one read of u
  old    kernels.transform_two_body(u, C)[:o, :o, o:, o:]                               the only route before
         (warm-ups, then new / old alternating ``reps`` times)
  lead   kernels.lead_contract(Ct[:o], u as (l, l^3)): step a alone; moved = e_u l^4 + e o l^3 bytes
  gemm   the same product through the general dispatch (kernels.matmul; same-dtype forms only), alternating with lead
``fraction of roof`` = (moved / lead) / (2 x bytes of u / copy)."""

import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from quantum_systems_amd import _lib, kernels  # noqa: E402

DEFAULT = "fp64:256:6,fp64:128:6,fp64:128:16,fp64:128:32,fp64:91:6,complex128:128:6,mixed:128:6"


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
    return f"{statistics.median(xs):10.4f} ms  [{min(xs):.4f}, {max(xs):.4f}]"


def run_case(form, l, o, reps, emit):
    cplx = torch.complex128
    cdt = torch.float64 if form == "fp64" else cplx
    u = fill((l, l, l, l), cplx if form == "complex128" else torch.float64, 1)
    C = fill((l, l), cdt, 2)
    Ct = kernels.default_bra(C)
    bo, kv = Ct[:o].contiguous(), C[:, o:].contiguous()
    nbytes = u.numel() * u.element_size()
    ncopy = nbytes // 16 * 16                # (the probe moves whole 16-byte items: an odd l leaves 8 bytes out)
    lib = _lib.load()

    dst = torch.empty(ncopy, dtype=torch.uint8, device="cuda")

    def copy():
        _lib.check(lib.qs_probe_stream_copy(u.data_ptr(), dst.data_ptr(), ncopy, kernels._stream()), "stream copy")

    t_copy = [timed(copy)[0] for _ in range(2 + reps)][2:]
    del dst
    torch.cuda.empty_cache()

    def new():
        return kernels.transform_two_body_blocks(u, bo, bo, kv, kv)

    def old():
        return kernels.transform_two_body(u, C)[:o, :o, o:, o:]

    for _ in range(2):
        w_new, w_old = new(), old()
    ran = lib.qs_last_dispatch().decode()
    w_new = new()
    ran_new = lib.qs_last_dispatch().decode()
    rel = float((w_new - w_old).abs().max() / w_old.abs().max())
    del w_old
    t_new, t_old = [], []
    for _ in range(reps):
        t_new.append(timed(new)[0])
        t_old.append(timed(old)[0])
    torch.cuda.empty_cache()
    work = lib.qs_transform_two_body_blocks_workspace(0 if u.dtype == torch.float64 else 1, 0 if form == "fp64" else 1,
                                                      l, o, o, l - o, l - o)
    old_work = lib.qs_transform_two_body_workspace(0 if form == "fp64" else 1, l, l)
    es = 8 if form == "fp64" else 16

    B = u.view(l, l**3)
    T = torch.empty((o, l**3), dtype=cdt, device="cuda")
    t_lead, t_gemm = [], []
    for i in range(2 + reps):
        a = timed(lambda: kernels.lead_contract(bo, B, out=T))[0]
        g = timed(lambda: kernels.matmul(bo, B, out=T))[0] if form != "mixed" else None
        if i >= 2:
            t_lead.append(a)
            if g is not None:
                t_gemm.append(g)
    ran_gemm = lib.qs_last_dispatch().decode() if form != "mixed" else "-"
    moved = nbytes + es * o * l**3
    m_new, m_old, m_copy, m_lead = (statistics.median(x) for x in (t_new, t_old, t_copy, t_lead))
    emit(f"{form} l={l} o={o}: u = {nbytes / 1e9:.3f} GB, max rel difference new/old {rel:.2e}")
    emit(f"  new kernels: {ran_new}")
    emit(f"  old kernels: {ran}")
    emit(f"  new  {stats(t_new)}   workspace {work / 1e9:.3f} GB + block {es * o * o * (l - o)**2 / 1e9:.4f} GB")
    emit(f"  old  {stats(t_old)}   speed-up {m_old / m_new:6.2f}x   (slowest new {max(t_new):.4f} vs fastest old {min(t_old):.4f})"
         f"   workspace {old_work / 1e9:.3f} GB + result {es * l**4 / 1e9:.3f} GB")
    emit(f"  copy {stats(t_copy)}   {2 * nbytes / m_copy / 1e9:8.3f} TB/s read + write")
    emit(f"  lead {stats(t_lead)}   {moved / m_lead / 1e9:8.3f} TB/s moved   fraction of roof {(moved / m_lead) / (2 * nbytes / m_copy):.3f}")
    if t_gemm:
        emit(f"  gemm {stats(t_gemm)}   lead / gemm {m_lead / statistics.median(t_gemm):.3f}   [{ran_gemm}]")
    del u, B, T
    torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--cases", default=DEFAULT)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("blocks_bench needs a GPU: timings are not taken on a CPU")
    fh = open(args.out, "a") if args.out else None

    def emit(line):
        print(line, flush=True)
        if fh:
            fh.write(line + "\n")
            fh.flush()

    emit(f"# blocks_bench: {torch.cuda.get_device_name(0)}, reps {args.reps}, new / old alternating (copy before them), HIP events, median [min, max]")
    for case in args.cases.split(","):
        form, l, o = case.split(":")
        run_case(form, int(l), int(o), args.reps, emit)


if __name__ == "__main__":
    main()
