#!/usr/bin/env python3
"""Real-input N-D transforms (fourier_hip_realnd_*, fourier_amd.rfftn / irfftn) against what a user could run without them, on the GPU.

  python tools/rfftn_bench.py [--cases f32_2048,f64_2048,f32_256,f32_1000] [--reps 10] [--out FILE]
      One JSON line per case, HIP-event milliseconds per call (median over alternating repetitions on shared buffers), three arms on
      the same input:
        rfftn   fourier_amd.rfftn / irfftn (the packed route for even W);
        chain   RealFft.rfft along the last axis, then fftn over the other transformed axes in place (the inverse: fftn's inverse
                out of place, then RealFft's inverse) -- the existing public API;
        complex fftn of a complex tensor of the same shape (the forward only).
      Cases: f32_2048 / f64_2048: [64, 2048, 2048], rfft2 over the last two axes; f32_256: a [256, 256, 256] volume, rfftn over all
      three; f32_1000: [64, 1000, 1000], rfft2.  A `rocprofv3 --kernel-trace --stats` run of the same case gives the kernels' own
      times (the N-D sweeps: realnd_post_kernel / realnd_pre_kernel)."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CASES = {"f32_2048": ("f32", (64, 2048, 2048), 2), "f64_2048": ("f64", (64, 2048, 2048), 2),
         "f32_256": ("f32", (256, 256, 256), 3), "f32_1000": ("f32", (64, 1000, 1000), 2)}


def time_arms(torch, arms, reps, warmup=1):
    """arms: {name: callable}; alternating order, HIP events on the current stream; median ms per arm."""
    for _ in range(warmup):
        for f in arms.values():
            f()
    torch.cuda.synchronize()
    ms = {k: [] for k in arms}
    for _ in range(reps):
        for k, f in arms.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            f()
            b.record()
            b.synchronize()
            ms[k].append(a.elapsed_time(b))
    return {k: {"median_ms": statistics.median(v), "min_ms": min(v), "max_ms": max(v)} for k, v in ms.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default=",".join(CASES))
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch

    import fourier_amd as fa

    lines = []
    stream = lambda: torch.cuda.current_stream().cuda_stream  # noqa: E731
    for case in args.cases.split(","):
        real, shape, rank = CASES[case]
        rdt, cdt = (torch.float32, torch.complex64) if real == "f32" else (torch.float64, torch.complex128)
        dims = tuple(range(len(shape) - rank, len(shape)))
        lead = dims[:-1]
        half = shape[:-1] + (shape[-1] // 2 + 1,)
        x = torch.randn(shape, dtype=rdt, device="cuda")
        X = torch.empty(half, dtype=cdt, device="cuda")
        T = torch.empty(half, dtype=cdt, device="cuda")
        y = torch.empty(shape, dtype=rdt, device="cuda")
        rp = fa.RealFft(shape[-1], real, 0)
        rp.reserve(x.numel() // shape[-1])
        fa.rfftn(x, dims, out=X)
        fa.irfftn(X, dims, shape[-1], out=y)
        t = time_arms(torch, {
            "rfftn": lambda: fa.rfftn(x, dims, out=X),
            "irfftn": lambda: fa.irfftn(X, dims, shape[-1], out=y),
            "chain_fwd": lambda: (rp.forward_batch_ptr(x.data_ptr(), T.data_ptr(), x.numel() // shape[-1], fa.Transform.Fft, stream()),
                                  fa.fftn(T, lead, fa.Transform.Fft, out=T)),
            "chain_inv": lambda: (fa.fftn(X, lead, fa.Transform.Ifft, out=T),
                                  rp.inverse_batch_ptr(T.data_ptr(), y.data_ptr(), x.numel() // shape[-1], fa.Transform.Ifft, stream()))},
            args.reps)
        del T
        xc = torch.randn(shape, dtype=cdt, device="cuda")
        yc = torch.empty_like(xc)
        t.update(time_arms(torch, {"complex": lambda: fa.fftn(xc, dims, fa.Transform.Fft, out=yc)}, args.reps))
        del xc, yc
        m = {k: v["median_ms"] for k, v in t.items()}
        e = X.element_size()
        rows = x.numel() // shape[-1]
        sweep_bytes = rows * (shape[-1] // 2 + (shape[-1] // 2 + 1)) * e  # read h, write h + 1 complex per row
        rec = {"case": case, "shape": list(shape), "dims": list(dims), "real": real,
               "plan": fa.RealFftN(shape[len(shape) - rank:], real, 0).describe(),
               **{k + "_ms": v for k, v in m.items()},
               "ratio_rfftn_over_complex": m["rfftn"] / m["complex"], "ratio_irfftn_over_complex": m["irfftn"] / m["complex"],
               "ratio_rfftn_over_chain": m["rfftn"] / m["chain_fwd"], "ratio_irfftn_over_chain": m["irfftn"] / m["chain_inv"],
               "sweep_bytes": sweep_bytes}
        del x, X, y
        torch.cuda.empty_cache()
        line = json.dumps(rec)
        print(line, flush=True)
        lines.append(line)
    if args.out:
        with open(args.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
