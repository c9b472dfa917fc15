#!/usr/bin/env python3
"""The MDCT handle (fourier_hip_mdct_*) against what a caller wrote before it, on the GPU.

  python tools/mdct_bench.py [--reals f32,f64] [--n 128,256,512,1024,2048,960] [--length 1048576] [--batch 64] [--reps 5] [--out FILE]
      One JSON line per precision and n (length 2^20, batch 64, center): HIP-event milliseconds per call (median / min / max over
      alternating repetitions on shared buffers) of the arms
        handle    Mdct.forward on its default route
        composed  the handle with "fusion" = 0
        fused     the handle with "fusion" = 1 (only where that route exists)
        caller    torch pad + unfold to frames of 2n + window multiply + complex pre-twiddle + Fft of 2n points + post-twiddle + .real:
                  what could be written without the handle
        inverse   Mdct.inverse, for information
      every arm's spread (max - min) / median, the ratios, the rate of every arm on the algorithmic bytes (length reals in and
      frames x n reals out per row) and the ratio the byte model predicts for fused over composed, 1 / 3."""
import argparse
import json
import math
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def time_arms(torch, arms, reps, warmup=1):
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
    return {k: {"median_ms": statistics.median(v), "min_ms": min(v), "max_ms": max(v),
                "spread": (max(v) - min(v)) / statistics.median(v)} for k, v in ms.items()}


def run_case(torch, fa, real, n, length, batch, reps):
    rdt, cdt = (torch.float32, torch.complex64) if real == "f32" else (torch.float64, torch.complex128)
    val = torch.empty(0, dtype=rdt).element_size()
    x = torch.randn(batch, length, dtype=rdt, device="cuda")
    plans = {}
    for arm, fusion in (("handle", None), ("composed", 0), ("fused", 1)):
        p = fa.Mdct(n, real, True, 0)
        if fusion is not None:
            p.set_option("fusion", fusion)
        p.reserve(length, batch)
        plans[arm] = p
    if not plans["fused"].describe().startswith("mdct fused"):
        del plans["fused"]
    nf = plans["handle"].frames(length)
    out = torch.empty(batch, nf, n, dtype=rdt, device="cuda")
    back = torch.empty(batch, length, dtype=rdt, device="cuda")
    fft = fa.Fft(2 * n, real, 0)
    fft.reserve(batch * nf, True)
    stream = torch.cuda.current_stream().cuda_stream
    m = torch.arange(2 * n, dtype=torch.float64, device="cuda")
    k = torch.arange(n, dtype=torch.float64, device="cuda")
    w = torch.sin(math.pi * (m + 0.5) / (2 * n)).to(rdt)
    pre = torch.polar(torch.ones_like(m), -math.pi * m / (2 * n)).to(cdt) * w
    post = torch.polar(torch.ones_like(k), -math.pi * (n + 1) * (2 * k + 1) / (4 * n)).to(cdt)

    def caller():
        xp = torch.nn.functional.pad(x, (n, (nf + 1) * n - n - length))
        z = (xp.unfold(-1, 2 * n, n) * pre).contiguous()
        fft.transform_batch_ptr(z.data_ptr(), z.data_ptr(), batch * nf, 0, stream)
        torch.mul(z[..., :n], post).real.contiguous()

    arms = {arm: (lambda p: (lambda: p.forward(x, out=out)))(p) for arm, p in plans.items()}
    arms["caller"] = caller
    inv = plans["handle"]
    arms["inverse"] = lambda: inv.inverse(out, length, out=back)
    t = time_arms(torch, arms, reps)
    med = {a: v["median_ms"] for a, v in t.items()}
    nbytes = batch * (length + nf * n) * val
    rec = {"real": real, "n": n, "length": length, "batch": batch, "frames": nf,
           "describe": {a: p.describe() for a, p in plans.items()}, "ms": t,
           "handle_over_caller": med["handle"] / med["caller"], "composed_over_caller": med["composed"] / med["caller"],
           "fused_over_composed": med["fused"] / med["composed"] if "fused" in med else None,
           "fused_beats_composed_by_more_than_its_spread": (med["fused"] < med["composed"] * (1 - t["composed"]["spread"])) if "fused" in med else None,
           "byte_model_fused_over_composed": 1 / 3,
           "algorithmic_bytes": nbytes, "tbs_on_algorithmic_bytes": {a: nbytes / (v * 1e-3) / 1e12 for a, v in med.items()}}
    del x, out, back, plans, arms, fft
    torch.cuda.empty_cache()
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reals", default="f32,f64")
    ap.add_argument("--n", default="128,256,512,1024,2048,960")
    ap.add_argument("--length", type=int, default=1 << 20)
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch

    if not torch.cuda.is_available():
        raise SystemExit("needs a GPU")
    import fourier_amd

    recs = []
    for real in [r for r in args.reals.split(",") if r]:
        for n in [int(v) for v in args.n.split(",") if v]:
            r = run_case(torch, fourier_amd, real, n, args.length, args.batch, args.reps)
            recs.append(r)
            print(json.dumps(r), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as f:
            for r in recs:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
