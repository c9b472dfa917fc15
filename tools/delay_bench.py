#!/usr/bin/env python3
"""The delay handle (fourier_hip_delay_*) against its own composed route and what a caller wrote before it, on the GPU.

  python tools/delay_bench.py [--shapes f32:2048,f32:8192,f32:32768,f64:2048,f64:8192,f64:16384] [--mib 512] [--reps 5] [--out FILE]
      One JSON line per shape (precision : L) and channel count (1, 8): real rows of n = L / 2 samples, one delay per row, uniform in
      (-n/2, n/2) (the linear delay: L >= n + |d|); the batch is chosen so that the input is about --mib MiB.  HIP-event milliseconds
      per call (median / min / max over alternating repetitions on shared buffers, one process) of the arms
        one_launch  Delay.apply, "fusion" = 1 (C = 1 only; absent where the library has no one-launch kernel for the length)
        composed    the same with "fusion" = 0
        caller      RealFft.rfft of the rows padded to L, a torch phase ramp exp(-2 pi i k d / L) (the turns reduced in f64, which
                    is what a careful caller needs above k d = 2^24) and a multiply, (C = 8) a torch sum over the channels BEFORE the
                    inverse, RealFft.irfft, a slice
      every arm's spread (max - min) / median, every handle arm over the caller arm, the one-launch arm over the composed one and
      whether it beats it by more than the larger of the two arms' widths (the rule a default follows), and the byte model (DESIGN.md
      section 4): about 4 L one-launch, about 52 L composed, about 56 L plus the phase tensor for the caller, in bytes per f32 row at C = 1."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def time_arms(torch, arms, reps, warmup=2):
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


def run_case(torch, fa, real, L, channels, mib, reps):
    rdt = torch.float32 if real == "f32" else torch.float64
    rs = 4 if real == "f32" else 8
    n = L // 2
    batch = max(channels, int(mib * (1 << 20)) // (n * rs) // channels * channels)
    x = torch.randn(batch, n, dtype=rdt, device="cuda")
    d = (torch.rand(batch, dtype=rdt, device="cuda") - 0.5) * n
    out = torch.empty(batch // channels, n, dtype=rdt, device="cuda")
    plans = {}
    for arm, fusion in (("one_launch", 1), ("composed", 0)):
        p = fa.Delay(n, L, real, True, channels, 0)
        p.set_option("fusion", fusion)
        p.reserve(batch)
        plans[arm] = p
    default = fa.Delay(n, L, real, True, channels, 0).describe()
    if not plans["one_launch"].describe().startswith("delay one-launch"):
        del plans["one_launch"]
    rfft = fa.RealFft(L, real, 0)
    rfft.reserve(batch)
    px = torch.zeros(batch, L, dtype=rdt, device="cuda")
    k = torch.arange(L // 2 + 1, dtype=torch.float64, device="cuda")

    def caller():
        px[:, :n].copy_(x)
        X = rfft.rfft(px)
        turns = torch.remainder(k[None, :] * d[:, None].to(torch.float64) / L, 1.0)
        X = X * torch.polar(torch.ones_like(turns), -2 * torch.pi * turns).to(X.dtype)
        if channels > 1:
            X = X.view(batch // channels, channels, -1).sum(dim=1)
        out.copy_(rfft.irfft(X)[:, :n])

    arms = {arm: (lambda p: (lambda: p.apply(x, d, out=out)))(p) for arm, p in plans.items()}
    arms["caller"] = caller
    t = time_arms(torch, arms, reps)
    med = {a: v["median_ms"] for a, v in t.items()}
    width = lambda a: t[a]["max_ms"] - t[a]["min_ms"]  # noqa: E731
    fused = None
    if "one_launch" in plans:
        fused = {"over_composed": med["one_launch"] / med["composed"],
                 "beats_composed_by_more_than_the_spread": med["composed"] - med["one_launch"] > max(width("one_launch"), width("composed"))}
    rec = {"real": real, "L": L, "n": n, "channels": channels, "batch": batch, "input_bytes": batch * n * rs, "default": default,
           "describe": {a: p.describe() for a, p in plans.items()}, "rfft": rfft.describe(), "ms": t,
           "over_caller": {a: med[a] / med["caller"] for a in plans}, "one_launch": fused,
           "byte_model_bytes_per_f32_row_over_L_at_one_channel": {"one_launch": 4, "composed": 52, "caller": 56}}
    del x, d, out, px, plans, arms, rfft
    torch.cuda.empty_cache()
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="f32:2048,f32:8192,f32:32768,f64:2048,f64:8192,f64:16384")
    ap.add_argument("--mib", type=float, default=512.0)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch

    if not torch.cuda.is_available():
        raise SystemExit("needs a GPU")
    import fourier_amd

    recs = []
    for shape in [s for s in args.shapes.split(",") if s]:
        real, L = shape.split(":")
        for channels in (1, 8):
            r = run_case(torch, fourier_amd, real, int(L), channels, args.mib, args.reps)
            recs.append(r)
            print(json.dumps(r), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as f:
            for r in recs:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
