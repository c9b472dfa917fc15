#!/usr/bin/env python3
"""The cepstrum handle (fourier_hip_cepstrum_*) against its own composed route and what a caller wrote before it, on the GPU.

  python tools/cepstrum_bench.py [--shapes f32:2048,f32:8192,f32:32768,f64:2048,f64:8192,f64:16384] [--mib 512] [--reps 5] [--out FILE]
      One JSON line per shape (precision : L) and mode (cepstrum, minimum_phase): real rows of n = L / 2 samples (x[0] = 1 plus small
      noise, so that no bin is near 0), m = n outputs; the batch is chosen so that the input is about --mib MiB.  HIP-event
      milliseconds per call (median / min / max over alternating repetitions on shared buffers, one process) of the arms
        one_launch  Cepstrum.apply, "fusion" = 1 (absent where the library has no one-launch kernel for the length and the mode)
        composed    the same with "fusion" = 0
        caller      RealFft.rfft of the rows padded to L, torch abs / log, RealFft.irfft, a slice; for the minimum-phase row the fold
                    (a multiply by the weight row), RealFft.rfft, torch.exp of the complex tensor, RealFft.irfft, a slice
      every arm's spread (max - min) / median, every handle arm over the caller arm, the one-launch arm over the composed one and
      whether it beats it by more than the larger of the two arms' widths (the rule a default follows), and the byte model (DESIGN.md
      section 4): about 4 L one-launch; about 56 L composed for the cepstrum and about twice that for the minimum-phase row, in bytes
      per f32 row."""
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


def run_case(torch, fa, real, L, mode, mib, reps):
    rdt = torch.float32 if real == "f32" else torch.float64
    rs = 4 if real == "f32" else 8
    n = L // 2
    batch = max(1, int(mib * (1 << 20)) // (n * rs))
    x = 0.2 * torch.randn(batch, n, dtype=rdt, device="cuda") / n ** 0.5
    x[:, 0] += 1.0
    out = torch.empty(batch, n, dtype=rdt, device="cuda")
    plans = {}
    for arm, fusion in (("one_launch", 1), ("composed", 0)):
        p = fa.Cepstrum(n, L, real, n, mode, 0)
        p.set_option("fusion", fusion)
        p.reserve(batch)
        plans[arm] = p
    default = fa.Cepstrum(n, L, real, n, mode, 0).describe()
    if not plans["one_launch"].describe().startswith("cepstrum one-launch"):
        del plans["one_launch"]
    rfft = fa.RealFft(L, real, 0)
    rfft.reserve(batch)
    px = torch.zeros(batch, L, dtype=rdt, device="cuda")
    w = torch.zeros(L, dtype=rdt, device="cuda")
    w[0], w[1:L // 2], w[L // 2] = 1.0, 2.0, 1.0

    def caller():
        px[:, :n].copy_(x)
        c = rfft.irfft(torch.log(torch.abs(rfft.rfft(px))).to(torch.complex64 if real == "f32" else torch.complex128))
        if mode == 0:
            out.copy_(c[:, :n])
            return
        out.copy_(rfft.irfft(torch.exp(rfft.rfft(c * w)))[:, :n])

    arms = {arm: (lambda p: (lambda: p.apply(x, out=out)))(p) for arm, p in plans.items()}
    arms["caller"] = caller
    t = time_arms(torch, arms, reps)
    med = {a: v["median_ms"] for a, v in t.items()}
    width = lambda a: t[a]["max_ms"] - t[a]["min_ms"]  # noqa: E731
    fused = None
    if "one_launch" in plans:
        fused = {"over_composed": med["one_launch"] / med["composed"],
                 "beats_composed_by_more_than_the_spread": med["composed"] - med["one_launch"] > max(width("one_launch"), width("composed"))}
    rec = {"real": real, "L": L, "n": n, "mode": ("cepstrum", "minimum_phase")[mode], "batch": batch, "input_bytes": batch * n * rs,
           "default": default, "describe": {a: p.describe() for a, p in plans.items()}, "rfft": rfft.describe(), "ms": t,
           "over_caller": {a: med[a] / med["caller"] for a in plans}, "one_launch": fused,
           "byte_model_bytes_per_f32_row_over_L": {"one_launch": 4, "composed": 56 if mode == 0 else 112}}
    del x, out, px, plans, arms, rfft
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
        for mode in (0, 1):
            r = run_case(torch, fourier_amd, real, int(L), mode, args.mib, args.reps)
            recs.append(r)
            print(json.dumps(r), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as f:
            for r in recs:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
