#!/usr/bin/env python3
"""The resampling handle (fourier_hip_resample_*) against its own composed route and what a caller wrote before it, on the GPU.

  python tools/resample_bench.py [--shapes 64:1048576:524288,64:1048576:2097152,1024:48000:44100,1024:44100:48000]
                                 [--reals f32,f64] [--reps 5] [--out FILE]
      One JSON line per shape (rows : N : M), precision and kind of row (real, complex).  HIP-event milliseconds per call (median / min /
      max over alternating repetitions on shared buffers, one process) of the arms
        fused     Resample.forward, "fusion" = 1 (real rows with N and M both even only)
        composed  the same with "fusion" = 0 (complex rows: the one route there is)
        caller    RealFft(N).rfft, torch slice or pad of the half spectrum with the Nyquist factor and M / N, RealFft(M).irfft
                  (complex rows: Fft(N), torch slices into a zeroed spectrum of M bins, Fft(M) inverse)
      every arm's spread (max - min) / median, every handle arm over the caller arm, the fused arm over the composed one and whether it
      beats it by more than the larger of the two arms' spreads (the rule the default of "fusion" follows), and the byte model
      (DESIGN.md section 4): 24N fused, 40N composed, about 56N caller, in bytes per f32 row at N = M."""
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


def run_case(torch, fa, real, rows, n, m, complex_rows, reps):
    from fourier_amd import Transform

    rdt, cdt = (torch.float32, torch.complex64) if real == "f32" else (torch.float64, torch.complex128)
    dt = cdt if complex_rows else rdt
    x = torch.randn(rows, n, dtype=dt, device="cuda")
    out = torch.empty(rows, m, dtype=dt, device="cuda")
    plans = {}
    for arm, fusion in (("fused", 1), ("composed", 0)):
        p = fa.Resample(n, m, real, 0, real_input=not complex_rows)
        p.set_option("fusion", fusion)
        p.reserve(rows)
        plans[arm] = p
    default = fa.Resample(n, m, real, 0, real_input=not complex_rows).describe()
    if plans["fused"].describe() == plans["composed"].describe():
        del plans["fused"]
    k, scale = min(n, m), m / n
    if complex_rows:
        fin, fout = fa.Fft(n, real, 0), fa.Fft(m, real, 0)
        fin.reserve(rows)
        fout.reserve(rows, True)
        X = torch.empty(rows, n, dtype=cdt, device="cuda")
        Y = torch.empty(rows, m, dtype=cdt, device="cuda")
        lo, hi = (k + 1) // 2, (k - 1) // 2  # bins 0 ... lo - 1 and the last hi

        def caller():
            fin.transform(x, X, Transform.Fft)
            Y.zero_()
            Y[:, :lo] = X[:, :lo]
            if hi:
                Y[:, m - hi:] = X[:, n - hi:]
            if k % 2 == 0:
                h = k // 2
                if m < n:
                    Y[:, h] = X[:, h] + X[:, n - h]
                elif n < m:
                    Y[:, h] = X[:, h] * 0.5
                    Y[:, m - h] = Y[:, h]
                else:
                    Y[:, h] = X[:, h]
            Y.mul_(scale)
            fout.transform(Y, out, Transform.Ifft)
    else:
        fin, fout = fa.RealFft(n, real, 0), fa.RealFft(m, real, 0)
        fin.reserve(rows)
        fout.reserve(rows)
        Y = torch.empty(rows, m // 2 + 1, dtype=cdt, device="cuda")
        keep = min(n // 2 + 1, m // 2 + 1)

        def caller():
            X = fin.rfft(x)
            if m > n:
                Y.zero_()
            Y[:, :keep] = X[:, :keep]
            if k % 2 == 0 and m != n:
                Y[:, k // 2] *= 2.0 if m < n else 0.5
            Y.mul_(scale)
            out.copy_(fout.irfft(Y))

    arms = {arm: (lambda p: (lambda: p.forward(x, out=out)))(p) for arm, p in plans.items()}
    arms["caller"] = caller
    # the arms agree before they are timed
    results = {}
    for a, f in arms.items():
        f()
        results[a] = out.clone()
    agree = {a: float((results[a] - results["composed"]).norm() / results["composed"].norm()) for a in arms}
    t = time_arms(torch, arms, reps)
    med = {a: v["median_ms"] for a, v in t.items()}
    width = lambda a: t[a]["max_ms"] - t[a]["min_ms"]  # noqa: E731
    fused = None
    if "fused" in plans:
        fused = {"over_composed": med["fused"] / med["composed"],
                 "beats_composed_by_more_than_the_spread": med["composed"] - med["fused"] > max(width("fused"), width("composed"))}
    rec = {"real": real, "rows": rows, "n": n, "m": m, "kind": "complex" if complex_rows else "real", "default": default,
           "describe": {a: p.describe() for a, p in plans.items()}, "ms": t, "over_caller": {a: med[a] / med["caller"] for a in plans},
           "fused": fused, "relative_l2_against_composed": agree,
           "byte_model_bytes_per_f32_row_over_n_at_n_equal_m": {"fused": 24, "composed": 40, "caller": 56}}
    del x, out, plans, arms, fin, fout, results
    torch.cuda.empty_cache()
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="64:1048576:524288,64:1048576:2097152,1024:48000:44100,1024:44100:48000")
    ap.add_argument("--reals", default="f32,f64")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch

    if not torch.cuda.is_available():
        raise SystemExit("needs a GPU")
    import fourier_amd

    for shape in [s for s in args.shapes.split(",") if s]:
        rows, n, m = (int(v) for v in shape.split(":"))
        for real in args.reals.split(","):
            for complex_rows in (False, True):
                r = run_case(torch, fourier_amd, real, rows, n, m, complex_rows, args.reps)
                print(json.dumps(r), flush=True)
                if args.out:
                    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
                    with open(args.out, "a") as f:
                        f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
