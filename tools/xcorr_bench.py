#!/usr/bin/env python3
"""The cross-correlation handle (fourier_hip_xcorr_*) against its own composed route and what a caller wrote before it, on the GPU.

  python tools/xcorr_bench.py [--shapes f32:2048,f32:8192,f32:32768,f64:2048,f64:8192,f64:16384] [--mib 512] [--reps 5]
                              [--experiments] [--out FILE]
      One JSON line per shape (precision : L) and weighting (none, phat): real rows of n = L / 2 samples, the full linear window
      (lag_first = -(n - 1), lags = 2n - 1); the batch is chosen so that the two inputs are about --mib MiB.  HIP-event milliseconds
      per call (median / min / max over alternating repetitions on shared buffers, one process) of the arms
        one_launch  CrossCorrelation.correlate, "fusion" = 1 (absent where the library has no one-launch kernel for the shape and
                    weighting: the product holds only those without scratch memory; --experiments binds the experiments library under
                    FOURIER_XCORR_SPILLING=1, which admits every instance -- a measurement of kernels the product does not run)
        composed    the same with "fusion" = 0
        caller      RealFft.rfft of the two rows padded to L, torch conj * (and / abs of each spectrum for PHAT), RealFft.irfft, a slice
                    and a roll into the window
      every arm's spread (max - min) / median, every handle arm over the caller arm, the one-launch arm over the composed one and
      whether it beats it by more than the larger of the two arms' widths (the rule a default follows), and the byte model (DESIGN.md
      section 4): about 8 L one-launch, about 60 L composed, more for the caller, in bytes per pair of f32 rows."""
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


def run_case(torch, fa, real, L, phat, mib, reps):
    rdt = torch.float32 if real == "f32" else torch.float64
    rs = 4 if real == "f32" else 8
    n = L // 2
    first, lags = -(n - 1), 2 * n - 1
    batch = max(1, int(mib * (1 << 20)) // (2 * n * rs))
    x = torch.randn(batch, n, dtype=rdt, device="cuda")
    y = torch.randn(batch, n, dtype=rdt, device="cuda")
    out = torch.empty(batch, lags, dtype=rdt, device="cuda")
    plans = {}
    for arm, fusion in (("one_launch", 1), ("composed", 0)):
        p = fa.CrossCorrelation(n, L, first, lags, real, True, 0)
        p.set_option("weighting", int(phat))
        p.set_option("fusion", fusion)
        p.reserve(batch)
        plans[arm] = p
    default = fa.CrossCorrelation(n, L, first, lags, real, True, 0).describe()
    if not plans["one_launch"].describe().startswith("xcorr one-launch"):
        del plans["one_launch"]
    rfft = fa.RealFft(L, real, 0)
    rfft.reserve(batch)
    px = torch.zeros(batch, L, dtype=rdt, device="cuda")
    py = torch.zeros(batch, L, dtype=rdt, device="cuda")

    def caller():
        px[:, :n].copy_(x)
        py[:, :n].copy_(y)
        X, Y = rfft.rfft(px), rfft.rfft(py)
        if phat:
            X = X / X.abs()
            Y = Y / Y.abs()
        r = rfft.irfft(X.conj() * Y)
        out[:, :n - 1].copy_(r[:, L - (n - 1):])
        out[:, n - 1:].copy_(r[:, :n])

    arms = {arm: (lambda p: (lambda: p.correlate(x, y, out=out)))(p) for arm, p in plans.items()}
    arms["caller"] = caller
    t = time_arms(torch, arms, reps)
    med = {a: v["median_ms"] for a, v in t.items()}
    width = lambda a: t[a]["max_ms"] - t[a]["min_ms"]  # noqa: E731
    fused = None
    if "one_launch" in plans:
        fused = {"over_composed": med["one_launch"] / med["composed"],
                 "beats_composed_by_more_than_the_spread": med["composed"] - med["one_launch"] > max(width("one_launch"), width("composed"))}
    rec = {"real": real, "L": L, "n": n, "lags": lags, "weighting": "phat" if phat else "none", "batch": batch,
           "input_bytes": 2 * batch * n * rs, "default": default, "describe": {a: p.describe() for a, p in plans.items()},
           "rfft": rfft.describe(), "ms": t, "over_caller": {a: med[a] / med["caller"] for a in plans}, "one_launch": fused,
           "byte_model_bytes_per_pair_of_f32_rows_over_L": {"one_launch": 8, "composed": 60}}
    del x, y, out, px, py, plans, arms, rfft
    torch.cuda.empty_cache()
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="f32:2048,f32:8192,f32:32768,f64:2048,f64:8192,f64:16384")
    ap.add_argument("--mib", type=float, default=512.0)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--experiments", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch

    if not torch.cuda.is_available():
        raise SystemExit("needs a GPU")
    import fourier_amd

    library = "product"
    if args.experiments:
        import ctypes

        from fourier_amd import _lib, build

        os.environ["FOURIER_XCORR_SPILLING"] = "1"
        _lib._lib = _lib.bind(ctypes.CDLL(build.OUT_EXPERIMENTS))
        library = "experiments, FOURIER_XCORR_SPILLING=1"
    recs = []
    for shape in [s for s in args.shapes.split(",") if s]:
        real, L = shape.split(":")
        for phat in (False, True):
            r = run_case(torch, fourier_amd, real, int(L), phat, args.mib, args.reps)
            r["library"] = library
            recs.append(r)
            print(json.dumps(r), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as f:
            for r in recs:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
