#!/usr/bin/env python3
"""The analytic-signal handle (fourier_hip_hilbert_*) against its own composed route and what a caller wrote before it, on the GPU.

  python tools/hilbert_bench.py [--shapes f32:2048,f32:8192,f32:32768,f64:2048,f64:16384] [--gib 1.0] [--reps 7] [--out FILE]
      One JSON line per shape (precision : N) and output (analytic, envelope); the batch is chosen so that input plus output is
      about --gib GiB.  HIP-event milliseconds per call (median / min / max over alternating repetitions on shared buffers, one
      process) of the arms
        fused     Hilbert.analytic / .envelope, "fusion" = 1 (absent where the length has no one-launch kernel)
        composed  the same with "fusion" = 0
        caller_a  cast to complex, Fft forward, torch multiply by the mask, Fft inverse (and torch.abs for the envelope)
        caller_b  cast to complex, complex FftConv with the mask's impulse response as its one filter (and torch.abs)
      every arm's spread (max - min) / median, every handle arm over each caller arm, the fused arm over the composed one and whether
      it beats it by more than the larger of the two arms' spreads (the rule a default follows), and the byte model of the analytic
      signal: 12N fused, about 36N composed, about 60N caller_a, in bytes per f32 row."""
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


def mask(torch, n, dtype):
    m = torch.zeros(n, dtype=dtype, device="cuda")
    m[0] = 1
    if n % 2 == 0:
        m[n // 2] = 1
        m[1:n // 2] = 2
    else:
        m[1:(n + 1) // 2] = 2
    return m


def run_case(torch, fa, real, n, what, gib, reps):
    from fourier_amd import Transform

    rdt, cdt = (torch.float32, torch.complex64) if real == "f32" else (torch.float64, torch.complex128)
    rs = 4 if real == "f32" else 8
    per_row = n * rs * (3 if what == "analytic" else 2)  # input plus output
    batch = max(1, int(gib * (1 << 30)) // per_row)
    x = torch.randn(batch, n, dtype=rdt, device="cuda")
    out = torch.empty(batch, n, dtype=cdt if what == "analytic" else rdt, device="cuda")
    plans = {}
    for arm, fusion in (("fused", 1), ("composed", 0)):
        p = fa.Hilbert(n, real, 0)
        p.set_option("fusion", fusion)
        p.reserve(batch)
        plans[arm] = p
    default = fa.Hilbert(n, real, 0).describe()
    if plans["fused"].describe() == plans["composed"].describe():
        del plans["fused"]
    fft = fa.Fft(n, real, 0)
    fft.reserve(batch, True)
    conv = fa.FftConv(n, real, False, 0)
    m = mask(torch, n, rdt)
    taps = torch.fft.ifft(m.to(cdt))  # set-up only: the mask's impulse response
    conv.set_filters(taps.contiguous())
    conv.reserve(batch)
    work = torch.empty(batch, n, dtype=cdt, device="cuda")

    def finish():
        if what == "envelope":
            torch.abs(work, out=out)
        else:
            out.copy_(work)

    def caller_a():
        work.copy_(x)  # the cast to complex
        fft.transform(work, work, Transform.Fft)
        work.mul_(m)
        fft.transform(work, work, Transform.Ifft)
        finish()

    def caller_b():
        work.copy_(x)
        conv.apply(work, out=work)
        finish()

    arms = {arm: (lambda p: (lambda: getattr(p, what)(x, out=out)))(p) for arm, p in plans.items()}
    arms["caller_a"] = caller_a
    arms["caller_b"] = caller_b
    t = time_arms(torch, arms, reps)
    med = {a: v["median_ms"] for a, v in t.items()}
    width = lambda a: t[a]["max_ms"] - t[a]["min_ms"]  # noqa: E731
    over = {a: {c: med[a] / med[c] for c in ("caller_a", "caller_b")} for a in plans}
    fused = None
    if "fused" in plans:
        fused = {"over_composed": med["fused"] / med["composed"],
                 "beats_composed_by_more_than_the_spread": med["composed"] - med["fused"] > max(width("fused"), width("composed"))}
    rec = {"real": real, "n": n, "output": what, "batch": batch, "bytes_in_plus_out": batch * per_row, "default": default,
           "describe": {a: p.describe() for a, p in plans.items()}, "fft": fft.describe(), "conv": conv.describe(), "ms": t,
           "over_caller": over, "fused": fused,
           "byte_model_analytic_bytes_per_f32_row_over_n": {"fused": 12, "composed": 36, "caller_a": 60}}
    del x, out, work, plans, arms, fft, conv
    torch.cuda.empty_cache()
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="f32:2048,f32:8192,f32:32768,f64:2048,f64:16384")
    ap.add_argument("--gib", type=float, default=1.0)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch

    if not torch.cuda.is_available():
        raise SystemExit("needs a GPU")
    import fourier_amd

    recs = []
    for shape in [s for s in args.shapes.split(",") if s]:
        real, n = shape.split(":")
        for what in ("analytic", "envelope"):
            r = run_case(torch, fourier_amd, real, int(n), what, args.gib, args.reps)
            recs.append(r)
            print(json.dumps(r), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as f:
            for r in recs:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
