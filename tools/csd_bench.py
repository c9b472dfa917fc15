#!/usr/bin/env python3
"""The cross-spectrum handle (fourier_hip_csd_*) against what a caller wrote before it, on the GPU.

  python tools/csd_bench.py [--shapes f32:1024:64,f32:256:64,f64:1024:32] [--reps 7] [--out FILE]
      One JSON line per shape (precision : n_fft : rows; hop n_fft / 2, Welch's usual one; rows of 2^20): HIP-event milliseconds per
      call (median / min / max over alternating repetitions on shared buffers, one process) of the arms
        csd_fused           CrossSpectrum.csd, "fusion" = 1 (absent where the fused route does not exist)
        csd_composed        the same with "fusion" = 0
        csd_caller          Stft.forward(x), Stft.forward(y), (conj(X) * Y).mean(1): the composition a caller had before this handle
        coherence_fused     CrossSpectrum.coherence, "fusion" = 1
        coherence_composed  the same with "fusion" = 0
        coherence_caller    ... plus the two power means and the division
      every arm's spread (max - min) / median, every handle arm over its caller arm, the fused arm over the composed one and whether it
      beats it by more than the larger of the two arms' spreads (the rule a default follows), and the byte model's ratio
      (DESIGN.md section 4): 8L / 56L at hop = n_fft / 2."""
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


def byte_model(n, hop):
    """values moved per input sample of ONE signal, v = bins / hop complex output values per sample, in reals: (the fused CSD, the
    caller's CSD composition).  The composition is counted at its least: two STFTs (1 + 2v each), the product that reads both and writes
    one (6v), the mean that reads it (2v).  hop = n_fft / 2, v = 1: 2 and 14 -- 8L and 56L bytes at f32."""
    v = (n / 2 + 1) / hop
    return 2.0, 2 * (1 + 2 * v) + 6 * v + 2 * v


def run_case(torch, fa, real, n, hop, length, batch, reps):
    rdt, cdt = (torch.float32, torch.complex64) if real == "f32" else (torch.float64, torch.complex128)
    x = torch.randn(batch, length, dtype=rdt, device="cuda")
    y = 0.6 * torch.roll(x, 5, -1) + 0.8 * torch.randn(batch, length, dtype=rdt, device="cuda")
    w = torch.hann_window(n, dtype=rdt, device="cuda")
    plans = {}
    for arm, fusion in (("fused", 1), ("composed", 0)):
        p = fa.CrossSpectrum(n, real, hop, device=0)
        p.set_window(w)
        p.set_option("fusion", fusion)
        p.reserve(length, batch)
        plans[arm] = p
    default = fa.CrossSpectrum(n, real, hop, device=0).describe()
    if plans["fused"].describe() == plans["composed"].describe():
        del plans["fused"]
    stft = fa.Stft(n, real, hop, device=0)
    stft.set_window(w)
    stft.reserve(length, batch)
    nf, bins = stft.frames(length), n // 2 + 1
    X = torch.empty(batch, nf, bins, dtype=cdt, device="cuda")
    Y = torch.empty(batch, nf, bins, dtype=cdt, device="cuda")
    P = torch.empty(batch, bins, dtype=cdt, device="cuda")
    C = torch.empty(batch, bins, dtype=rdt, device="cuda")

    def caller_csd():
        stft.forward(x, out=X)
        stft.forward(y, out=Y)
        return (torch.conj(X) * Y).mean(1)

    def caller_coherence():
        pxy = caller_csd()
        return pxy.abs().square() / (X.abs().square().mean(1) * Y.abs().square().mean(1))

    arms = {}
    for arm, p in plans.items():
        arms["csd_" + arm] = (lambda p: (lambda: p.csd(x, y, False, 1.0, out=P)))(p)
        arms["coherence_" + arm] = (lambda p: (lambda: p.coherence(x, y, out=C)))(p)
    arms["csd_caller"] = caller_csd
    arms["coherence_caller"] = caller_coherence
    t = time_arms(torch, arms, reps)
    med = {a: v["median_ms"] for a, v in t.items()}
    width = lambda a: t[a]["max_ms"] - t[a]["min_ms"]  # noqa: E731
    ratios, fused = {}, {}
    for a in med:
        kind, who = a.split("_")
        if who != "caller":
            ratios[a] = med[a] / med[kind + "_caller"]
        if who == "fused":
            c = kind + "_composed"
            fused[kind] = {"over_composed": med[a] / med[c], "beats_composed_by_more_than_the_spread": med[c] - med[a] > max(width(a), width(c))}
    m = byte_model(n, hop)
    rec = {"real": real, "n_fft": n, "hop": hop, "length": length, "batch": batch, "frames": nf, "default": default,
           "describe": {a: p.describe() for a, p in plans.items()}, "stft": stft.describe(), "ms": t, "over_caller": ratios, "fused": fused,
           "byte_model_over_caller": m[0] / m[1]}
    del x, y, X, Y, P, C, plans, arms, stft
    torch.cuda.empty_cache()
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="f32:1024:64,f32:256:64,f64:1024:32")
    ap.add_argument("--length", type=int, default=1 << 20)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch

    if not torch.cuda.is_available():
        raise SystemExit("needs a GPU")
    import fourier_amd

    recs = []
    for shape in [s for s in args.shapes.split(",") if s]:
        real, n, batch = shape.split(":")
        r = run_case(torch, fourier_amd, real, int(n), int(n) // 2, args.length, int(batch), args.reps)
        recs.append(r)
        print(json.dumps(r), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as f:
            for r in recs:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
