#!/usr/bin/env python3
"""The spectrogram handle (fourier_hip_spectrogram_*) against what a caller wrote before it, on the GPU.

  python tools/spectrogram_bench.py [--reals f32,f64] [--nfft 256,512,1024,2048] [--reps 5] [--out FILE]
      One JSON line per precision, n_fft and hop (n_fft / 4 and n_fft / 2; 64 rows of 2^20): HIP-event milliseconds per call (median /
      min / max over alternating repetitions on shared buffers, one process) of the arms
        spec_fused      Spectrogram.forward, power 2, "fusion" = 1 (absent where the fused route does not exist)
        spec_composed   the same with "fusion" = 0
        spec_caller     Stft.forward + .abs().square(): the composition a caller had before this handle (the comparison arm)
        welch_fused     Spectrogram.welch, "fusion" = 1
        welch_composed  the same with "fusion" = 0
        welch_caller    Stft.forward + .abs().square().mean(1)
      every arm's spread (max - min) / median, every handle arm over its caller arm, whether it beats the caller by more than the
      caller arm's spread, and the byte model's ratios: 12L / 44L and 4L / 52L at hop = n_fft / 4."""
import argparse
import json
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


def byte_model(n, hop):
    """values moved per input sample, v = bins / hop output values per sample: (fused spectrogram, fused Welch, the spectrogram
    composition, the Welch composition).  The composition is counted at its least: the STFT (1 + 2v), one elementwise pass that reads
    the complex frames and writes reals (3v), and for Welch one read of those (v).  hop = n_fft / 4: 3, 1, 11, 13 -- 12L, 4L, 44L, 52L."""
    v = (n / 2 + 1) / hop
    return 1 + v, 1.0, 1 + 5 * v, 1 + 6 * v


def run_case(torch, fa, real, n, hop, length, batch, reps):
    rdt, cdt = (torch.float32, torch.complex64) if real == "f32" else (torch.float64, torch.complex128)
    x = torch.randn(batch, length, dtype=rdt, device="cuda")
    w = torch.hann_window(n, dtype=rdt, device="cuda")
    plans = {}
    for arm, fusion in (("fused", 1), ("composed", 0)):
        p = fa.Spectrogram(n, real, hop, device=0)
        p.set_window(w)
        p.set_option("fusion", fusion)
        p.reserve(length, batch)
        plans[arm] = p
    default = fa.Spectrogram(n, real, hop, device=0).describe()
    if plans["fused"].describe() == plans["composed"].describe():
        del plans["fused"]
    stft = fa.Stft(n, real, hop, device=0)
    stft.set_window(w)
    stft.reserve(length, batch)
    nf, bins = stft.frames(length), n // 2 + 1
    X = torch.empty(batch, nf, bins, dtype=cdt, device="cuda")
    S = torch.empty(batch, nf, bins, dtype=rdt, device="cuda")
    P = torch.empty(batch, bins, dtype=rdt, device="cuda")
    arms = {}
    for arm, p in plans.items():
        arms["spec_" + arm] = (lambda p: (lambda: p.forward(x, 2, out=S)))(p)
        arms["welch_" + arm] = (lambda p: (lambda: p.welch(x, False, 1.0, out=P)))(p)
    arms["spec_caller"] = lambda: stft.forward(x, out=X).abs().square()
    arms["welch_caller"] = lambda: stft.forward(x, out=X).abs().square().mean(1)
    t = time_arms(torch, arms, reps)
    med = {a: v["median_ms"] for a, v in t.items()}
    ratios, beats = {}, {}
    for a in med:
        kind, who = a.split("_")
        if who != "caller":
            c = kind + "_caller"
            ratios[a] = med[a] / med[c]
            beats[a] = med[c] - med[a] > t[c]["max_ms"] - t[c]["min_ms"]
    m = byte_model(n, hop)
    rec = {"real": real, "n_fft": n, "hop": hop, "length": length, "batch": batch, "frames": nf, "default": default,
           "describe": {a: p.describe() for a, p in plans.items()}, "stft": stft.describe(), "ms": t, "over_caller": ratios,
           "beats_caller_by_more_than_its_spread": beats,
           "byte_model_over_caller": {"spec_fused": m[0] / m[2], "welch_fused": m[1] / m[3]}}
    del x, X, S, P, plans, arms, stft
    torch.cuda.empty_cache()
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reals", default="f32,f64")
    ap.add_argument("--nfft", default="256,512,1024,2048")
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
        for n in [int(v) for v in args.nfft.split(",") if v]:
            for hop in (n // 4, n // 2):
                r = run_case(torch, fourier_amd, real, n, hop, args.length, args.batch, args.reps)
                recs.append(r)
                print(json.dumps(r), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as f:
            for r in recs:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
