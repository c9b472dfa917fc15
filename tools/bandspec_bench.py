#!/usr/bin/env python3
"""The band-spectrogram handle (fourier_hip_bandspec_*): its fused route against its composed route and what a caller wrote before it,
on the GPU.

  python tools/bandspec_bench.py [--shapes f32:1024:256:80,...] [--length 1048576] [--batch 64] [--reps 5] [--out FILE]
      One JSON line per shape (precision : n_fft : hop : mels): `batch` rows of `length` reals under a Hann window and the HTK mel bank
      of 16 kHz (mel_filterbank).  The default shapes are f32 and f64 at (512, 128, 40), (1024, 256, 80) and (2048, 512, 128); f64 at
      2048 has no fused kernel and runs the composed route only.  HIP-event milliseconds per call (median / min / max over alternating
      repetitions on shared buffers, one process) of the arms
        fused     BandSpectrogram.forward, "fusion" = 1
        composed  the same with "fusion" = 0
        caller    Spectrogram.forward on its default route into a preallocated (batch, frames, bins) buffer, then torch.matmul with
                  the dense (bins, mels) matrix into a preallocated output
      every arm's spread (max - min) / median, each handle arm over the caller's, the fused arm over the composed one and whether it
      beats it by more than the larger of the two arms' spreads (the rule the default follows: at EVERY shape where the fused route
      exists), and TB/s of every arm on the ALGORITHMIC bytes: the signal in once, the band energies out once.
  A shape is one step: run each group under its own time limit, e.g.  timeout -k 10 300 python tools/bandspec_bench.py --shapes ... --out ..."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

DEFAULT_SHAPES = ",".join(f"{real}:{n}:{hop}:{mels}" for real in ("f32", "f64") for n, hop, mels in ((512, 128, 40), (1024, 256, 80), (2048, 512, 128)))


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


def run_case(torch, fa, real, n_fft, hop, mels, length, batch, reps):
    rdt = torch.float32 if real == "f32" else torch.float64
    es = 4 if real == "f32" else 8
    x = torch.randn(batch, length, dtype=rdt, device="cuda")
    w = torch.hann_window(n_fft, dtype=rdt, device="cuda")
    W = fa.mel_filterbank(n_fft // 2 + 1, 0.0, 8000.0, mels, 16000.0)
    plans = {}
    for arm, fusion in (("fused", 1), ("composed", 0)):
        p = fa.BandSpectrogram(n_fft, mels, real, hop, device=0)
        p.set_option("fusion", fusion)
        p.set_window(w)
        p.set_bands(W)
        p.reserve(length, batch)
        plans[arm] = p
    default = fa.BandSpectrogram(n_fft, mels, real, hop, device=0).describe()
    if plans["fused"].describe() == plans["composed"].describe():
        del plans["fused"]
    nf, bins = plans["composed"].frames(length), plans["composed"].bins()
    out = torch.empty(batch, nf, mels, dtype=rdt, device="cuda")
    # the caller's composition: the full power spectrogram to memory, read back by a dense matmul
    spec = fa.Spectrogram(n_fft, real, hop, device=0)
    spec.set_window(w)
    spec.reserve(length, batch)
    S = torch.empty(batch, nf, bins, dtype=rdt, device="cuda")
    Wt = torch.from_numpy(W).to(rdt).cuda().T.contiguous()

    def caller():
        spec.forward(x, 2, False, out=S)
        torch.matmul(S, Wt, out=out)

    arms = {arm: (lambda p: (lambda: p.forward(x, out=out)))(p) for arm, p in plans.items()}
    arms["caller"] = caller
    # the arms agree before they are timed
    ref = plans["composed"].forward(x[:2]).clone()
    caller()
    agree = {"caller": float((out[:2] - ref).norm() / ref.norm())}
    if "fused" in plans:
        agree["fused"] = float((plans["fused"].forward(x[:2]) - ref).norm() / ref.norm())
    t = time_arms(torch, arms, reps)
    med = {a: v["median_ms"] for a, v in t.items()}
    width = lambda a: t[a]["max_ms"] - t[a]["min_ms"]  # noqa: E731
    fused = None
    if "fused" in plans:
        fused = {"over_composed": med["fused"] / med["composed"],
                 "beats_composed_by_more_than_the_spread": med["composed"] - med["fused"] > max(width("fused"), width("composed"))}
    bytes_in, bytes_out = batch * length * es, batch * nf * mels * es
    rec = {"real": real, "n_fft": n_fft, "hop": hop, "mels": mels, "length": length, "batch": batch, "frames": nf, "bins": bins,
           "bytes_in": bytes_in, "bytes_out": bytes_out, "spectrogram_bytes": batch * nf * bins * es, "default": default,
           "describe": {a: p.describe() for a, p in plans.items()}, "caller_spectrogram": spec.describe(), "ms": t,
           "rel_l2_against_composed": agree, "over_caller": {a: med[a] / med["caller"] for a in plans}, "fused": fused,
           "algorithmic_tb_per_s": {a: (bytes_in + bytes_out) / (med[a] * 1e-3) / 1e12 for a in med}}
    del x, out, S, Wt, plans, arms, spec
    torch.cuda.empty_cache()
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default=DEFAULT_SHAPES)
    ap.add_argument("--length", type=int, default=1 << 20)
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch

    if not torch.cuda.is_available():
        raise SystemExit("needs a GPU")
    import fourier_amd

    for shape in [s for s in args.shapes.split(",") if s]:
        real, n_fft, hop, mels = shape.split(":")
        r = run_case(torch, fourier_amd, real, int(n_fft), int(hop), int(mels), args.length, args.batch, args.reps)
        print(json.dumps(r), flush=True)
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "a") as f:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
