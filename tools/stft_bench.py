#!/usr/bin/env python3
"""The STFT handle (fourier_hip_stft_*) against what a caller wrote before it, on the GPU.

  python tools/stft_bench.py [--reals f32,f64] [--nfft 256,512,1024,2048] [--speech] [--reps 5] [--out FILE]
      One JSON line per precision, n_fft and hop (n_fft / 4 and n_fft / 2; length 2^20, batch 64; --speech adds 400 / 160, length
      2^18, batch 256): HIP-event milliseconds per call (median / min / max over alternating repetitions on shared buffers) of the arms
        handle    Stft.forward on its default route
        composed  the handle with "fusion" = 0
        fused     the handle with "fusion" = 1 (only where that route exists and is not the default already)
        caller    torch reflect pad + unfold + window multiply + RealFft.rfft: what could be written without the handle
        torch     torch.stft, for information
      every arm's spread (max - min) / median, the ratios, the rate of every arm on the algorithmic bytes (length reals in and
      frames x bins complex out per row) and the ratio the byte model predicts for fused over composed,
      (n_fft + 2 + hop) / (5 n_fft + hop)."""
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


def run_case(torch, fa, real, n, hop, length, batch, reps):
    rdt, cdt = (torch.float32, torch.complex64) if real == "f32" else (torch.float64, torch.complex128)
    val = torch.empty(0, dtype=rdt).element_size()
    x = torch.randn(batch, length, dtype=rdt, device="cuda")
    w = torch.hann_window(n, dtype=rdt, device="cuda")
    plans = {}
    for arm, fusion in (("handle", None), ("composed", 0), ("fused", 1)):
        p = fa.Stft(n, real, hop, device=0)
        p.set_window(w)
        if fusion is not None:
            p.set_option("fusion", fusion)
        p.reserve(length, batch)
        plans[arm] = p
    if plans["fused"].describe() in (plans["handle"].describe(), plans["composed"].describe()):
        del plans["fused"]
    nf, bins = plans["handle"].frames(length), n // 2 + 1
    out = torch.empty(batch, nf, bins, dtype=cdt, device="cuda")
    rfft = fa.RealFft(n, real, 0)
    rfft.reserve(batch * nf)
    stream = torch.cuda.current_stream().cuda_stream

    def caller():
        xp = torch.nn.functional.pad(x[:, None], (n // 2, n // 2), mode="reflect")[:, 0]
        fr = xp.unfold(-1, n, hop) * w
        rfft.forward_batch_ptr(fr.data_ptr(), out.data_ptr(), batch * nf, 0, stream)

    arms = {arm: (lambda p: (lambda: p.forward(x, out=out)))(p) for arm, p in plans.items()}
    arms["caller"] = caller
    arms["torch"] = lambda: torch.stft(x, n, hop, n, w, center=True, pad_mode="reflect", onesided=True, return_complex=True)
    t = time_arms(torch, arms, reps)
    med = {a: v["median_ms"] for a, v in t.items()}
    nbytes = batch * (length * val + nf * bins * 2 * val)
    fused_ms = med.get("fused", med["handle"] if plans["handle"].describe().startswith("stft fused") else None)
    rec = {"real": real, "n_fft": n, "hop": hop, "length": length, "batch": batch, "frames": nf,
           "describe": {a: p.describe() for a, p in plans.items()}, "ms": t,
           "handle_over_caller": med["handle"] / med["caller"], "composed_over_caller": med["composed"] / med["caller"],
           "fused_over_composed": fused_ms / med["composed"] if fused_ms else None,
           "byte_model_fused_over_composed": (n + 2 + hop) / (5 * n + hop),
           "algorithmic_bytes": nbytes, "tbs_on_algorithmic_bytes": {a: nbytes / (v * 1e-3) / 1e12 for a, v in med.items()}}
    del x, out, plans, arms, rfft
    torch.cuda.empty_cache()
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reals", default="f32,f64")
    ap.add_argument("--nfft", default="256,512,1024,2048")
    ap.add_argument("--speech", action="store_true")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch

    if not torch.cuda.is_available():
        raise SystemExit("needs a GPU")
    import fourier_amd

    cases = []
    for real in [r for r in args.reals.split(",") if r]:
        for n in [int(v) for v in args.nfft.split(",") if v]:
            for hop in (n // 4, n // 2):
                cases.append((real, n, hop, 1 << 20, 64))
        if args.speech:
            cases.append((real, 400, 160, 1 << 18, 256))
    recs = []
    for case in cases:
        r = run_case(torch, fourier_amd, *case, args.reps)
        recs.append(r)
        print(json.dumps(r), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as f:
            for r in recs:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
