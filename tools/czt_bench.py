#!/usr/bin/env python3
"""The chirp-z handle (fourier_hip_czt_*): its one-launch route against its composed route and what a caller wrote before it, on the GPU.

  python tools/czt_bench.py [--shapes f32:2048,f32:8192,f32:32768,f64:2048,f64:8192,f64:16384] [--gib 1.0] [--reps 7] [--out FILE]
      One JSON line per shape (precision : L): n = m = L / 2 complex rows on the zoom arc (w_turns = -0.1 / m, a_turns = 0.2), the batch
      chosen so that the input is about --gib GiB.  HIP-event milliseconds per call (median / min / max over alternating repetitions on
      shared buffers, one process) of the arms
        fused     Czt.transform, "fusion" = 1 (absent where L has no one-launch kernel)
        composed  the same with "fusion" = 0
        caller    torch: chirp multiply into a zero-padded (batch, L) array, complex FftConv of L points with v as its one filter,
                  slice and chirp multiply
      every arm's spread (max - min) / median, each handle arm over the caller's, the fused arm over the composed one and whether it
      beats it by more than the larger of the two arms' spreads (the rule the default follows: at EVERY measured L), and the byte MODEL
      per f32 complex row (a model, not a measurement): 8n + 8m fused, at least 8n + 8m + 48L composed.
  A shape is one step: run each under its own time limit, e.g.  timeout -k 10 300 python tools/czt_bench.py --shapes f32:2048 --out ..."""
import argparse
import json
import os
import statistics
import sys

import numpy as np

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


def chirp(turns, idx):
    """exp(2 pi i frac(turns idx^2 / 2)) in f64 (the caller's tables: set-up only)"""
    q = np.asarray(idx, dtype=np.float64) ** 2 / 2
    return np.exp(2j * np.pi * np.modf(turns * q)[0])


def run_case(torch, fa, real, L, gib, reps):
    cdt = torch.complex64 if real == "f32" else torch.complex128
    es = 8 if real == "f32" else 16
    n = m = L // 2
    w_turns, a_turns = -0.1 / m, 0.2
    batch = max(1, int(gib * (1 << 30)) // (n * es))
    x = torch.randn(batch, n, dtype=cdt, device="cuda")
    out = torch.empty(batch, m, dtype=cdt, device="cuda")
    plans = {}
    for arm, fusion in (("fused", 1), ("composed", 0)):
        p = fa.Czt(n, m, 1.0, w_turns, 1.0, a_turns, real, False, 0)
        p.set_option("fusion", fusion)
        p.reserve(batch)
        plans[arm] = p
    default = fa.Czt(n, m, 1.0, w_turns, 1.0, a_turns, real, False, 0).describe()
    if plans["fused"].describe() == plans["composed"].describe():
        del plans["fused"]
    # the caller's composition: tables once, then per call multiply + pad, FftConv, slice + multiply
    j = np.arange(n)
    A = torch.from_numpy(chirp(w_turns, j) * np.exp(-2j * np.pi * np.modf(a_turns * j)[0])).to(cdt).cuda()
    B = torch.from_numpy(chirp(w_turns, np.arange(m))).to(cdt).cuda()
    v = np.zeros(L, np.complex128)
    v[:m] = chirp(-w_turns, np.arange(m))
    v[L - n + 1:] = chirp(-w_turns, np.arange(n - 1, 0, -1))
    conv = fa.FftConv(L, real, False, 0)
    conv.set_filters(torch.from_numpy(v).to(cdt).cuda().contiguous())
    conv.reserve(batch)
    work = torch.zeros(batch, L, dtype=cdt, device="cuda")

    def caller():
        torch.mul(x, A, out=work[:, :n])
        work[:, n:].zero_()
        conv.apply(work, out=work)
        torch.mul(work[:, :m], B, out=out)

    arms = {arm: (lambda p: (lambda: p.transform(x, out=out)))(p) for arm, p in plans.items()}
    arms["caller"] = caller
    # the arms agree before they are timed
    ref = plans["composed"].transform(x[:4]).clone()
    caller()
    agree = {"caller": float((out[:4] - ref).norm() / ref.norm())}
    if "fused" in plans:
        agree["fused"] = float((plans["fused"].transform(x[:4]) - ref).norm() / ref.norm())
    t = time_arms(torch, arms, reps)
    med = {a: v_["median_ms"] for a, v_ in t.items()}
    width = lambda a: t[a]["max_ms"] - t[a]["min_ms"]  # noqa: E731
    fused = None
    if "fused" in plans:
        fused = {"over_composed": med["fused"] / med["composed"],
                 "beats_composed_by_more_than_the_spread": med["composed"] - med["fused"] > max(width("fused"), width("composed"))}
    rec = {"real": real, "L": L, "n": n, "m": m, "batch": batch, "bytes_in": batch * n * es, "bytes_out": batch * m * es, "default": default,
           "describe": {a: p.describe() for a, p in plans.items()}, "conv": conv.describe(), "ms": t,
           "rel_l2_against_composed": agree, "over_caller": {a: med[a] / med["caller"] for a in plans}, "fused": fused,
           "byte_model_f32_bytes_per_row": {"fused": 8 * n + 8 * m, "composed_at_least": 8 * n + 8 * m + 48 * L}}
    del x, out, work, plans, arms, conv
    torch.cuda.empty_cache()
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="f32:2048,f32:8192,f32:32768,f64:2048,f64:8192,f64:16384")
    ap.add_argument("--gib", type=float, default=1.0)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch

    if not torch.cuda.is_available():
        raise SystemExit("needs a GPU")
    import fourier_amd

    for shape in [s for s in args.shapes.split(",") if s]:
        real, L = shape.split(":")
        r = run_case(torch, fourier_amd, real, int(L), args.gib, args.reps)
        print(json.dumps(r), flush=True)
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "a") as f:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
