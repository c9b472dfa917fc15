#!/usr/bin/env python3
"""The non-uniform FFT handle (fourier_hip_nufft_*) on its two routes against what a caller wrote before it, on the GPU.

  python tools/nufft_bench.py [--cases large:f32,large:f64,many:f32,many:f64,clustered:f32] [--scale 1] [--reps 5] [--out FILE]
      Two JSON lines per case, type 1 (to_modes, isign -1) and type 2 (to_points, isign +1):
        large      N = 2^20 modes, M = 2^21 uniform random points, batch 16
        many       N = 4096, M = 8192 uniform random points, batch 4096
        clustered  the `large` shape with every point inside 1 % of the period (reported as it is: the gather's lanes over the
                   cluster walk runs a hundred times the average, the others none)
      eps = 1e-6 at f32, 1e-12 at f64.  (--scale divides the batch, for a quick look.)  HIP-event milliseconds per call (median / min
      / max over alternating repetitions on shared buffers, one process) of the arms
        evaluated  Nufft, "table" = 0
        tabulated  Nufft, "table" = 1
        caller     the composition a caller had: w torch index_add_ passes (atomics: not reproducible) onto a zeroed grid, Fft, a
                   slice and a multiply for type 1; a zero-fill, scatter and multiply, Fft and w gathers for type 2; its weights
                   and factors prepared outside the timed region
      every arm's spread (max - min) / median, every handle arm over the caller arm, the tabulated arm over the evaluated one and
      whether it beats it by more than the larger of the two arms' widths (the rule the default follows), and the handle arms' relative
      L2 distance from the caller arm."""
import argparse
import json
import math
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

CASES = {"large": (1 << 20, 1 << 21, 16, 1.0), "many": (4096, 8192, 4096, 1.0), "clustered": (1 << 20, 1 << 21, 16, 0.01)}
EPS = {"f32": 1e-6, "f64": 1e-12}


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


def caller_tables(torch, truth, x, n, w, L, rdt):
    """the caller's own preparation: cells [M, w], weights [M, w] in T, 1 / phihat per mode (k ascending) and the modes' cells"""
    import numpy as np

    xt = torch.from_numpy(x).cuda()
    xg = torch.remainder(xt, 2 * math.pi) * (L / (2 * math.pi))
    xg = torch.where(xg >= L, xg - L, xg)
    c = torch.ceil(xg - w / 2)
    d = c - xg
    t = torch.arange(w, device="cuda", dtype=torch.float64)
    z = (d[:, None] + t[None, :]) * (2.0 / w)
    wt = torch.exp(2.30 * w * (torch.sqrt(torch.clamp(1 - z * z, min=0)) - 1)).to(rdt)
    cells = torch.remainder(c.long()[:, None] + torch.arange(w, device="cuda")[None, :], L)
    mags = np.arange(n // 2 + 1)
    ph = np.concatenate([truth.phihat(w, L, mags[i:i + 16384]) for i in range(0, len(mags), 16384)])
    k = truth.mode_indices(n, 0)
    inv = torch.from_numpy((1.0 / ph)[np.abs(k)]).cuda().to(rdt)
    cell_of_k = torch.from_numpy(np.where(k < 0, k + L, k)).cuda()
    return cells, wt, inv, cell_of_k


def run_case(torch, fa, truth, name, real, scale, reps):
    import numpy as np

    n, m, batch, width = CASES[name]
    batch = max(1, batch // scale)
    eps = EPS[real]
    rdt, cdt = (torch.float32, torch.complex64) if real == "f32" else (torch.float64, torch.complex128)
    rng = np.random.default_rng(1)
    x = rng.uniform(-math.pi * width, math.pi * width, m)
    c = torch.randn((batch, m), dtype=cdt, device="cuda")
    f = torch.randn((batch, n), dtype=cdt, device="cuda")
    oc, of = torch.empty_like(c), torch.empty_like(f)
    plans = {}
    for arm, table in (("evaluated", 0), ("tabulated", 1)):
        p = fa.Nufft(n, eps, real, 0)
        p.set_option("table", table)
        p.set_points(x)
        p.reserve(batch)
        plans[arm] = p
    default = fa.Nufft(n, eps, real, 0).describe()
    w, L = (int(s) for s in plans["evaluated"].describe().split(": ")[1].replace("w ", "").replace("L ", "").split(", ")[:2])
    cells, wt, inv, cell_of_k = caller_tables(torch, truth, x, n, w, L, rdt)
    fft = fa.Fft(L, real, 0)
    grid, grid2 = torch.empty((batch, L), dtype=cdt, device="cuda"), torch.empty((batch, L), dtype=cdt, device="cuda")

    def caller1():
        grid.zero_()
        gr, cr = torch.view_as_real(grid), torch.view_as_real(c)
        for t in range(w):
            gr.index_add_(1, cells[:, t], cr * wt[None, :, t, None])
        fft.transform(grid, grid2, fa.Transform.Fft)
        torch.mul(grid2[:, cell_of_k], inv[None, :], out=of)

    def caller2():
        grid.zero_()
        grid[:, cell_of_k] = f * inv[None, :]
        fft.transform(grid, grid2, fa.Transform.UnscaledIfft)
        oc.zero_()
        for t in range(w):
            oc.add_(grid2[:, cells[:, t]] * wt[None, :, t])

    recs = []
    for typ, callerf, out, run in ((1, caller1, of, lambda p: p.to_modes(c, -1, 0, out=of)), (2, caller2, oc, lambda p: p.to_points(f, 1, 0, out=oc))):
        arms = {arm: (lambda p: (lambda: run(p)))(p) for arm, p in plans.items()}
        arms["caller"] = callerf
        t = time_arms(torch, arms, reps)
        med = {arm: v["median_ms"] for arm, v in t.items()}
        wid = lambda arm: t[arm]["max_ms"] - t[arm]["min_ms"]  # noqa: E731
        ys = {}
        for arm, fn in arms.items():
            fn()
            ys[arm] = out.clone()
        ref = ys["caller"].to(torch.complex128)
        agree = {arm: float(((ys[arm].to(torch.complex128) - ref).norm() / ref.norm()).item()) for arm in plans}
        recs.append({"case": name, "real": real, "type": typ, "n_modes": n, "points": m, "batch": batch, "eps": eps, "w": w, "L": L,
                     "points_within": width, "default": default, "describe": {arm: p.describe() for arm, p in plans.items()}, "ms": t,
                     "over_caller": {arm: med[arm] / med["caller"] for arm in plans},
                     "tabulated": {"over_evaluated": med["tabulated"] / med["evaluated"],
                                   "beats_evaluated_by_more_than_the_spread": med["evaluated"] - med["tabulated"] > max(wid("tabulated"), wid("evaluated"))},
                     "rel_l2_against_caller": agree})
        del ys, ref
    del c, f, oc, of, grid, grid2, plans, cells, wt
    torch.cuda.empty_cache()
    return recs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default="large:f32,large:f64,many:f32,many:f64,clustered:f32")
    ap.add_argument("--scale", type=int, default=1)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch

    if not torch.cuda.is_available():
        raise SystemExit("needs a GPU")
    import fourier_amd
    import nufft_truth

    recs = []
    for case in [s for s in args.cases.split(",") if s]:
        name, real = case.split(":")
        for r in run_case(torch, fourier_amd, nufft_truth, name, real, args.scale, args.reps):
            recs.append(r)
            print(json.dumps(r), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as f:
            for r in recs:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
