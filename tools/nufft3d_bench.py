#!/usr/bin/env python3
"""The 3-D non-uniform FFT handle (fourier_hip_nufft3d_*) on its two routes against what a caller wrote before it, on the GPU.

  python tools/nufft3d_bench.py [--cases large:f32,large:f64,many:f32,many:f64,clustered:f32,clustered:f64] [--scale 1] [--reps 5]
                                [--caller-reps-f64 N] [--out FILE]
      Two JSON lines per case, type 1 (to_modes, isign -1) and type 2 (to_points, isign +1):
        large      n = 128 x 128 x 128 modes, M = 2^22 uniform random points, batch 2
        many       n = 32 x 32 x 32, M = 2^15 uniform random points, batch 128
        clustered  the `large` shape with every point inside 10 % of the period in every coordinate (reported as it is: the gather's
                   lanes over the cluster walk runs a thousand times the average, the others none)
      eps = 1e-6 at f32, 1e-12 at f64.  (--scale divides the batch and M, for a quick look.)  HIP-event milliseconds per call (median
      / min / max over alternating repetitions on shared buffers, one process) of the arms
        evaluated  Nufft3d, "table" = 0
        tabulated  Nufft3d, "table" = 1
        caller     the composition a caller had: w^3 torch index_add_ passes (atomics: not reproducible) onto a zeroed grid, fftn, a
                   slice and a multiply for type 1; a zero-fill, scatter and multiply, fftn and w^3 gathers for type 2; its weights
                   and factors prepared outside the timed region
      every arm's spread (max - min) / median, every handle arm over the caller arm, the tabulated arm over the evaluated one and
      whether it beats it by more than the larger of the two arms' widths (the rule the default follows), and the handle arms' relative
      L2 distance from the caller arm.  The caller arm makes w^3 passes over M points, 2197 at f64: --caller-reps-f64 gives it fewer
      repetitions there (it then joins the first N rounds of the alternation only, after one warm-up call instead of two); each line
      says how many repetitions every arm had ("reps")."""
import argparse
import json
import math
import os
import re
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from tools.nufft2d_bench import caller_axis  # noqa: E402  (the caller's own preparation for one axis)

CASES = {"large": ((128, 128, 128), 1 << 22, 2, 1.0), "many": ((32, 32, 32), 1 << 15, 128, 1.0), "clustered": ((128, 128, 128), 1 << 22, 2, 0.1)}
EPS = {"f32": 1e-6, "f64": 1e-12}


def time_arms(torch, arms, reps, warmup=2):
    """reps: repetitions per arm; an arm with fewer joins the first rounds only, and has one warm-up call fewer per repetition it lacks
    (never less than one)"""
    rounds = max(reps.values())
    for i in range(warmup):
        for k, f in arms.items():
            if i < max(1, warmup - (rounds - reps[k])):
                f()
    torch.cuda.synchronize()
    ms = {k: [] for k in arms}
    for i in range(rounds):
        for k, f in arms.items():
            if i >= reps[k]:
                continue
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            f()
            b.record()
            b.synchronize()
            ms[k].append(a.elapsed_time(b))
    return {k: {"median_ms": statistics.median(v), "min_ms": min(v), "max_ms": max(v), "reps": len(v),
                "spread": (max(v) - min(v)) / statistics.median(v)} for k, v in ms.items()}


def run_case(torch, fa, truth, name, real, scale, reps, caller_reps):
    import numpy as np

    n, m, batch, width = CASES[name]
    batch, m = max(1, batch // scale), max(1, m // scale)
    eps = EPS[real]
    rdt, cdt = (torch.float32, torch.complex64) if real == "f32" else (torch.float64, torch.complex128)
    rng = np.random.default_rng(1)
    x = [rng.uniform(-math.pi * width, math.pi * width, m) for _ in range(3)]
    c = torch.randn((batch, m), dtype=cdt, device="cuda")
    f = torch.randn((batch,) + n, dtype=cdt, device="cuda")
    oc, of = torch.empty_like(c), torch.empty_like(f)
    plans = {}
    for arm, table in (("evaluated", 0), ("tabulated", 1)):
        p = fa.Nufft3d(n, eps, real, 0)
        p.set_option("table", table)
        p.set_points(*x)
        p.reserve(batch)
        plans[arm] = p
    default = fa.Nufft3d(n, eps, real, 0).describe()
    w, L1, L2, L3 = (int(s) for s in re.match(r"nufft3d \w+: w (\d+), L (\d+) x (\d+) x (\d+), ", plans["evaluated"].describe()).groups())
    L = (L1, L2, L3)
    ax = [caller_axis(torch, truth, x[d], n[d], w, L[d], rdt) for d in range(3)]
    (cells1, wt1, inv1, ck1), (cells2, wt2, inv2, ck2), (cells3, wt3, inv3, ck3) = ax
    inv = inv1[:, None, None] * inv2[None, :, None] * inv3[None, None, :]
    mode_cells = ((ck1[:, None, None] * L2 + ck2[None, :, None]) * L3 + ck3[None, None, :]).reshape(-1)  # the flat cell of every mode
    cells = L1 * L2 * L3
    grid, grid2 = torch.empty((batch,) + L, dtype=cdt, device="cuda"), torch.empty((batch,) + L, dtype=cdt, device="cuda")
    flat, flat2 = grid.view(batch, cells), grid2.view(batch, cells)

    def caller1():
        grid.zero_()
        gr, cr = torch.view_as_real(flat), torch.view_as_real(c)
        for t1 in range(w):
            for t2 in range(w):
                c12, w12 = (cells1[:, t1] * L2 + cells2[:, t2]) * L3, wt1[:, t1] * wt2[:, t2]
                for t3 in range(w):
                    gr.index_add_(1, c12 + cells3[:, t3], cr * (w12 * wt3[:, t3])[None, :, None])
        fa.fftn(grid, (-3, -2, -1), fa.Transform.Fft, out=grid2)
        torch.mul(flat2[:, mode_cells].view((batch,) + n), inv[None], out=of)

    def caller2():
        grid.zero_()
        flat[:, mode_cells] = (f * inv[None]).view(batch, -1)
        fa.fftn(grid, (-3, -2, -1), fa.Transform.UnscaledIfft, out=grid2)
        oc.zero_()
        for t1 in range(w):
            for t2 in range(w):
                c12, w12 = (cells1[:, t1] * L2 + cells2[:, t2]) * L3, wt1[:, t1] * wt2[:, t2]
                for t3 in range(w):
                    oc.add_(flat2[:, c12 + cells3[:, t3]] * (w12 * wt3[:, t3])[None, :])

    recs = []
    for typ, callerf, out, run in ((1, caller1, of, lambda p: p.to_modes(c, -1, 0, out=of)), (2, caller2, oc, lambda p: p.to_points(f, 1, 0, out=oc))):
        arms = {arm: (lambda p: (lambda: run(p)))(p) for arm, p in plans.items()}
        arms["caller"] = callerf
        t = time_arms(torch, arms, {"evaluated": reps, "tabulated": reps, "caller": caller_reps})
        med = {arm: v["median_ms"] for arm, v in t.items()}
        wid = lambda arm: t[arm]["max_ms"] - t[arm]["min_ms"]  # noqa: E731
        ys = {}
        for arm, fn in arms.items():
            fn()
            ys[arm] = out.clone()
        ref = ys["caller"].to(torch.complex128)
        agree = {arm: float(((ys[arm].to(torch.complex128) - ref).norm() / ref.norm()).item()) for arm in plans}
        recs.append({"case": name, "real": real, "type": typ, "n_modes": list(n), "points": m, "batch": batch, "eps": eps, "w": w, "L": list(L),
                     "points_within": width, "default": default, "describe": {arm: p.describe() for arm, p in plans.items()}, "ms": t,
                     "over_caller": {arm: med[arm] / med["caller"] for arm in plans},
                     "tabulated": {"over_evaluated": med["tabulated"] / med["evaluated"],
                                   "beats_evaluated_by_more_than_the_spread": med["evaluated"] - med["tabulated"] > max(wid("tabulated"), wid("evaluated"))},
                     "rel_l2_against_caller": agree})
        del ys, ref
    del c, f, oc, of, grid, grid2, flat, flat2, plans, ax, cells1, cells2, cells3, wt1, wt2, wt3
    torch.cuda.empty_cache()
    return recs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default="large:f32,large:f64,many:f32,many:f64,clustered:f32,clustered:f64")
    ap.add_argument("--scale", type=int, default=1)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--caller-reps-f64", type=int, default=None, help="repetitions of the caller arm at f64 (default: --reps)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch

    if not torch.cuda.is_available():
        raise SystemExit("needs a GPU")
    import fourier_amd
    import nufft_truth

    for case in [s for s in args.cases.split(",") if s]:
        name, real = case.split(":")
        caller_reps = args.caller_reps_f64 if real == "f64" and args.caller_reps_f64 else args.reps
        if caller_reps < args.reps:
            print(f"# {case}: the caller arm runs {caller_reps} of the {args.reps} repetitions (w^3 passes over the points per call)", flush=True)
        for r in run_case(torch, fourier_amd, nufft_truth, name, real, args.scale, args.reps, caller_reps):
            print(json.dumps(r), flush=True)
            if args.out:  # appended line by line: a run that is cut short keeps what it measured
                os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
                with open(args.out, "a") as f:
                    f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
