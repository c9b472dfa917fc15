#!/usr/bin/env python3
"""The 2-D non-uniform FFT handle (fourier_hip_nufft2d_*) on its two routes against what a caller wrote before it, on the GPU.

  python tools/nufft2d_bench.py [--cases large:f32,large:f64,many:f32,many:f64,clustered:f32] [--scale 1] [--reps 5] [--out FILE]
      Two JSON lines per case, type 1 (to_modes, isign -1) and type 2 (to_points, isign +1):
        large      n = 1024 x 1024 modes, M = 2^22 uniform random points, batch 4
        many       n = 64 x 64, M = 8192 uniform random points, batch 1024
        clustered  the `large` shape with every point inside 10 % of the period in both coordinates (reported as it is: the gather's
                   lanes over the cluster walk runs a hundred times the average, the others none)
      eps = 1e-6 at f32, 1e-12 at f64.  (--scale divides the batch and M, for a quick look.)  HIP-event milliseconds per call (median
      / min / max over alternating repetitions on shared buffers, one process) of the arms
        evaluated  Nufft2d, "table" = 0
        tabulated  Nufft2d, "table" = 1
        caller     the composition a caller had: w^2 torch index_add_ passes (atomics: not reproducible) onto a zeroed grid, fftn, a
                   slice and a multiply for type 1; a zero-fill, scatter and multiply, fftn and w^2 gathers for type 2; its weights
                   and factors prepared outside the timed region
      every arm's spread (max - min) / median, every handle arm over the caller arm, the tabulated arm over the evaluated one and
      whether it beats it by more than the larger of the two arms' widths (the rule the default follows), and the handle arms' relative
      L2 distance from the caller arm."""
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

CASES = {"large": ((1024, 1024), 1 << 22, 4, 1.0), "many": ((64, 64), 8192, 1024, 1.0), "clustered": ((1024, 1024), 1 << 22, 4, 0.1)}
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


def caller_axis(torch, truth, x, n, w, L, rdt):
    """the caller's own preparation for one axis: cells [M, w], weights [M, w] in T, 1 / phihat per mode (k ascending), the modes' cells"""
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
    k = truth.mode_indices(n, 0)
    inv = torch.from_numpy((1.0 / truth.phihat(w, L, np.arange(n // 2 + 1)))[np.abs(k)]).cuda().to(rdt)
    cell_of_k = torch.from_numpy(np.where(k < 0, k + L, k)).cuda()
    return cells, wt, inv, cell_of_k


def run_case(torch, fa, truth, name, real, scale, reps):
    import numpy as np

    n, m, batch, width = CASES[name]
    batch, m = max(1, batch // scale), max(1, m // scale)
    eps = EPS[real]
    rdt, cdt = (torch.float32, torch.complex64) if real == "f32" else (torch.float64, torch.complex128)
    rng = np.random.default_rng(1)
    x1, x2 = rng.uniform(-math.pi * width, math.pi * width, m), rng.uniform(-math.pi * width, math.pi * width, m)
    c = torch.randn((batch, m), dtype=cdt, device="cuda")
    f = torch.randn((batch,) + n, dtype=cdt, device="cuda")
    oc, of = torch.empty_like(c), torch.empty_like(f)
    plans = {}
    for arm, table in (("evaluated", 0), ("tabulated", 1)):
        p = fa.Nufft2d(n, eps, real, 0)
        p.set_option("table", table)
        p.set_points(x1, x2)
        p.reserve(batch)
        plans[arm] = p
    default = fa.Nufft2d(n, eps, real, 0).describe()
    w, L1, L2 = (int(s) for s in re.match(r"nufft2d \w+: w (\d+), L (\d+) x (\d+), ", plans["evaluated"].describe()).groups())
    cells1, wt1, inv1, ck1 = caller_axis(torch, truth, x1, n[0], w, L1, rdt)
    cells2, wt2, inv2, ck2 = caller_axis(torch, truth, x2, n[1], w, L2, rdt)
    inv = inv1[:, None] * inv2[None, :]
    mode_cells = (ck1[:, None] * L2 + ck2[None, :]).reshape(-1)  # the flat cell of every mode, C order
    grid, grid2 = torch.empty((batch, L1, L2), dtype=cdt, device="cuda"), torch.empty((batch, L1, L2), dtype=cdt, device="cuda")
    flat, flat2 = grid.view(batch, L1 * L2), grid2.view(batch, L1 * L2)

    def caller1():
        grid.zero_()
        gr, cr = torch.view_as_real(flat), torch.view_as_real(c)
        for t1 in range(w):
            for t2 in range(w):
                gr.index_add_(1, cells1[:, t1] * L2 + cells2[:, t2], cr * (wt1[:, t1] * wt2[:, t2])[None, :, None])
        fa.fft2(grid, fa.Transform.Fft, out=grid2)
        torch.mul(flat2[:, mode_cells].view(batch, n[0], n[1]), inv[None], out=of)

    def caller2():
        grid.zero_()
        flat[:, mode_cells] = (f * inv[None]).view(batch, -1)
        fa.fft2(grid, fa.Transform.UnscaledIfft, out=grid2)
        oc.zero_()
        for t1 in range(w):
            for t2 in range(w):
                oc.add_(flat2[:, cells1[:, t1] * L2 + cells2[:, t2]] * (wt1[:, t1] * wt2[:, t2])[None, :])

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
        recs.append({"case": name, "real": real, "type": typ, "n_modes": list(n), "points": m, "batch": batch, "eps": eps, "w": w, "L": [L1, L2],
                     "points_within": width, "default": default, "describe": {arm: p.describe() for arm, p in plans.items()}, "ms": t,
                     "over_caller": {arm: med[arm] / med["caller"] for arm in plans},
                     "tabulated": {"over_evaluated": med["tabulated"] / med["evaluated"],
                                   "beats_evaluated_by_more_than_the_spread": med["evaluated"] - med["tabulated"] > max(wid("tabulated"), wid("evaluated"))},
                     "rel_l2_against_caller": agree})
        del ys, ref
    del c, f, oc, of, grid, grid2, flat, flat2, plans, cells1, cells2, wt1, wt2
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
