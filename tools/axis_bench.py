#!/usr/bin/env python3
"""Transforms along a strided axis (fourier_hip_transform_axis_*, fourier_amd.fft2) against the contiguous transforms of the same
bytes, on the GPU.

  python tools/axis_bench.py [--cases fft2,col_f32,col_f64,tr_4096,tr_1000] [--reps 10] [--out FILE]
      One JSON line per case, HIP-event milliseconds per call (median over alternating repetitions on shared buffers):
        fft2     f32 fft2 of [64, 2048, 2048] against the 1-D 2^22 x 64 transform (both two HBM round trips);
        col_*    the column-tile route on [256][1024][4096] against the contiguous transform of the same 1024 x (256 * 4096) rows
                 and against the forced transpose route (lib/libfourier_experiments.so, FOURIER_AXIS_ROUTE=transpose at create);
        tr_*     the transpose route at N = 4096 / 1000 on [64][N][1024] f32 against the contiguous transform of the same rows; the
                 two transposes' share is estimated as the difference, with their rate on 4 x the array's bytes (each transpose
                 reads and writes it once).  A `rocprofv3 --kernel-trace --stats` run of the same case gives the kernels' own times.
Codes: SQRT_SCALED_FFT everywhere (unitary: repeated calls on shared buffers keep the data's magnitude)."""
import argparse
import ctypes
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CODE = 3


def time_arms(torch, arms, reps, warmup=1):
    """arms: {name: callable}; alternating order, HIP events on the current stream; median ms per arm."""
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
    return {k: {"median_ms": statistics.median(v), "min_ms": min(v), "max_ms": max(v)} for k, v in ms.items()}


def forced_transpose_plan(n, real):
    """A plan of the experiments library created with FOURIER_AXIS_ROUTE=transpose."""
    import fourier_amd
    from fourier_amd import _lib, build

    prev = _lib._lib
    exp = _lib.bind(ctypes.CDLL(build.OUT_EXPERIMENTS))
    os.environ["FOURIER_AXIS_ROUTE"] = "transpose"
    try:
        _lib._lib = exp
        return fourier_amd.Fft(n, real, 0)
    finally:
        _lib._lib = prev
        del os.environ["FOURIER_AXIS_ROUTE"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default="fft2,col_f32,col_f64,tr_4096,tr_1000")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch

    import fourier_amd as fa

    lines = []
    stream = lambda: torch.cuda.current_stream().cuda_stream  # noqa: E731
    for case in args.cases.split(","):
        if case == "fft2":
            x = torch.randn(64, 2048, 2048, dtype=torch.complex64, device="cuda")
            y = torch.empty_like(x)
            p22 = fa.create_fft_f32(1 << 22, 0)
            p2k = fa.create_fft_f32(2048, 0)
            t = time_arms(torch, {"fft2": lambda: fa.fftn(x, (-2, -1), CODE, out=y),
                                  "rows_2^22": lambda: p22.transform_batch_ptr(x.data_ptr(), y.data_ptr(), 64, CODE, stream())}, args.reps)
            rec = {"case": case, "shape": [64, 2048, 2048], "real": "f32", "routes": [p2k.describe_axis(2048), p2k.describe_axis(1)],
                   "plan_2^22": p22.describe(), **{k + "_ms": v["median_ms"] for k, v in t.items()},
                   "ratio_fft2_over_rows": t["fft2"]["median_ms"] / t["rows_2^22"]["median_ms"]}
            del x, y
        elif case.startswith("col_"):
            real = case[4:]
            outer, n, inner = 256, 1024, 4096
            dt = torch.complex64 if real == "f32" else torch.complex128
            x = torch.randn(outer, n, inner, dtype=dt, device="cuda")
            y = torch.empty_like(x)
            plan = (fa.create_fft_f32 if real == "f32" else fa.create_fft_f64)(n, 0)
            forced = forced_transpose_plan(n, real)
            t = time_arms(torch, {
                "column": lambda: plan.transform_axis_ptr(x.data_ptr(), y.data_ptr(), outer, inner, CODE, stream()),
                "rows": lambda: plan.transform_batch_ptr(x.data_ptr(), y.data_ptr(), outer * inner, CODE, stream()),
                "transpose": lambda: forced.transform_axis_ptr(x.data_ptr(), y.data_ptr(), outer, inner, CODE, stream())}, args.reps)
            nbytes = 2 * x.numel() * x.element_size()
            rec = {"case": case, "shape": [outer, n, inner], "real": real, "route": plan.describe_axis(inner),
                   "forced": forced.describe_axis(inner), **{k + "_ms": v["median_ms"] for k, v in t.items()},
                   "column_tbs": nbytes / t["column"]["median_ms"] / 1e9,
                   "ratio_column_over_rows": t["column"]["median_ms"] / t["rows"]["median_ms"],
                   "ratio_transpose_over_column": t["transpose"]["median_ms"] / t["column"]["median_ms"]}
            del x, y
        elif case.startswith("tr_"):
            n = int(case[3:])
            outer, inner = 64, 1024
            x = torch.randn(outer, n, inner, dtype=torch.complex64, device="cuda")
            y = torch.empty_like(x)
            plan = fa.create_fft_f32(n, 0)
            plan.reserve_axis(outer, inner)
            t = time_arms(torch, {
                "transpose": lambda: plan.transform_axis_ptr(x.data_ptr(), y.data_ptr(), outer, inner, CODE, stream()),
                "rows": lambda: plan.transform_batch_ptr(x.data_ptr(), y.data_ptr(), outer * inner, CODE, stream())}, args.reps)
            extra = t["transpose"]["median_ms"] - t["rows"]["median_ms"]
            nbytes = x.numel() * x.element_size()
            rec = {"case": case, "shape": [outer, n, inner], "real": "f32", "route": plan.describe_axis(inner),
                   **{k + "_ms": v["median_ms"] for k, v in t.items()},
                   "ratio_transpose_over_rows": t["transpose"]["median_ms"] / t["rows"]["median_ms"],
                   "transposes_ms_est": extra, "transpose_tbs_est": 4 * nbytes / extra / 1e9 if extra > 0 else None}
            del x, y
        else:
            raise SystemExit(f"unknown case {case}")
        torch.cuda.empty_cache()
        line = json.dumps(rec)
        print(line, flush=True)
        lines.append(line)
    if args.out:
        with open(args.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
