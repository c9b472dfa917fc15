#!/usr/bin/env python3
"""Real-input transforms (fourier_hip_real_*) against the complex transform of the same N and the complex N/2 plan, on the GPU.

  python tools/real_fft_bench.py [--cases f32_20,f64_20,f32_22] [--reps 10] [--no-cap-ab] [--out FILE]
      One JSON line per case: HIP-event milliseconds per call (median over alternating repetitions on shared buffers) of
      r2c, c2r, the complex N transform and the complex N/2 plan, the ratios r2c / complex N, and the untangle sweep's time
      estimated as r2c - complex N/2 (and c2r - complex N/2) with its rate on the algorithmic bytes (read N/2, write N/2+1
      complex per row).  Then, unless --no-cap-ab, the scratch-bound A/B at f32 N = 2^20 x 4096: 1 GiB (the default) against
      256 MiB against the whole batch, through lib/libfourier_experiments.so (FOURIER_REAL_SCRATCH_BYTES, read at create).
  python tools/real_fft_bench.py --kernel-stats DIR --cases ... --reps R
      Reads the kernel trace a `rocprofv3 --kernel-trace --stats -d DIR -- python tools/real_fft_bench.py --no-cap-ab --cases C
      --reps R` run left and reports real_post_kernel / real_pre_kernel time per call and their rate on the algorithmic bytes.

Codes: the unitary pair (SQRT_SCALED_FFT / SQRT_SCALED_IFFT) everywhere, so that repeated calls on shared buffers keep the data's
magnitude; the scale is one multiply in the last store of every route and costs nothing measurable."""
import argparse
import csv
import glob
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CASES = {"f32_20": ("f32", 1 << 20, 4096), "f64_20": ("f64", 1 << 20, 4096), "f32_22": ("f32", 1 << 22, 1024)}
PEAK_TBS = 8.0


def untangle_bytes(real, n, batch):
    e = 8 if real == "f32" else 16
    return batch * (n // 2 + n // 2 + 1) * e


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


def buffers(torch, real, n, batch):
    dt = torch.float32 if real == "f32" else torch.float64
    a = torch.empty(batch * n * 2, dtype=dt, device="cuda")
    b = torch.empty_like(a)
    a.normal_()
    b.normal_()
    return a, b


def run_case(torch, fa, key, reps):
    real, n, batch = CASES[key]
    a, b = buffers(torch, real, n, batch)
    rp = (fa.create_rfft_f32 if real == "f32" else fa.create_rfft_f64)(n, 0)
    mk = fa.create_fft_f32 if real == "f32" else fa.create_fft_f64
    cn, ch = mk(n, 0), mk(n // 2, 0)
    rp.reserve(batch)
    st = torch.cuda.current_stream().cuda_stream
    arms = {
        "r2c": lambda: rp.forward_batch_ptr(a.data_ptr(), b.data_ptr(), batch, fa.Transform.SqrtScaledFft, st),
        "c2r": lambda: rp.inverse_batch_ptr(b.data_ptr(), a.data_ptr(), batch, fa.Transform.SqrtScaledIfft, st),
        "complex_n": lambda: cn.transform_batch_ptr(a.data_ptr(), b.data_ptr(), batch, fa.Transform.SqrtScaledFft, st),
        "complex_half": lambda: ch.transform_batch_ptr(a.data_ptr(), b.data_ptr(), batch, fa.Transform.SqrtScaledFft, st),
    }
    t = time_arms(torch, arms, reps)
    ub = untangle_bytes(real, n, batch)
    rec = {"case": key, "real": real, "n": n, "batch": batch, "describe": rp.describe(), "ms": t,
           "r2c_over_complex_n": t["r2c"]["median_ms"] / t["complex_n"]["median_ms"],
           "c2r_over_complex_n": t["c2r"]["median_ms"] / t["complex_n"]["median_ms"],
           "untangle_bytes_per_call": ub}
    for arm in ("r2c", "c2r"):
        d = t[arm]["median_ms"] - t["complex_half"]["median_ms"]
        rec[f"{arm}_minus_half_ms"] = d
        rec[f"{arm}_untangle_tbs_est"] = ub / (d * 1e-3) / 1e12 if d > 0 else None
    del a, b
    torch.cuda.empty_cache()
    return rec


def cap_ab(torch, reps):
    """Scratch bound A/B through the experiments library (FOURIER_REAL_SCRATCH_BYTES, read at create)."""
    import ctypes

    import fourier_amd
    from fourier_amd import _lib, build

    real, n, batch = CASES["f32_20"]
    prev = _lib._lib
    _lib._lib = _lib.bind(ctypes.CDLL(build.OUT_EXPERIMENTS))
    try:
        a, b = buffers(torch, real, n, batch)
        st = torch.cuda.current_stream().cuda_stream
        caps = {"1GiB": 1 << 30, "256MiB": 256 << 20, "whole_batch": 1 << 50}
        plans = {}
        for name, cap in caps.items():
            os.environ["FOURIER_REAL_SCRATCH_BYTES"] = str(cap)
            plans[name] = fourier_amd.create_rfft_f32(n, 0)
            plans[name].reserve(batch)
        os.environ.pop("FOURIER_REAL_SCRATCH_BYTES")
        arms = {}
        for name, p in plans.items():
            arms[f"r2c_{name}"] = (lambda p=p: p.forward_batch_ptr(a.data_ptr(), b.data_ptr(), batch, fourier_amd.Transform.SqrtScaledFft, st))
            arms[f"c2r_{name}"] = (lambda p=p: p.inverse_batch_ptr(b.data_ptr(), a.data_ptr(), batch, fourier_amd.Transform.SqrtScaledIfft, st))
        t = time_arms(torch, arms, reps)
        del plans, a, b
        torch.cuda.empty_cache()
        return {"case": "scratch_cap_ab", "real": real, "n": n, "batch": batch, "ms": t}
    finally:
        _lib._lib = prev


def kernel_stats(trace_dir, keys, calls):
    """Per-call time of the untangle kernels from a rocprofv3 kernel trace (one case per trace directory)."""
    files = glob.glob(os.path.join(trace_dir, "**", "*kernel_trace.csv"), recursive=True)
    if not files:
        raise SystemExit(f"no *kernel_trace.csv under {trace_dir}")
    real, n, batch = CASES[keys[0]]
    tot = {"real_post_kernel": [0.0, 0], "real_pre_kernel": [0.0, 0]}
    for f in files:
        with open(f) as fh:
            for row in csv.DictReader(fh):
                name = row.get("Kernel_Name", "")
                for k in tot:
                    if k in name:
                        tot[k][0] += (int(row["End_Timestamp"]) - int(row["Start_Timestamp"])) * 1e-6
                        tot[k][1] += 1
    ub = untangle_bytes(real, n, batch)
    out = {"case": keys[0], "source": "rocprofv3 --kernel-trace", "calls_per_arm": calls, "untangle_bytes_per_call": ub}
    for k, (ms, cnt) in tot.items():
        per = ms / calls if calls else 0.0
        out[k] = {"dispatches": cnt, "ms_per_call": per, "tbs": ub / (per * 1e-3) / 1e12 if per > 0 else None,
                  "frac_of_peak": (ub / (per * 1e-3) / 1e12) / PEAK_TBS if per > 0 else None}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default="f32_20,f64_20,f32_22")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--no-cap-ab", action="store_true")
    ap.add_argument("--out", default=None)
    ap.add_argument("--kernel-stats", default=None, metavar="DIR")
    args = ap.parse_args()
    keys = [k for k in args.cases.split(",") if k]
    recs = []
    if args.kernel_stats:
        recs.append(kernel_stats(args.kernel_stats, keys, 1 + args.reps))
    else:
        import torch

        if not torch.cuda.is_available():
            raise SystemExit("needs a GPU")
        import fourier_amd

        for k in keys:
            recs.append(run_case(torch, fourier_amd, k, args.reps))
            print(json.dumps(recs[-1]), flush=True)
        if not args.no_cap_ab:
            recs.append(cap_ab(torch, args.reps))
            print(json.dumps(recs[-1]), flush=True)
    if args.kernel_stats:
        print(json.dumps(recs[-1]))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as f:
            for r in recs:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
