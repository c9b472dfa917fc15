#!/usr/bin/env python3
"""Convolution with a prepared filter bank (fourier_hip_conv_*) against its own composed route and against the composition a
caller can write from the transforms alone, on the GPU.

  python tools/conv_bench.py [--cases c32_20,r32_20,...] [--filters 1,64] [--reps 5] [--out FILE]
      One JSON line per case and filter count: HIP-event milliseconds per call (median / min / max over alternating repetitions on
      shared buffers) of three arms
        fused     the handle with "fusion" = 1 (its default route)
        composed  the same handle with "fusion" = 0
        api       Fft.transform forward, an in-place torch multiply by the spectrum, Fft.transform unscaled inverse
                  (real data: RealFft.rfft, multiply, RealFft.irfft) -- what the public interface offered before the handle
      the ratio fused / composed with the composed arm's own spread (max - min) / median, the ratio fused / api, and the rate of
      every arm on the algorithmic bytes of the fused route's model (rows in, rows out and the intermediates of the route; the
      bank's bytes are NOT counted: `bank_bytes_counted` in the record).
  python tools/conv_bench.py --kernel-stats DIR --cases C --filters F --reps R
      Reads the kernel trace a `rocprofv3 --kernel-trace --stats -d DIR -- python tools/conv_bench.py --cases C --filters F --reps R`
      run left and reports the total time of conv_mul_kernel, real_conv_mid_kernel, fft_conv_kernel, real_post_kernel and
      real_pre_kernel and their rate on the bytes their grids move."""
import argparse
import csv
import glob
import json
import os
import re
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

# key: (precision, real data, N, batch)
CASES = {"c32_20": ("f32", False, 1 << 20, 4096), "r32_20": ("f32", True, 1 << 20, 4096),
         "c64_20": ("f64", False, 1 << 20, 4096), "r64_20": ("f64", True, 1 << 20, 2048),
         "c32_14": ("f32", False, 1 << 14, 262144), "c32_12": ("f32", False, 1 << 12, 1 << 20)}


def passes_of(describe):
    """HBM round trips of the plan a describe string names: "1024x512" = 2, "128x128 one-launch" = 1, anything else 1."""
    m = re.search(r"(\d+(?:x\d+)+)( one-launch)?", describe)
    return 1 if not m or m.group(2) else m.group(1).count("x") + 1


def model_bytes(real, real_data, n, batch, describe):
    """Algorithmic bytes of one apply on the route `describe` names, the bank not counted."""
    e = 8 if real == "f32" else 16
    p = passes_of(describe)
    if real_data:
        h = n // 2
        if "fused untangle" in describe:  # inner plan forward, the mid sweep, inner plan inverse
            return batch * h * e * (2 * p + 2 + 2 * p)
        return batch * e * (4 * p * h + 2 * (2 * h + 1) + 2 * (h + 1))  # ... untangle, product sweep, retangle in between
    if "one-launch" in describe and describe.startswith("conv one-launch"):
        return batch * n * e * 2
    if "fused passes" in describe:
        return batch * n * e * (4 * p - 2)  # the conv kernel is the last forward and the first inverse pass
    return batch * n * e * (4 * p + 2)


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
    return {k: {"median_ms": statistics.median(v), "min_ms": min(v), "max_ms": max(v)} for k, v in ms.items()}


def run_case(torch, fa, key, filters, reps):
    real, real_data, n, batch = CASES[key]
    rdt = torch.float32 if real == "f32" else torch.float64
    cdt = torch.complex64 if real == "f32" else torch.complex128
    dt = rdt if real_data else cdt
    x = torch.empty(batch, n, dtype=dt, device="cuda")
    y = torch.empty_like(x)
    torch.view_as_real(x).normal_() if not real_data else x.normal_()
    taps = torch.zeros(filters, 129, dtype=dt, device="cuda")
    taps[:, 0] = 1  # an impulse plus a little: repeated calls on shared buffers keep the data's magnitude
    taps[:, 1:] = 1e-3
    fused = fa.FftConv(n, real, real_data, 0)
    composed = fa.FftConv(n, real, real_data, 0)
    composed.set_option("fusion", 0)
    for p in (fused, composed):
        p.set_filters(taps)
        p.reserve(batch)
    # the public interface without the handle: whole-batch spectra, one torch multiply
    if real_data:
        rp = fa.RealFft(n, real, 0)
        rp.reserve(batch)
        H = rp.rfft(torch.nn.functional.pad(taps, (0, n - taps.shape[1])))
        spec = torch.empty(batch, n // 2 + 1, dtype=cdt, device="cuda")
        st = torch.cuda.current_stream().cuda_stream
        sv = spec.view(batch // filters, filters, n // 2 + 1)  # row b = i * F + f takes filter f

        def api():
            rp.forward_batch_ptr(x.data_ptr(), spec.data_ptr(), batch, fa.Transform.Fft, st)
            sv.mul_(H)
            rp.inverse_batch_ptr(spec.data_ptr(), y.data_ptr(), batch, fa.Transform.Ifft, st)
    else:
        cp = fa.Fft(n, real, 0)
        cp.reserve(batch)
        H = torch.zeros(filters, n, dtype=cdt, device="cuda")
        H[:, :taps.shape[1]] = taps
        cp.transform(H, H, fa.Transform.Fft)
        yv = y.view(batch // filters, filters, n)  # row b = i * F + f takes filter f

        def api():
            cp.transform(x, y, fa.Transform.Fft)
            yv.mul_(H)
            cp.transform(y, y, fa.Transform.Ifft)
    arms = {"fused": lambda: fused.apply(x, out=y), "composed": lambda: composed.apply(x, out=y), "api": api}
    t = time_arms(torch, arms, reps)
    mb = model_bytes(real, real_data, n, batch, fused.describe())
    med = {k: v["median_ms"] for k, v in t.items()}
    rec = {"case": key, "real": real, "real_data": real_data, "n": n, "batch": batch, "filters": filters,
           "describe_fused": fused.describe(), "describe_composed": composed.describe(), "ms": t,
           "fused_over_composed": med["fused"] / med["composed"],
           "composed_spread": (t["composed"]["max_ms"] - t["composed"]["min_ms"]) / med["composed"],
           "fused_over_api": med["fused"] / med["api"], "composed_over_api": med["composed"] / med["api"],
           "model_bytes_fused_route": mb, "bank_bytes_counted": False,
           "tbs_on_model_bytes": {k: mb / (v * 1e-3) / 1e12 for k, v in med.items()}}
    del x, y, H, fused, composed
    torch.cuda.empty_cache()
    return rec


def kernel_stats(trace_dir, key):
    """Time and rate of the convolution kernels over EVERY dispatch of a traced run.  The bytes of a dispatch follow from its grid
    (work-items, the trace's Grid_Size): the sweeps run one lane per element (conv_mul_kernel: read + write one complex value) or per
    mirrored pair (real_conv_mid_kernel, real_post_kernel, real_pre_kernel: two values read, two written); a thread of fft_conv_kernel
    holds 16 units of 16 bytes, read once and written once.  The bank and the twiddles are not counted."""
    files = glob.glob(os.path.join(trace_dir, "**", "*kernel_trace.csv"), recursive=True)
    if not files:
        raise SystemExit(f"no *kernel_trace.csv under {trace_dir}")
    real = CASES[key][0]
    e = 8 if real == "f32" else 16
    per_item = {"conv_mul_kernel": 2 * e, "real_conv_mid_kernel": 4 * e, "fft_conv_kernel": 2 * 16 * 16, "real_post_kernel": 4 * e,
                "real_pre_kernel": 4 * e}
    tot = {k: [0.0, 0, 0] for k in per_item}
    for f in files:
        with open(f) as fh:
            for row in csv.DictReader(fh):
                name = row.get("Kernel_Name", "")
                for k in tot:
                    if k in name:
                        tot[k][0] += (int(row["End_Timestamp"]) - int(row["Start_Timestamp"])) * 1e-6
                        tot[k][1] += 1
                        tot[k][2] += int(row.get("Grid_Size") or row.get("Grid_Size_X") or 0) * per_item[k]
    out = {"case": key, "source": "rocprofv3 --kernel-trace", "bank_bytes_counted": False}
    for k, (ms, cnt, nbytes) in tot.items():
        out[k] = {"dispatches": cnt, "ms_total": ms, "bytes_total": nbytes, "tbs": nbytes / (ms * 1e-3) / 1e12 if ms > 0 and nbytes else None}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default=",".join(CASES))
    ap.add_argument("--filters", default="1,64")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--kernel-stats", default=None, metavar="DIR")
    args = ap.parse_args()
    keys = [k for k in args.cases.split(",") if k]
    recs = []
    if args.kernel_stats:
        recs.append(kernel_stats(args.kernel_stats, keys[0]))
        print(json.dumps(recs[-1]))
    else:
        import torch

        if not torch.cuda.is_available():
            raise SystemExit("needs a GPU")
        import fourier_amd

        for k in keys:
            for f in [int(v) for v in args.filters.split(",") if v]:
                recs.append(run_case(torch, fourier_amd, k, f, args.reps))
                print(json.dumps(recs[-1]), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as f:
            for r in recs:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
