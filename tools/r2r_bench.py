#!/usr/bin/env python3
"""DCT-II through the real-to-real handle (fourier_hip_r2r_*) against the composition a caller can write from RealFft.rfft and torch
ops, and against RealFft.rfft alone as the floor, on the GPU.

  python tools/r2r_bench.py [--cases d32_20,d32_14,...] [--reps 5] [--out FILE]
      One JSON line per case: HIP-event milliseconds per call (median / min / max over alternating repetitions on shared buffers) of
      three arms
        handle       R2R.transform_batch_ptr, DCT-II, backward norm
        composition  torch index permutation (two strided copies), RealFft.rfft, torch multiply by exp(-i pi k / 2N), real and
                     imaginary parts into the output -- what the public interface offered before the handle
        rfft         RealFft.rfft of the same rows alone
      the ratio handle / composition with the composition arm's own spread (max - min) / median, the ratio handle / rfft, the same
      for DCT-III (handle only: "handle_dct3"), and the relative L2 difference of the two DCT-II results.
  python tools/r2r_bench.py --kernel-stats DIR --cases C
      Reads the kernel trace a `rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/r2r_bench.py --cases C --reps R` run left and
      reports the total time of r2r_pack_kernel, r2r_post_kernel, r2r_pre_kernel, r2r_unpack_kernel and real_post_kernel and their
      rate on the bytes their grids move."""
import argparse
import csv
import glob
import json
import math
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

# key: (precision, N, batch)
CASES = {"d32_20": ("f32", 1 << 20, 4096), "d32_14": ("f32", 1 << 14, 262144), "d32_1000": ("f32", 1000, 1 << 20),
         "d64_20": ("f64", 1 << 20, 2048), "d64_14": ("f64", 1 << 14, 131072), "d64_1000": ("f64", 1000, 1 << 19)}


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


def run_case(torch, fa, key, reps):
    real, n, batch = CASES[key]
    rdt = torch.float32 if real == "f32" else torch.float64
    cdt = torch.complex64 if real == "f32" else torch.complex128
    h = n // 2
    x = torch.randn(batch, n, dtype=rdt, device="cuda")
    y = torch.empty_like(x)
    y2 = torch.empty_like(x)
    v = torch.empty_like(x)
    spec = torch.empty(batch, h + 1, dtype=cdt, device="cuda")
    k = torch.arange(h + 1, device="cuda", dtype=torch.float64)
    c2 = (2 * torch.polar(torch.ones_like(k), -math.pi * k / (2 * n))).to(cdt)
    plan = fa.R2R(n, real, 0)
    rp = fa.RealFft(n, real, 0)
    plan.reserve(batch)
    rp.reserve(batch)
    st = torch.cuda.current_stream().cuda_stream

    def handle():
        plan.transform_batch_ptr(x.data_ptr(), y.data_ptr(), batch, 0, 0, st)

    def handle_dct3():
        plan.transform_batch_ptr(x.data_ptr(), y2.data_ptr(), batch, 1, 0, st)

    def composition():
        v[:, :n - h].copy_(x[:, 0::2])
        v[:, n - h:].copy_(x[:, 1::2].flip(-1))
        rp.forward_batch_ptr(v.data_ptr(), spec.data_ptr(), batch, fa.Transform.Fft, st)
        spec.mul_(c2)
        y2[:, :h + 1].copy_(spec.real)
        torch.neg(spec.imag[:, 1:h].flip(-1), out=y2[:, h + 1:])

    def rfft():
        rp.forward_batch_ptr(x.data_ptr(), spec.data_ptr(), batch, fa.Transform.Fft, st)

    handle()
    composition()
    sl = slice(0, max(1, min(batch, (1 << 22) // n)))
    diff = (torch.linalg.norm((y[sl] - y2[sl]).double()) / torch.linalg.norm(y2[sl].double())).item()
    t = time_arms(torch, {"handle": handle, "composition": composition, "rfft": rfft, "handle_dct3": handle_dct3}, reps)
    med = {a: r["median_ms"] for a, r in t.items()}
    rec = {"case": key, "real": real, "n": n, "batch": batch, "describe": plan.describe(), "describe_rfft": rp.describe(), "ms": t,
           "handle_over_composition": med["handle"] / med["composition"],
           "composition_spread": (t["composition"]["max_ms"] - t["composition"]["min_ms"]) / med["composition"],
           "handle_over_rfft": med["handle"] / med["rfft"], "handle_dct3_over_rfft": med["handle_dct3"] / med["rfft"],
           "rel_l2_handle_vs_composition": diff}
    del x, y, y2, v, spec, plan, rp
    torch.cuda.empty_cache()
    return rec


def kernel_stats(trace_dir, key):
    """Time and rate of the sweeps over EVERY dispatch of a traced run.  The bytes of a dispatch follow from its grid (work-items, the
    trace's Grid_Size): a lane of each of the four r2r sweeps moves four reals one way and two complex values the other, a lane of
    real_post_kernel two complex values each way -- eight reals per lane in every case.  The tables are not counted."""
    files = glob.glob(os.path.join(trace_dir, "**", "*kernel_trace.csv"), recursive=True)
    if not files:
        raise SystemExit(f"no *kernel_trace.csv under {trace_dir}")
    per_item = 8 * (4 if CASES[key][0] == "f32" else 8)
    names = ("r2r_pack_kernel", "r2r_post_kernel", "r2r_pre_kernel", "r2r_unpack_kernel", "real_post_kernel")
    tot = {k: [0.0, 0, 0] for k in names}
    for f in files:
        with open(f) as fh:
            for row in csv.DictReader(fh):
                name = row.get("Kernel_Name", "")
                for k in tot:
                    if k in name:
                        tot[k][0] += (int(row["End_Timestamp"]) - int(row["Start_Timestamp"])) * 1e-6
                        tot[k][1] += 1
                        tot[k][2] += int(row.get("Grid_Size") or row.get("Grid_Size_X") or 0) * per_item
    out = {"case": key, "source": "rocprofv3 --kernel-trace", "table_bytes_counted": False}
    for k, (ms, cnt, nbytes) in tot.items():
        out[k] = {"dispatches": cnt, "ms_total": ms, "bytes_total": nbytes, "tbs": nbytes / (ms * 1e-3) / 1e12 if ms > 0 and nbytes else None}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default=",".join(CASES))
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
            recs.append(run_case(torch, fourier_amd, k, args.reps))
            print(json.dumps(recs[-1]), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as f:
            for r in recs:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
