#!/usr/bin/env python3
"""Linear convolution with a prepared filter bank (fourier_hip_lconv_*) against what a caller wrote before the handle and against
its own padded route, on the GPU.

  python tools/lconv_bench.py [--cases c32,r32,c64,short] [--taps 17,129,1025,8193] [--reps 5] [--sweep] [--out FILE]
      One JSON line per case and tap count: HIP-event milliseconds per call (median / min / max over alternating repetitions on
      shared buffers) of the arms
        handle   LinearConv.apply on its default route
        caller   torch.nn.functional.pad to M = the smallest power of two >= Lx + K - 1, FftConv(M).apply in place, a slice copy
        padded   the handle with "overlap_save" = 0 (only where the default route is the overlap-save one)
      every arm's spread (max - min) / median, the ratios, and every arm's rate on the algorithmic bytes (Lx + Lout) values per row.
      --sweep adds one line per forced block 2^11 ... 2^15 of the handle (median / min / max) beside the rule's choice."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

# key: (precision, real data, Lx, batch); the mode is "same"
CASES = {"c32": ("f32", False, 1 << 20, 128), "r32": ("f32", True, 1 << 20, 128), "c64": ("f64", False, 1 << 20, 64),
         "short": ("f32", False, 4096, 1 << 16)}


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


def run_case(torch, fa, key, k, reps, sweep):
    real, real_data, lx, batch = CASES[key]
    rdt, cdt = (torch.float32, torch.complex64) if real == "f32" else (torch.float64, torch.complex128)
    dt = rdt if real_data else cdt
    val = torch.empty(0, dtype=dt).element_size()
    x = torch.empty(batch, lx, dtype=dt, device="cuda")
    x.normal_() if real_data else torch.view_as_real(x).normal_()
    taps = torch.zeros(1, k, dtype=dt, device="cuda")
    taps[:, 0] = 1
    taps[:, 1:] = 1e-3
    handle = fa.LinearConv(lx, k, real, "same", real_data, 0)
    handle.set_filters(taps)
    handle.reserve(batch)
    y = torch.empty(batch, handle.out_length(), dtype=dt, device="cuda")
    m = 1
    while m < lx + k - 1:
        m *= 2
    circ = fa.FftConv(m, real, real_data, 0)
    circ.set_filters(taps)
    circ.reserve(batch)
    off = (k - 1) // 2

    def caller():
        z = torch.nn.functional.pad(x, (0, m - lx))
        circ.apply(z, out=z)
        y.copy_(z[:, off:off + lx])

    arms = {"handle": lambda: handle.apply(x, out=y), "caller": caller}
    padded = None
    if handle.describe().startswith("lconv overlap-save"):
        padded = fa.LinearConv(lx, k, real, "same", real_data, 0)
        padded.set_option("overlap_save", 0)
        padded.set_filters(taps)
        padded.reserve(batch)
        arms["padded"] = lambda: padded.apply(x, out=y)
    t = time_arms(torch, arms, reps)
    nbytes = batch * (lx + handle.out_length()) * val
    med = {a: v["median_ms"] for a, v in t.items()}
    recs = [{"case": key, "real": real, "real_data": real_data, "lx": lx, "taps": k, "batch": batch, "mode": "same",
             "describe": handle.describe(), "describe_caller": circ.describe(), "describe_padded": padded.describe() if padded else None,
             "ms": t, "handle_over_caller": med["handle"] / med["caller"],
             "handle_over_padded": med["handle"] / med["padded"] if padded else None,
             "algorithmic_bytes": nbytes, "tbs_on_algorithmic_bytes": {a: nbytes / (v * 1e-3) / 1e12 for a, v in med.items()}}]
    if sweep and padded is not None:
        blocks = {}
        for v in range(11, 16):
            p = fa.LinearConv(lx, k, real, "same", real_data, 0)
            try:
                p.set_option("block", v)
            except fa.FourierError:
                continue
            p.set_filters(taps)
            blocks[str(1 << v)] = (lambda q: (lambda: q.apply(x, out=y)))(p)
        if blocks:
            recs.append({"case": key, "taps": k, "sweep": True, "rule": handle.describe(), "ms": time_arms(torch, blocks, reps)})
    del x, y, handle, circ, padded, arms
    torch.cuda.empty_cache()
    return recs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default=",".join(CASES))
    ap.add_argument("--taps", default="17,129,1025,8193")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--sweep", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch

    if not torch.cuda.is_available():
        raise SystemExit("needs a GPU")
    import fourier_amd

    recs = []
    for key in [c for c in args.cases.split(",") if c]:
        for k in ([129] if key == "short" else [int(v) for v in args.taps.split(",") if v]):
            for r in run_case(torch, fourier_amd, key, k, args.reps, args.sweep):
                recs.append(r)
                print(json.dumps(r), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as f:
            for r in recs:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
