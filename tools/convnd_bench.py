#!/usr/bin/env python3
"""The N-D convolution handle (fourier_hip_convnd_*) on its two routes against what a caller wrote before it, on the GPU.

  python tools/convnd_bench.py [--cases circular:f32,circular:f64,same:f32,same:f64,volume:f32] [--scale 1] [--reps 5] [--out FILE]
      One JSON line per case:
        circular  one filter of 31 x 31 taps over items of [2048, 2048]: 64 items at f32, 32 at f64
        same      scipy's "same" of 2000 x 2000 images with 31 x 31 taps (transform shape next_fast_len, [2048, 2048]): 64 / 32 images
        volume    one filter of 5 x 5 x 5 taps over 8 items of [256, 256, 256], f32
      (--scale divides the item counts, for a quick look.)  HIP-event milliseconds per call (median / min / max over alternating
      repetitions on shared buffers, one process) of the arms
        fused     FftConvNd.apply, "fusion" = 1
        composed  the same with "fusion" = 0
        caller    fourier_amd.rfft2 / rfftn of the items, a torch multiply with a prepared spectrum in place, irfft2 / irfftn; for the
                  "same" case a copy into a zeroed padded buffer in front and a slice copy behind
      every arm's spread (max - min) / median, every handle arm over the caller arm, the fused arm over the composed one and whether it
      beats it by more than the larger of the two arms' widths (the rule the default follows), and the byte model:
      40 N fused against 56 N composed per item of N f32 reals, windows not counted."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CASES = {"circular": ((2048, 2048), (31, 31), {"f32": 64, "f64": 32}, False),
         "same": ((2000, 2000), (31, 31), {"f32": 64, "f64": 32}, True),
         "volume": ((256, 256, 256), (5, 5, 5), {"f32": 8}, False)}


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


def run_case(torch, fa, name, real, scale, reps):
    a, k, counts, linear = CASES[name]
    rdt = torch.float32 if real == "f32" else torch.float64
    r = len(a)
    batch = max(1, counts[real] // scale)
    if linear:
        shape = tuple(fa.next_fast_len(n + m - 1, even=(d == r - 1)) for d, (n, m) in enumerate(zip(a, k)))
        first, size = tuple((m - 1) // 2 for m in k), a
    else:
        shape, first, size = a, (0,) * r, a
    x = torch.randn((batch,) + a, dtype=rdt, device="cuda")
    h = torch.randn((1,) + k, dtype=rdt, device="cuda")
    out = torch.empty((batch,) + size, dtype=rdt, device="cuda")
    plans = {}
    for arm, fusion in (("fused", 1), ("composed", 0)):
        p = fa.FftConvNd(shape, real, 0)
        p.set_option("fusion", fusion)
        p.set_window(a, first, size)
        p.set_filters(h)
        p.reserve(batch)
        plans[arm] = p
    default = fa.FftConvNd(shape, real, 0).describe()
    if not plans["fused"].describe().startswith("convnd fused"):
        del plans["fused"]
    dims = tuple(range(-r, 0))
    hp = torch.zeros((1,) + shape, dtype=rdt, device="cuda")
    hp[(slice(None),) + tuple(slice(0, m) for m in k)] = h
    Hs = fa.rfftn(hp, dims)  # the prepared spectrum; irfftn carries the 1/P
    px = torch.zeros((batch,) + shape, dtype=rdt, device="cuda") if linear else None
    py = torch.empty((batch,) + shape, dtype=rdt, device="cuda") if linear else None
    X = torch.empty((batch,) + shape[:-1] + (shape[-1] // 2 + 1,), dtype=Hs.dtype, device="cuda")
    window = (slice(None),) + tuple(slice(f, f + n) for f, n in zip(first, size))
    inside = (slice(None),) + tuple(slice(0, n) for n in a)

    def caller():
        if linear:
            px[inside].copy_(x)
        fa.rfftn(px if linear else x, dims, out=X)
        torch.mul(X, Hs, out=X)
        fa.irfftn(X, dims, n=shape[-1], out=py if linear else out)
        if linear:
            out.copy_(py[window])

    arms = {arm: (lambda p: (lambda: p.apply(x, out=out)))(p) for arm, p in plans.items()}
    arms["caller"] = caller
    t = time_arms(torch, arms, reps)
    med = {arm: v["median_ms"] for arm, v in t.items()}
    width = lambda arm: t[arm]["max_ms"] - t[arm]["min_ms"]  # noqa: E731
    fused = None
    if "fused" in plans:
        fused = {"over_composed": med["fused"] / med["composed"],
                 "beats_composed_by_more_than_the_spread": med["composed"] - med["fused"] > max(width("fused"), width("composed"))}
    # the arms agree (the last repetition's outputs)
    ys = {}
    for arm, f in arms.items():
        f()
        ys[arm] = out.clone()
    ref = ys["caller"].double()
    agree = {arm: float(((ys[arm].double() - ref).norm() / ref.norm()).item()) for arm in plans}
    rec = {"case": name, "real": real, "items": list(a), "taps": list(k), "transform_shape": list(shape), "window_first": list(first),
           "batch": batch, "input_bytes": x.numel() * x.element_size(), "default": default,
           "describe": {arm: p.describe() for arm, p in plans.items()}, "ms": t,
           "over_caller": {arm: med[arm] / med["caller"] for arm in plans}, "fused": fused, "rel_l2_against_caller": agree,
           "byte_model_bytes_per_f32_real": {"fused": 40, "composed": 56, "caller": 56}}
    del x, out, px, py, X, plans, arms, ys, ref
    torch.cuda.empty_cache()
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default="circular:f32,circular:f64,same:f32,same:f64,volume:f32")
    ap.add_argument("--scale", type=int, default=1)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch

    if not torch.cuda.is_available():
        raise SystemExit("needs a GPU")
    import fourier_amd

    recs = []
    for case in [s for s in args.cases.split(",") if s]:
        name, real = case.split(":")
        r = run_case(torch, fourier_amd, name, real, args.scale, args.reps)
        recs.append(r)
        print(json.dumps(r), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as f:
            for r in recs:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
