#!/usr/bin/env python3
"""The polyphase filter bank handle (fourier_hip_pfb_*): its fused route against its composed route and what a caller wrote before it,
on the GPU.

  python tools/pfb_bench.py [--shapes f32:c:256:4:256,...] [--length 1048576] [--batch 64] [--reps 5] [--out FILE]
      One JSON line per shape (precision : c|r for complex | real rows : P : T : D): `batch` rows of `length` values under the
      sinc-Hamming prototype (pfb_prototype).  The default shapes are f32 and f64, complex and real rows, P in {256, 1024} where the
      kind has a fused kernel, T in {4, 8}, D = P and 3 P / 4.  HIP-event milliseconds per call (median / min / max over alternating
      repetitions on shared buffers, one process) of the arms
        fused     Pfb.forward, "fusion" = 1
        composed  the same with "fusion" = 0
        caller    torch: unfold x filter into a materialised (batch, frames, P T) array, reshape-sum over the taps, then
                  Fft.transform_batch / RealFft.rfft of P points (preallocated buffers throughout)
      every arm's spread (max - min) / median, each handle arm over the caller's, the fused arm over the composed one and whether it
      beats it by more than the larger of the two arms' spreads (the rule the default follows: at EVERY measured shape of a precision
      and input kind), and TB/s of every arm on the ALGORITHMIC bytes: the signal in once, the channels out once.
  A shape is one step: run each group under its own time limit, e.g.  timeout -k 10 300 python tools/pfb_bench.py --shapes ... --out ..."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def default_shapes():
    shapes = []
    for real in ("f32", "f64"):
        for kind in ("c", "r"):
            for P in (256, 1024):
                if kind == "c" and P == 1024 and real == "f64":
                    continue  # the 1024-point f64 plan is a one-launch 32 x 32 plan: no whole-row kernel, no fused route
                for T in (4, 8):
                    for D in (P, 3 * P // 4):
                        shapes.append(f"{real}:{kind}:{P}:{T}:{D}")
    return ",".join(shapes)


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


def run_case(torch, fa, real, real_input, P, T, D, length, batch, reps):
    rdt, cdt = (torch.float32, torch.complex64) if real == "f32" else (torch.float64, torch.complex128)
    es = 8 if real == "f32" else 16
    if real_input:
        x = torch.randn(batch, length, dtype=rdt, device="cuda")
    else:
        x = torch.view_as_complex(torch.randn(batch, length, 2, dtype=rdt, device="cuda"))
    h = fa.pfb_prototype(P, T, rdt).cuda()
    plans = {}
    for arm, fusion in (("fused", 1), ("composed", 0)):
        p = fa.Pfb(P, T, real, D, real_input, 0)
        p.set_option("fusion", fusion)
        p.set_filter(h)
        p.reserve(length, batch)
        plans[arm] = p
    default = fa.Pfb(P, T, real, D, real_input, 0).describe()
    if plans["fused"].describe() == plans["composed"].describe():
        del plans["fused"]
    nf, bins = plans["composed"].frames(length), plans["composed"].bins()
    out = torch.empty(batch, nf, bins, dtype=cdt, device="cuda")
    # the caller's composition: the materialised frame tensor is T times the signal
    work = torch.empty(batch, nf, P * T, dtype=x.dtype, device="cuda")
    u = torch.empty(batch, nf, P, dtype=x.dtype, device="cuda")
    inner = fa.RealFft(P, real, 0) if real_input else fa.Fft(P, real, 0)
    inner.reserve(batch * nf)
    stream = torch.cuda.current_stream().cuda_stream

    def caller():
        torch.mul(x.unfold(-1, P * T, D), h, out=work)
        torch.sum(work.view(batch, nf, T, P), dim=2, out=u)
        if real_input:
            inner.forward_batch_ptr(u.data_ptr(), out.data_ptr(), batch * nf, fa.Transform.Fft, stream)
        else:
            inner.transform_batch_ptr(u.data_ptr(), out.data_ptr(), batch * nf, fa.Transform.Fft, stream)

    arms = {arm: (lambda p: (lambda: p.forward(x, out=out)))(p) for arm, p in plans.items()}
    arms["caller"] = caller
    # the arms agree before they are timed
    ref = plans["composed"].forward(x[:2]).clone()
    caller()
    agree = {"caller": float((out[:2] - ref).norm() / ref.norm())}
    if "fused" in plans:
        agree["fused"] = float((plans["fused"].forward(x[:2]) - ref).norm() / ref.norm())
    t = time_arms(torch, arms, reps)
    med = {a: v["median_ms"] for a, v in t.items()}
    width = lambda a: t[a]["max_ms"] - t[a]["min_ms"]  # noqa: E731
    fused = None
    if "fused" in plans:
        fused = {"over_composed": med["fused"] / med["composed"],
                 "beats_composed_by_more_than_the_spread": med["composed"] - med["fused"] > max(width("fused"), width("composed"))}
    bytes_in = batch * length * (es // 2 if real_input else es)
    bytes_out = batch * nf * bins * es
    rec = {"real": real, "input": "real" if real_input else "complex", "P": P, "T": T, "D": D, "length": length, "batch": batch,
           "frames": nf, "bins": bins, "bytes_in": bytes_in, "bytes_out": bytes_out, "default": default,
           "describe": {a: p.describe() for a, p in plans.items()}, "caller_inner": inner.describe(), "ms": t,
           "rel_l2_against_composed": agree, "over_caller": {a: med[a] / med["caller"] for a in plans}, "fused": fused,
           "algorithmic_tb_per_s": {a: (bytes_in + bytes_out) / (med[a] * 1e-3) / 1e12 for a in med}}
    del x, out, work, u, plans, arms, inner
    torch.cuda.empty_cache()
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default=default_shapes())
    ap.add_argument("--length", type=int, default=1 << 20)
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch

    if not torch.cuda.is_available():
        raise SystemExit("needs a GPU")
    import fourier_amd

    for shape in [s for s in args.shapes.split(",") if s]:
        real, kind, P, T, D = shape.split(":")
        r = run_case(torch, fourier_amd, real, kind == "r", int(P), int(T), int(D), args.length, args.batch, args.reps)
        print(json.dumps(r), flush=True)
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "a") as f:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
