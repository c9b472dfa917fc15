#!/usr/bin/env python3
"""The polyphase synthesis bank handle (fourier_hip_ipfb_*) against what a caller wrote before it, on the GPU.

  python tools/ipfb_bench.py [--shapes f32:c:256:4:256,...] [--length 1048576] [--batch 64] [--reps 5] [--out FILE]
      One JSON line per shape (precision : c|r for complex | real output rows : P : T : D): `batch` rows of about `length` values (the
      frames that fit: 1 + (length - P T) / D of them, the row they give in full) under the sinc-Hamming prototype (pfb_prototype).
      The default shapes are the analysis bench's: f32 and f64, complex and real rows, P in {256, 1024}, T in {4, 8}, D = P and 3 P / 4.
      HIP-event milliseconds per call (median / min / max over alternating repetitions on shared buffers, one process) of the arms
        handle    Ipfb.inverse (the one route, "ipfb composed")
        caller    torch: torch.fft.ifft / irfft of every frame, the frames tiled T times and multiplied by g into a materialised
                  (batch, frames, P T) array, then torch.nn.functional.fold on the real view (D = P: a reshape-sum over the T
                  shifted blocks instead); preallocated buffers where torch takes them
      every arm's spread (max - min) / median, the handle over the caller, and TB/s of each arm on the ALGORITHMIC bytes: the frames in
      once, the samples out once.  Both arms give the same rows within the test tolerance, asserted before anything is timed.
      Nothing is gated on these numbers: the handle has one route.
  A shape is one step: run each group under its own time limit, e.g.  timeout -k 10 300 python tools/ipfb_bench.py --shapes ... --out ..."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def default_shapes():
    return ",".join(f"{real}:{kind}:{P}:{T}:{D}" for real in ("f32", "f64") for kind in ("c", "r") for P in (256, 1024) for T in (4, 8)
                    for D in (P, 3 * P // 4))


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


def caller_arm(torch, Y, g, P, T, D, real_output, out):
    """the composition in torch, into `out`"""
    batch, nf = Y.shape[:2]
    full = (nf - 1) * D + P * T
    work = torch.empty(batch, nf, T, P, dtype=out.dtype, device=Y.device)
    gt = g.view(1, 1, T, P)

    def run():
        v = torch.fft.irfft(Y, n=P) if real_output else torch.fft.ifft(Y)
        torch.mul(v.unsqueeze(2), gt, out=work)  # frame f's P T weighted values g[t P + n] v[f, n]
        if D == P:  # block j of the row is the sum of the frames' blocks t of frame j - t
            blocks = out.view(batch, nf + T - 1, P)
            blocks.zero_()
            for t in range(T):
                blocks[:, t: t + nf] += work[:, :, t]
            return
        if real_output:
            cols = work.view(batch, nf, P * T).transpose(1, 2)  # (batch, P T, frames)
            y = torch.nn.functional.fold(cols, (full, 1), (P * T, 1), stride=(D, 1))
            out.copy_(y.view(batch, full))
        else:
            cols = torch.view_as_real(work.view(batch, nf, P * T)).permute(0, 3, 2, 1).reshape(batch, 2 * P * T, nf)
            y = torch.nn.functional.fold(cols, (full, 1), (P * T, 1), stride=(D, 1))  # (batch, 2, full, 1)
            torch.view_as_real(out).copy_(y.view(batch, 2, full).permute(0, 2, 1))

    return run


def run_case(torch, fa, real, real_output, P, T, D, length, batch, reps):
    rdt, cdt = (torch.float32, torch.complex64) if real == "f32" else (torch.float64, torch.complex128)
    es = 8 if real == "f32" else 16
    nf = 1 + (length - P * T) // D
    bins = P // 2 + 1 if real_output else P
    Y = torch.view_as_complex(torch.randn(batch, nf, bins, 2, dtype=rdt, device="cuda"))
    g = fa.pfb_prototype(P, T, rdt).cuda()
    plan = fa.Ipfb(P, T, real, D, real_output, 0)
    plan.set_filter(g)
    plan.reserve(nf, batch)
    full = plan.length(nf)
    odt = rdt if real_output else cdt
    out_h = torch.empty(batch, full, dtype=odt, device="cuda")
    out_c = torch.empty(batch, full, dtype=odt, device="cuda")
    arms = {"handle": lambda: plan.inverse(Y, out=out_h), "caller": caller_arm(torch, Y, g, P, T, D, real_output, out_c)}
    # the arms agree before they are timed: the tests' tolerance, a transform plus one more rounding stage
    for f in arms.values():
        f()
    torch.cuda.synchronize()
    agree = float((out_h - out_c).norm() / out_c.norm())
    bound = 2 * (2e-6 if real == "f32" else 1e-13)
    assert agree <= bound, (real, real_output, P, T, D, agree, bound)
    t = time_arms(torch, arms, reps)
    med = {a: v["median_ms"] for a, v in t.items()}
    bytes_in = batch * nf * bins * es
    bytes_out = batch * full * (es // 2 if real_output else es)
    rec = {"real": real, "output": "real" if real_output else "complex", "P": P, "T": T, "D": D, "length": full, "batch": batch,
           "frames": nf, "bins": bins, "cover": -(-P * T // D), "bytes_in": bytes_in, "bytes_out": bytes_out,
           "describe": plan.describe(), "ms": t, "rel_l2_handle_against_caller": agree, "handle_over_caller": med["handle"] / med["caller"],
           "algorithmic_tb_per_s": {a: (bytes_in + bytes_out) / (med[a] * 1e-3) / 1e12 for a in med}}
    del Y, out_h, out_c, plan, arms
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
