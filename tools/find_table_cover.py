#!/usr/bin/env python3
"""Writes tests/golden/table_cover.json: the transform lengths through which tests/test_gpu_tables.py reaches every ahead-of-time tile-pass
kernel (kernels_regtile.cpp, kernels_tiled.cpp) in every role a default plan gives it.

  plain: rows (n, real, "AxB[xC]") -- for every menu length L and precision the smallest n whose default plan is "stockham mixed tiles" with L
         as its FIRST pass, and the smallest with L as its LAST pass.  Candidates are the products of two menu lengths, ascending; products of
         three (up to MAX_TRIPLE points) only for what no product of two reaches.
  blu:   rows (n, real, "M=... inner mixed tiles L1xL2") -- for every length of the Bluestein menu (64 ... 512 points) the smallest Bluestein
         length n whose default plan takes it as L1 (chirp-in and chirp-out pass) and the smallest that takes it as L2 (conv pass).  Candidates come
         from a restatement of BluTiledEngine::choose_m and of the rule "where it pays" (plan.h: init_bluestein), applied to every length with a
         prime factor above 13 up to 2^17.
  *_unreached: the (length, real, role) no candidate reached -- the test lists each of them with its reason.

Needs a GPU: every row is what describe() of a freshly created default plan says (FOURIER_HIP_SPECIALISE=0, as in the suite).  Creates plans
and reads their descriptions; launches no kernel.  Regenerate after a change to a menu or to the planner's rules:

    python tools/find_table_cover.py [--out tests/golden/table_cover.json]"""
import argparse
import bisect
import json
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
os.environ.setdefault("FOURIER_HIP_SPECIALISE", "0")

import kernel_tables as kt  # noqa: E402

MAX_TRIPLE = 2_500_000
REALS = ("f32", "f64")
_PRODUCTS = {}


def reg_tile_shape(L, real):
    """(r1, r2) of mixed_schedule.h: reg_tile_shape, (0, 0) where the length has no register-tile kernel in the precision"""
    max_factor = 40 if (real == "f32" and L > 512) else 32
    r2 = 0
    b = 2
    while b * b <= L:
        if L % b == 0 and L // b <= max_factor:
            r2 = b
        b += 1
    if r2 == 0 or L // r2 > 4 * r2:
        return 0, 0
    return L // r2, r2


def blu_menu(real):
    return [L for L in kt.tile_lengths()[0] if reg_tile_shape(L, real)[0]]


def choose_m(n, real, menu):
    """BluTiledEngine::choose_m (engine_tiled.h): (M, L1, L2) or (0, 0, 0)"""
    key = (real, tuple(menu))
    if key not in _PRODUCTS:  # every L1 x L2, L1 >= L2, by product; the loops of choose_m visit them in (L1, L2) order
        _PRODUCTS[key] = sorted((a * b, a, b) for a in menu for b in menu if b <= a)
    products = _PRODUCTS[key]
    need = 2 * n - 1
    lo = bisect.bisect_left(products, (need, 0, 0))
    if lo == len(products):
        return 0, 0, 0
    smallest = products[lo][0]
    hi = lo
    while hi < len(products) and products[hi][0] * 100 <= smallest * 104:
        hi += 1
    window = sorted(products[lo:hi], key=lambda p: (p[1], p[2]))

    def imbalance(L):
        r1, r2 = reg_tile_shape(L, real)
        return r1 / r2

    best, best_score, l1, l2 = 0, 0.0, 0, 0
    for relaxed in (False, True):  # the two lengths within a factor two of each other, if there is such a pair
        if best:
            break
        for m, a, b in window:
            if a > 2 * b and not relaxed:
                continue
            score = m * (1.0 + 0.10 * (imbalance(b) - 1.0) + 0.03 * (imbalance(a) - 1.0))
            if best == 0 or score < best_score:
                best, best_score, l1, l2 = m, score, a, b
    return best, l1, l2


def smooth_m_pays(n, real, menu):
    """plan.h: init_bluestein -- the product of two tile lengths a default plan of a Bluestein length n takes, or None"""
    m_pow2 = 1
    while m_pow2 < 2 * n - 1:
        m_pow2 <<= 1
    if m_pow2 <= (1 << (15 if real == "f32" else 14)):
        return None
    ms, l1, l2 = choose_m(n, real, menu)
    if ms and (8 * ms <= 5 * m_pow2 or (real == "f64" and 36 * ms <= 25 * m_pow2 and l2 <= 336)):
        return ms, l1, l2
    return None


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--out", default=kt.COVER_PATH)
    args = ap.parse_args()

    import fourier_amd as fa

    def describe(n, real):
        return (fa.create_fft_f32 if real == "f32" else fa.create_fft_f64)(n).describe()

    short, long_ = kt.tile_lengths()
    menu = short + long_
    cover = {"plain": [], "plain_unreached": [], "blu": [], "blu_unreached": []}
    created = 0

    # ---- plain passes ----
    for real in REALS:
        first, last = {}, {}  # length -> (n, passes, ragged)
        width = 16 if real == "f32" else 8  # columns of a 128-byte row segment

        def settled(found, L, n):  # a ragged plan found, or none up to what a partner of 105 instead of 64 points gives
            return L in found and (found[L][2] or n > found[L][0] * 105 // 64)

        def visit(cands):  # {n: [(first, last), ...]}
            nonlocal created
            for n in sorted(cands):
                if all(settled(first, a, n) and settled(last, c, n) for a, c in cands[n]):
                    continue
                d = describe(n, real)
                created += 1
                m = re.match(r"stockham mixed tiles (\d+(?:x\d+)+) ", d)
                if not m or "specialised" in d:
                    continue
                lens = [int(v) for v in m.group(1).split("x")]
                # the pass's column count (engine_tiled.h: run) off a multiple of the tile width: its last tile of every row is ragged
                for found, L in ((first, lens[0]), (last, lens[-1])):
                    ragged = (n // L) % width != 0
                    if L not in found or (ragged and not settled(found, L, n)):
                        found[L] = (n, m.group(1), ragged)

        pairs = {}
        for a in menu:
            for b in menu:
                if b <= a and a * b >= 4096:
                    pairs.setdefault(a * b, []).append((a, b))
        visit(pairs)
        triples = {}
        for a in menu:
            for b in menu:
                for c in menu:
                    if c <= b <= a and a * b * c <= MAX_TRIPLE and (a not in first or c not in last):
                        triples.setdefault(a * b * c, []).append((a, c))
        visit(triples)
        rows = {}
        for role, found in (("first", first), ("last", last)):
            for L in menu:
                if L in found:
                    rows.setdefault(found[L][:2], []).append(f"{role} {L}")
                else:
                    cover["plain_unreached"].append([L, real, role])
        for (n, passes), why in sorted(rows.items()):
            cover["plain"].append([n, real, passes])
        print(f"plain {real}: {len(rows)} lengths cover {len(first)} first and {len(last)} last passes of {len(menu)}", flush=True)

    # ---- Bluestein roles ----
    for real in REALS:
        bm = blu_menu(real)
        want1, want2 = {}, {}  # length -> [(n, M, l1, l2), ...] ascending in n
        for n in range(4097, (1 << 17) + 1):
            if kt.is_smooth(n):
                continue  # (a direct route; Bluestein lengths have a prime factor above 13)
            got = smooth_m_pays(n, real, bm)
            if got:
                want1.setdefault(got[1], []).append((n,) + got)
                want2.setdefault(got[2], []).append((n,) + got)
        rows, have1, have2 = {}, set(), set()
        for role, want, have in (("L1", want1, have1), ("L2", want2, have2)):
            for L in bm:
                for n, ms, l1, l2 in want.get(L, [])[:8]:  # the model's smallest lengths, until describe() agrees
                    d = describe(n, real)
                    created += 1
                    desc = f"M={ms} inner mixed tiles {l1}x{l2}"
                    if d.startswith("bluestein " + desc + " "):
                        rows.setdefault((n, desc), []).append(f"{role} {L}")
                        have.add(L)
                        break
                    print(f"model and plan disagree: n={n} {real} model '{desc}' plan '{d}'", flush=True)
                if L not in have:
                    cover["blu_unreached"].append([L, real, role])
        for L in short:
            if L not in bm:
                cover["blu_unreached"] += [[L, real, "L1"], [L, real, "L2"]]
        for (n, desc), why in sorted(rows.items()):
            cover["blu"].append([n, real, desc])
        print(f"blu {real}: {len(rows)} lengths cover {len(have1)} L1 and {len(have2)} L2 of {len(bm)} (+{len(short) - len(bm)} without kernels)", flush=True)

    for key in cover:
        cover[key].sort(key=lambda r: (r[1], r[0], str(r[2])))
    with open(args.out, "w") as f:
        f.write("{\n" + ",\n".join(f' "{k}": [\n' + ",\n".join("  " + json.dumps(r) for r in v) + "\n ]" for k, v in cover.items()) + "\n}\n")
    print(f"{created} plans created; wrote {args.out}", flush=True)


if __name__ == "__main__":
    main()
