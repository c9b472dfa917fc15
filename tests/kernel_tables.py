"""The engine's two ahead-of-time kernel tables as Python data, parsed from the sources that instantiate them: the register-stage rows of
fourier_amd/csrc/regfft_shapes.h (kernels_regfft.cpp) and the tile-pass menus of kernels_regtile.cpp / kernels_tiled.cpp.  Shared by
tests/test_kernel_tables.py (CPU), tests/test_gpu_tables.py and tools/find_table_cover.py."""
import collections
import json
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "fourier_amd", "csrc")
COVER_PATH = os.path.join(ROOT, "tests", "golden", "table_cover.json")

RegRow = collections.namedtuple("RegRow", "n r1 r2 r3 f32 f64 emu on_request")


def _read(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


def regfft_rows():
    """Every FOURIER_REGFFT_ROW / FOURIER_REGFFT_OPT_ROW of regfft_shapes.h, in file order."""
    return [RegRow(*(int(v) for v in m.groups()[1:]), on_request=bool(m.group(1)))
            for m in re.finditer(r"^FOURIER_REGFFT_(OPT_)?ROW\((\d+), (\d+), (\d+), (\d+), (\d+), (\d+), (\d+)\)\s*$", _read("regfft_shapes.h"), re.M)]


def regfft_row_lines():
    """The number of lines of regfft_shapes.h that start a row macro: equal to len(regfft_rows()) unless a row has a form the parser misses."""
    return len(re.findall(r"^FOURIER_REGFFT_\w*ROW\(", _read("regfft_shapes.h"), re.M))


def regfft_counts():
    """The header's own count lines: ((lengths, f32, f64) of the default rows, (lengths, f32, f64) of the rows on request)."""
    text = _read("regfft_shapes.h")
    a = re.search(r"^// (\d+) lengths: (\d+) in f32, (\d+) in f64", text, re.M)
    b = re.search(r"^// on request \(plan option \"register_stages\"\): (\d+) lengths 2\^a 3\^b, (\d+) in f32, (\d+) in f64", text, re.M)
    return tuple(int(v) for v in a.groups()), tuple(int(v) for v in b.groups())


def shape(row):
    return f"{row.r1}x{row.r2}" + (f"x{row.r3}" if row.r3 else "")


def flag(row, real):
    return row.f32 if real == "f32" else row.f64


def _shards(name):
    """{shard: [(macro, length), ...]} of a tile-kernel translation unit: the FOURIER_TILED / FOURIER_LONG uses after the #define lines"""
    out, shard = {}, None
    for line in _read(name).splitlines():
        m = re.match(r"#(?:if|elif) FOURIER_TILED_SHARD == (\d+)", line)
        if m:
            shard = int(m.group(1))
        elif line.startswith("#else"):
            shard = max(out) + 1
        elif line.startswith("#endif"):
            shard = None
        elif shard is not None and not line.startswith("#"):
            out.setdefault(shard, []).extend((k, int(v)) for k, v in re.findall(r"FOURIER_(TILED|LONG)\((\d+)\)", line))
    return out


def regtile_menu():
    """kernels_regtile.cpp: ({shard: lengths under FOURIER_TILED}, {shard: lengths under FOURIER_LONG})"""
    s = _shards("kernels_regtile.cpp")
    return ({i: [v for k, v in rows if k == "TILED"] for i, rows in s.items()}, {i: [v for k, v in rows if k == "LONG"] for i, rows in s.items()})


def lds_tile_menu():
    """kernels_tiled.cpp: {shard: lengths}"""
    return {i: [v for _, v in rows] for i, rows in _shards("kernels_tiled.cpp").items()}


def tile_lengths():
    """(the lengths of 64 ... 512 points, the lengths of 513 ... 1024 points), ascending"""
    short, long_ = regtile_menu()
    return sorted(v for rows in short.values() for v in rows), sorted(v for rows in long_.values() for v in rows)


def is_smooth(n, primes=(2, 3, 5, 7, 11, 13)):
    for p in primes:
        while n % p == 0:
            n //= p
    return n == 1


def load_cover():
    with open(COVER_PATH) as f:
        return json.load(f)
